"""xrsfm_ba_detect_keypoints without a GPU: the interface (exports, struct layout, defaults, every EINVAL with untouched outputs, the
empty call, ENODEV), the taps and the octave geometry, the yardstick's own checks (the float32 restatement within every bar, the
catalogue covers what DESIGN.md 5m promises), ba_sift_rule.h on the host as a stand-alone program built with the address and
undefined-behaviour sanitizers, and the kernels' register / LDS / scratch figures."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import sift_host_driver as H
from tests import sift_yardstick as Y

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("xrsfm_ba_sift_options_default", "xrsfm_ba_detect_keypoints", "xrsfm_ba_debug_sift_taps", "xrsfm_ba_debug_sift_levels",
         "xrsfm_ba_debug_sift_offsets")
SMALL = ("a44x40", "b50x33", "c64x48", "c64x48_o0", "d64x48", "budget20", "budget60")


def test_exports_and_struct_layout(lib, tmp_path):
    from xrsfm_amd import capi
    hdr = open(os.path.join(ROOT, "include", "xrsfm_ba.h")).read()
    for name in NAMES:
        assert name in capi.EXPORTS and getattr(lib, name) is not None and re.search(r"\b%s\s*\(" % name, hdr)
    fields = [f for f, _ in capi.CSiftOptions._fields_]
    src = tmp_path / "p.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "xrsfm_ba.h"\nint main(){printf("%zu", sizeof(xrsfm_ba_sift_options));\n' +
                   "".join('printf(" %%zu", offsetof(xrsfm_ba_sift_options, %s));\n' % f for f in fields) +
                   'printf(" %d %d\\n", XRSFM_BA_SIFT_MAX_TAPS, XRSFM_BA_SIFT_MAX_OCTAVES);return 0;}\n')
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "p")], check=True)
    out = [int(x) for x in subprocess.run([str(tmp_path / "p")], capture_output=True, text=True, check=True).stdout.split()]
    o = capi.CSiftOptions
    assert out == [C.sizeof(o)] + [getattr(o, f).offset for f in fields] + [capi.SIFT_MAX_TAPS, capi.SIFT_MAX_OCTAVES]


def test_default_options_are_the_reference_values(lib):
    from xrsfm_amd import capi
    o = capi.sift_options()
    assert (o.first_octave, o.num_octaves, o.peak_threshold, o.edge_threshold, o.max_num_features, o.max_image_size) == \
        (-1, 4, np.float32(0.02) / np.float32(3), 10.0, 8192, 3200)
    assert {k: getattr(o, k) for k in Y.DEFAULTS} == Y.DEFAULTS
    assert capi.sift_options(first_octave=0, max_num_features=20).max_num_features == 20
    with pytest.raises(AttributeError):
        capi.sift_options(no_such_field=1)


class _Call:
    """A small valid call and sentinel-filled outputs for the raw C entry."""
    def __init__(self):
        self.images = [np.ascontiguousarray(Y.image(k)) for k in ("a44x40", "b50x33")]
        self.n = 2
        self.w = np.array([a.shape[1] for a in self.images], np.int32)
        self.h = np.array([a.shape[0] for a in self.images], np.int32)
        self.ptr = np.zeros(3, np.int64)
        self.ptr[1:] = np.cumsum([a.size for a in self.images])
        self.pix = np.concatenate([a.ravel() for a in self.images])
        self.cap = 500
        self.out = dict(kp=np.full(3, -77, np.int64), k=np.full((500, 4), -77, np.float32), l=np.full((500, 4), -77, np.int32), s=np.full(500, -77, np.int8),
                        lc=np.full((2, 12), -77, np.int32))

    def untouched(self):
        return all(np.all(v == -77) for v in self.out.values())

    def run(self, lib, opt, null=()):
        p = lambda a, t: a.ctypes.data_as(C.POINTER(t))
        o = self.out
        a = dict(opt=C.byref(opt) if opt is not None else None, w=p(self.w, C.c_int32), h=p(self.h, C.c_int32), ptr=p(self.ptr, C.c_int64), pix=p(self.pix, C.c_uint8),
                 kp=p(o["kp"], C.c_int64), k=p(o["k"], C.c_float), l=p(o["l"], C.c_int32), s=p(o["s"], C.c_int8), lc=p(o["lc"], C.c_int32))
        for k in null:
            a[k] = None
        return lib.xrsfm_ba_detect_keypoints(a["opt"], self.n, a["w"], a["h"], a["ptr"], a["pix"], self.cap, a["kp"], a["k"], a["l"], a["s"], a["lc"])


def _einval_cases():
    def opt(**kw):
        return lambda c, o: [setattr(o, k, v) for k, v in kw.items()]

    def field(name, fn):
        return lambda c, o: fn(getattr(c, name))
    return {
        "null_opt": None, "null_width": ("w",), "null_height": ("h",), "null_pixel_ptr": ("ptr",), "null_pixels": ("pix",), "null_key_ptr": ("kp",),
        "null_keys": ("k",), "null_loc": ("l",), "null_sign": ("s",),
        "negative_images": lambda c, o: setattr(c, "n", -1), "negative_capacity": lambda c, o: setattr(c, "cap", -1),
        "width_truncates_below_16": field("w", lambda w: w.__setitem__(0, 19)), "height_below_16": field("h", lambda h: h.__setitem__(1, 15)),
        "negative_width": field("w", lambda w: w.__setitem__(0, -44)),
        "side_above_max": opt(max_image_size=49), "max_image_size_zero": opt(max_image_size=0),
        "ptr_not_from_zero": field("ptr", lambda p: p.__setitem__(0, 1)), "ptr_disagrees": field("ptr", lambda p: p.__setitem__(1, int(p[1]) - 1)),
        "first_octave_low": opt(first_octave=-2), "first_octave_high": opt(first_octave=1),
        "octaves_zero": opt(num_octaves=0), "octaves_nine": opt(num_octaves=9),
        "peak_zero": opt(peak_threshold=0.0), "peak_negative": opt(peak_threshold=-0.01), "peak_nan": opt(peak_threshold=float("nan")),
        "edge_zero": opt(edge_threshold=0.0), "edge_inf": opt(edge_threshold=float("inf")),
        "features_zero": opt(max_num_features=0), "features_negative": opt(max_num_features=-3),
    }


@pytest.mark.parametrize("name", sorted(_einval_cases()))
def test_einval_without_a_device_and_outputs_untouched(lib, name, capfd):
    from xrsfm_amd import capi
    how = _einval_cases()[name]
    c, o = _Call(), capi.sift_options()
    if how is None:
        code = c.run(lib, None)
    elif isinstance(how, tuple):
        code = c.run(lib, o, null=how)
    else:
        how(c, o)
        code = c.run(lib, o)
    assert code == capi.EINVAL
    assert c.untouched()
    err = capfd.readouterr().err
    assert err.count("\n") == 1 and "xrsfm_ba_detect_keypoints" in err


def test_no_images_is_success_without_a_device(lib):
    from xrsfm_amd import capi
    c = _Call()
    c.n = 0
    assert c.run(lib, capi.sift_options()) == 0 and c.untouched()
    assert c.run(lib, capi.sift_options(), null=("w", "h", "ptr", "pix", "kp", "k", "l", "s", "lc")) == 0
    assert capi.detect_keypoints([]) == []


def test_valid_call_without_a_device_is_enodev(lib):
    import torch
    from xrsfm_amd import capi
    if torch.cuda.is_available() and capi.device_count() > 0:
        pytest.skip("a GPU is present")
    c = _Call()
    assert c.run(lib, capi.sift_options()) == -2 and c.untouched()
    assert c.run(lib, capi.sift_options(), null=("lc",)) == -2 and c.untouched()
    with pytest.raises(RuntimeError, match="ENODEV"):
        capi.detect_keypoints(c.images)
    with pytest.raises(RuntimeError, match="ENODEV"):
        capi.debug_sift_levels(c.images[0], 0)
    with pytest.raises(RuntimeError, match="ENODEV"):
        capi.debug_sift_offsets(c.images[0])
    with pytest.raises(ValueError):
        capi.debug_sift_levels(c.images[0], 3)
    with pytest.raises(ValueError):
        capi.detect_keypoints([np.zeros((20, 20), np.float32)])


def test_taps_bit_for_bit(lib):
    """the five level filters and the initial smoothing of both first_octave values: seven sigmas"""
    from xrsfm_amd import capi
    sig = [float(s) for s in Y.params(-1)["level_sigma"]] + [float(Y.params(-1)["init_sigma"]), float(Y.params(0)["init_sigma"])]
    assert len(set(sig)) == 7 and abs(sig[5] - 1.249) < 1e-3 and abs(sig[6] - 1.520) < 1e-3
    widths = []
    for s in sig:
        got, want = capi.debug_sift_taps(s), Y.taps(s)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), s
        assert abs(float(got.astype(np.float64).sum()) - 1.0) < 4 * Y.EPS * len(got) and np.array_equal(got, got[::-1])
        widths.append(len(got))
    assert widths == [11, 13, 17, 21, 25, 11, 13]
    assert len(capi.debug_sift_taps(0.3)) == 5 and len(capi.debug_sift_taps(9.0)) == 33
    assert lib.xrsfm_ba_debug_sift_taps(1.0, None, None) == capi.EINVAL
    t, w = np.zeros(33, np.float32), C.c_int32(0)
    assert lib.xrsfm_ba_debug_sift_taps(-1.0, t.ctypes.data_as(C.POINTER(C.c_float)), C.byref(w)) == capi.EINVAL


GEOMETRY = {
    (44, 40, -1, 4): [(88, 80), (44, 40), (24, 20)],
    (50, 33, 0, 4): [(48, 33), (24, 16)],
    (64, 48, -1, 4): [(128, 96), (64, 48), (32, 24)],
    (64, 48, 0, 4): [(64, 48), (32, 24)],
    (300, 260, -1, 4): [(600, 520), (300, 260), (152, 130), (76, 65)],
    (96, 80, -1, 4): [(192, 160), (96, 80), (48, 40), (24, 20)],
    (19, 16, 0, 4): [(16, 16)],
    (1024, 768, -1, 4): [(2048, 1536), (1024, 768), (512, 384), (256, 192)],
    (1024, 768, -1, 8): [(2048, 1536), (1024, 768), (512, 384), (256, 192), (128, 96), (64, 48), (32, 24)],
    (3200, 2400, -1, 2): [(6400, 4800), (3200, 2400)],
    (1023, 37, 0, 4): [(1020, 37), (512, 18)],
}


@pytest.fixture(scope="module")
def rule_program(tmp_path_factory):
    """the stand-alone program around xsift::geometry and xsift::key_decide, built with the sanitizers"""
    d = tmp_path_factory.mktemp("sift_rule")
    return H.build(d, name="sift_rule", text=H.RULE_DRIVER), d


def test_octave_geometry(lib, rule_program):
    """the table through the yardstick, the ctypes helper that sizes the buffers of debug_sift_levels, and xsift::geometry itself"""
    from xrsfm_amd import capi
    exe, d = rule_program
    none = np.zeros((0, 3, 3), np.float32)
    got, _ = H.run_rule(exe, d, list(GEOMETRY), none, none, none, np.zeros((0, 3), np.float32))
    for ((w, h, fo, no), want), (w_in, h_in, octaves) in zip(GEOMETRY.items(), got):
        assert Y.geometry(w, h, fo, no) == want, (w, h, fo, no)
        assert capi.sift_geometry(w, h, capi.sift_options(first_octave=fo, num_octaves=no)) == want
        assert (w_in, h_in) == (w & ~3, h) and octaves == want, (w, h, fo, no, octaves)


# ---------------------------------------------------------------------------------------------------- the yardstick itself
def _within_bars(levels, ref):
    """levels: [(G, D)] of a tested implementation; -> worst ratio of a deviation to its bar"""
    worst = 0.0
    for (G, D), (Gr, Dr), (gb, db) in zip(levels, ref["pyramid"], ref["bars"]):
        for i in range(6):
            worst = max(worst, float(np.abs(G[i].astype(np.longdouble) - Gr[i]).max()) / gb[i])
        for j in range(5):
            worst = max(worst, float(np.abs(D[j].astype(np.longdouble) - Dr[j]).max()) / db[j])
    return worst


def test_float32_restatement_is_within_every_bar():
    union = fragile = 0
    for name in Y.CATALOGUE:
        a, b = Y.catalogue_reference(name, True), Y.catalogue_reference(name, False)
        assert len(a["pyramid"]) == len(b["pyramid"]) and _within_bars(b["pyramid"], a) <= 1.0, name
        mism, u, f = Y.compare(Y.pre_budget_levels(b), a)
        assert mism == [], (name, mism[:5])
        union, fragile = union + u, fragile + f
        n, worst = Y.check_values(b["loc"], b["off"], b["keys"], a)
        assert n >= 0.9 * len(a["loc"]) and worst <= 1.0 / 16.0 + 1e-12, (name, n, worst)
    assert union >= 1000 and fragile <= 0.05 * union, (union, fragile)
    dev = Y.measured_deviation()
    print("measured deviation of the float32 restatement:", dev, "union", union, "fragile", fragile)
    assert 1e-6 < dev["off"] < 1e-2 and dev["gauss"] < 1e-6 and dev["dog"] < 1e-6


def _hand_neighbourhood(kind):
    """3 x 3 x 3 neighbourhoods for the branches no catalogue image produces"""
    P, Cc, N = (np.zeros((3, 3), np.float32) for _ in range(3))
    # With the thresholds of the reference no float32 neighbourhood reaches a guard: a pixel above 0.8 * 0.02 / 3 that passes the edge
    # test has |fxx| of at least its own last bit, about 5e-10.  With a threshold of 1e-12 these three do, one per guard:
    if kind == "guard_first":
        Cc[1, 1] = 1e-11                            # the largest pivot candidate is |fxx| = 2e-11 < 1e-10
    if kind == "guard_second":
        Cc[1, 1] = 2e-10; Cc[0, 1] = Cc[2, 1] = 1.7e-10         # fxx = -4e-10 is the pivot, then |fyy| = 6e-11 < 1e-10 (and the edge test passes)
    if kind == "guard_third":
        Cc[1, 1] = 1e-9; P[1, 1] = N[1, 1] = 1e-9 - 2e-11       # fxx = fyy = -2e-9, then |fss| = 4e-11 < 1e-10
    if kind == "tie_min":
        # a minimum whose value is met again in the next level: v == nmin passes READ_CMP_DOG_DATA on the minimum side
        Cc[:] = -0.01; Cc[1, 1] = -0.03; P[:] = -0.01; N[:] = -0.01; N[0, 0] = -0.03
    if kind == "tie_max_last_row":
        # a maximum tied in the very last row read passes, and is signed -1 (the reference's v > nmax is false)
        Cc[:] = 0.01; Cc[1, 1] = 0.03; P[:] = 0.01; N[:] = 0.01; N[2, 2] = 0.03
    if kind == "tie_max_earlier":
        # the same tie one row earlier moves the pixel to the minimum side, where the next row rejects it
        Cc[:] = 0.01; Cc[1, 1] = 0.03; P[:] = 0.01; N[:] = 0.01; N[1, 2] = 0.03
    return P, Cc, N


HAND = ("guard_first", "guard_second", "guard_third", "tie_min", "tie_max_last_row", "tie_max_earlier")
# kind -> (sign, why) under the thresholds (8e-13, 1e-12) and under the reference's; the offsets are 0 in every case: a kept guard
# leaves them 0, and the ties are symmetric
HAND_WANT = {
    "guard_first": ((1, "kept_guard"), (0, "threshold")), "guard_second": ((1, "kept_guard"), (0, "threshold")),
    "guard_third": ((1, "kept_guard"), (0, "threshold")),
    "tie_min": ((-1, "kept"), (-1, "kept")), "tie_max_last_row": ((-1, "kept"), (-1, "kept")),
    "tie_max_earlier": ((0, "neighbour"), (0, "neighbour")),
}


def test_hand_built_neighbourhoods(rule_program):
    """the guard-tripped keep (each of the three guards) and the ties, through xsift::key_decide of ba_sift_rule.h (a stand-alone
    program under the sanitizers) and through both precisions of the yardstick, under the 1e-12 thresholds and the reference's"""
    exe, d = rule_program
    p = Y.params(-1)
    th = [(np.float32(8e-13), np.float32(1e-12), p["E"]), (p["T0"], p["T"], p["E"])]
    items = [(kind, t) for kind in HAND for t in (0, 1)]
    Pn, Cn, Nn = (np.stack([_hand_neighbourhood(kind)[q] for kind, _ in items]) for q in range(3))
    _, got = H.run_rule(exe, d, [], Pn, Cn, Nn, np.array([th[t] for _, t in items], np.float32))
    for k, (kind, t) in enumerate(items):
        sign, why = HAND_WANT[kind][t]
        assert (got["sign"][k], Y.WHY[got["why"][k]]) == (sign, why), (kind, t, got["sign"][k], Y.WHY[got["why"][k]])
        assert (abs(got["dx"][k]), abs(got["dy"][k]), abs(got["ds"][k])) == (0, 0, 0), (kind, t)
        for dt in (np.float32, np.longdouble):
            y = {f: v[0] for f, v in Y.decide(Pn[k:k + 1], Cn[k:k + 1], Nn[k:k + 1], *th[t], dt).items()}
            assert (y["sign"], Y.WHY[y["why"]]) == (sign, why) and (abs(y["dx"]), abs(y["dy"]), abs(y["ds"])) == (0, 0, 0), (kind, t, dt)


def test_key_decide_equals_the_float32_restatement_on_every_candidate(rule_program):
    """every pixel of the catalogue above the threshold, through xsift::key_decide: sign, offsets and the deciding branch equal the
    float32 restatement's bit for bit, and every branch an image can reach is taken on the C++ side"""
    exe, d = rule_program
    Pn, Cn, Nn, th, want = [], [], [], [], {k: [] for k in ("sign", "dx", "dy", "ds", "why")}
    for name in ("a44x40", "b50x33", "c64x48", "c64x48_o0", "d64x48", "e300x260"):
        ref, p = Y.catalogue_reference(name, False), Y.params(Y.CATALOGUE[name][4])
        for (o, j), r in ref["levels"].items():
            D = ref["pyramid"][o][1]
            for lst, lev in ((Pn, D[j]), (Cn, D[j + 1]), (Nn, D[j + 2])):
                lst.append(Y._gather(lev, r["rows"], r["cols"]))
            th.append(np.tile(np.array([p["T0"], p["T"], p["E"]], np.float32), (len(r["rows"]), 1)))
            for k in want:
                want[k].append(r[k])
    Pn, Cn, Nn, th = (np.concatenate(x) for x in (Pn, Cn, Nn, th))
    _, got = H.run_rule(exe, d, [], Pn, Cn, Nn, th)
    assert len(Cn) > 50000
    solved = np.isin(got["why"], (0, 6, 7, 8, 9))          # (a pixel rejected before the elimination has offsets 0 in the C++ text; the
    for k in want:                                         # vectorised restatement computes them for every lane)
        w = np.concatenate(want[k]).astype(got[k].dtype)
        assert np.array_equal(got[k], w) if k in ("sign", "why") else np.array_equal(got[k][solved], w[solved]) and np.all(got[k][~solved] == 0), k
    assert solved.sum() > 1000
    seen = {Y.WHY[k] for k in np.unique(got["why"])}
    assert seen == set(Y.WHY) - {"kept_guard", "threshold"}, seen          # (these pixels are above the threshold; the guards: hand-built)


def test_catalogue_coverage():
    e = Y.catalogue_reference("e300x260")
    assert e["geometry"] == GEOMETRY[(300, 260, -1, 4)]
    for o in range(4):
        for j in range(3):
            s = e["levels"][(o, j)]["sign"]
            assert (s > 0).any() and (s < 0).any(), (o, j)
    assert [Y.catalogue_reference(k)["geometry"] for k in ("a44x40", "b50x33")] == [GEOMETRY[(44, 40, -1, 4)], GEOMETRY[(50, 33, 0, 4)]]
    why = np.concatenate([r["why"] for name in Y.CATALOGUE for r in Y.catalogue_reference(name)["levels"].values()])
    seen = {Y.WHY[k] for k in np.unique(why)}
    assert {"kept", "threshold", "centre_row", "neighbour", "edge_det", "edge_ratio", "contrast", "off_ds", "off_dx", "off_dy"} <= seen, seen
    # each of |dx|, |dy|, |ds| >= 1 alone
    alone = set()
    for name in Y.CATALOGUE:
        for r in Y.catalogue_reference(name)["levels"].values():
            m = np.isin(r["why"], (7, 8, 9))
            big = np.stack([np.abs(r["ds"][m]) >= 1, np.abs(r["dx"][m]) >= 1, np.abs(r["dy"][m]) >= 1], -1)
            for row in big[big.sum(-1) == 1]:
                alone.add(int(np.argmax(row)))
    assert alone == {0, 1, 2}, alone
    # the budget: whole fine levels cut, and an overshoot
    b20, b60, full = (Y.catalogue_reference(k) for k in ("budget20", "budget60", "d64x48"))
    assert np.array_equal(b20["level_count"], full["level_count"]) and full["total"] == int(full["level_count"].sum()) == len(full["loc"])
    assert b20["take"][:3].tolist() == [False, False, True] and b20["total"] == int(full["level_count"][2]) > 20
    assert b60["take"][:3].tolist() == [False, True, True] and b60["total"] == int(full["level_count"][1:3].sum()) > 60
    assert set(b20["loc"][:, 1].tolist()) == {2} and len(b20["loc"]) == b20["total"]


# ---------------------------------------------------------------------------------------------------- the header on the host
@pytest.fixture(scope="module")
def host_results(tmp_path_factory):
    d = tmp_path_factory.mktemp("sift_host")
    exe = H.build(d)
    names = list(SMALL) + ["e300x260"]
    res = H.run(exe, d, [Y.image(k) for k in names], [Y.entry_options(k) for k in names])
    return dict(zip(names, res))


def test_rule_header_parameters_equal_the_yardsticks(host_results):
    for name, fo in (("a44x40", -1), ("b50x33", 0)):
        p = Y.params(fo)
        want = np.array([p["sigma0"], p["step"], *p["level_sigma"], p["init_sigma"], *p["key_sigma"], p["T"], p["T0"], p["E"]], np.float32)
        assert np.array_equal(host_results[name]["params"].view(np.uint32), want.view(np.uint32)), (host_results[name]["params"], want)


def test_rule_header_on_the_host_reproduces_the_yardstick(host_results):
    """ba_sift_rule.h in a sequential program under the sanitizers: levels within the bars, key / no key and sign equal on every
    non-fragile pixel, offsets and values within 16 times the restatement's own deviation; against the float32 restatement, which
    rounds like this program (no contraction on the host), everything is equal bit for bit."""
    union = fragile = 0
    for name, got in host_results.items():
        a, b = Y.catalogue_reference(name, True), Y.catalogue_reference(name, False)
        assert got["geometry"] == a["geometry"]
        assert _within_bars(got["levels"], a) <= 1.0, name
        assert np.array_equal(got["level_count"], b["level_count"][:len(got["level_count"])]), name
        assert np.array_equal(got["loc"], b["loc"]) and np.array_equal(got["off"][:, 0].astype(np.int8), b["sign"]), name
        for (G, D), (Gb, Db) in zip(got["levels"], b["pyramid"]):
            assert np.array_equal(G, Gb) and np.array_equal(D, Db), name
        assert np.array_equal(got["off"][:, 1:], b["off"].astype(np.float32)), name
        mism, u, f = Y.compare(Y.levels_of(got["loc"], got["off"][:, 0]), a) if a["take"][:len(got["level_count"])].all() else ([], 0, 0)
        assert mism == [], (name, mism[:5])
        union, fragile = union + u, fragile + f
        n, worst = Y.check_values(got["loc"], got["off"][:, 1:], got["keys"], a)
        assert worst <= 1.0, (name, worst)
    assert union >= 1000 and fragile <= 0.05 * union


def test_sift_kernels_do_not_spill(tmp_path):
    """k_sift_base, k_sift_filter, k_sift_down and both k_sift_key of the gfx950 code object: no spilled register, no private
    (scratch) segment; the filter holds its two tiles in 40 KiB of LDS, the key test its three levels in under 27 KiB."""
    from xrsfm_amd import _build
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = tmp_path / "sift_only.hip"
    src.write_text('#include "ba_sift.h"\ntemplate __global__ void k_sift_key<false>(const SiftImg*, const SiftTile*, const float*, int, int, SiftKeyParams, int32_t*, const int32_t*, int32_t*, '
                   'float4*, int4*, float4*);\ntemplate __global__ void k_sift_key<true>(const SiftImg*, const SiftTile*, const float*, int, int, SiftKeyParams, '
                   'int32_t*, const int32_t*, int32_t*, float4*, int4*, float4*);\n')
    asm = tmp_path / "sift.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-I", _build.CSRC, str(src), "-o", str(asm)], check=True, capture_output=True)
    text = asm.read_text()
    seen = {}
    for blk in text.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        m = re.search(r"k_sift_(base|filter|down|key)", name)
        if not m:
            continue
        num = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, blk).group(1))
        fig = dict(vgpr=num("vgpr_count"), sgpr=num("sgpr_count"), lds=num("group_segment_fixed_size"), scratch=num("private_segment_fixed_size"), spill=num("vgpr_spill_count"))
        seen.setdefault(m.group(1), []).append(fig)
        assert fig["spill"] == 0 and fig["scratch"] == 0 and fig["vgpr"] <= 128, (name, fig)
    print("sift kernels:", seen)
    assert sorted(seen) == ["base", "down", "filter", "key"] and len(seen["key"]) == 2
    assert seen["filter"][0]["lds"] == 4 * (64 * 96 + 64 * 64) and all(k["lds"] <= 27 * 1024 for k in seen["key"])
    assert seen["base"][0]["lds"] == 0 and seen["down"][0]["lds"] == 0
