"""xrsfm_ba_match_descriptors without a GPU: the interface (exports, struct layout, defaults, every EINVAL with untouched outputs,
the empty call, ENODEV), the distance table, the capi helpers, the yardstick's own checks (its two formulations agree, the
catalogue covers what DESIGN.md 5l promises), ba_match_rule.h on the host as a stand-alone program built with the address and
undefined-behaviour sanitizers, and the kernels' register / scratch figures."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import match_host_driver as H
from tests import match_yardstick as Y

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("xrsfm_ba_match_options_default", "xrsfm_ba_match_descriptors", "xrsfm_ba_debug_match_table", "xrsfm_ba_debug_match_top2")


def test_exports_and_struct_layout(lib, tmp_path):
    from xrsfm_amd import capi
    hdr = open(os.path.join(ROOT, "include", "xrsfm_ba.h")).read()
    for name in NAMES:
        assert name in capi.EXPORTS + capi.EXPORTS_WITH_DIGITS and getattr(lib, name) is not None and re.search(r"\b%s\s*\(" % name, hdr)
    fields = [f for f, _ in capi.CMatchOptions._fields_]
    src = tmp_path / "p.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "xrsfm_ba.h"\nint main(){printf("%zu", sizeof(xrsfm_ba_match_options));\n' +
                   "".join('printf(" %%zu", offsetof(xrsfm_ba_match_options, %s));\n' % f for f in fields) +
                   'printf(" %d %d\\n", XRSFM_BA_MATCH_MAX_FEATURES, XRSFM_BA_MATCH_DIM);return 0;}\n')
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "p")], check=True)
    out = [int(x) for x in subprocess.run([str(tmp_path / "p")], capture_output=True, text=True, check=True).stdout.split()]
    o = capi.CMatchOptions
    assert out == [C.sizeof(o)] + [getattr(o, f).offset for f in fields] + [capi.MATCH_MAX_FEATURES, capi.MATCH_DIM]
    assert (capi.MATCH_MAX_FEATURES, capi.MATCH_DIM, capi.MATCH_TABLE_SIZE) == (Y.MAX_FEATURES, Y.DIM, Y.TAB_MAX + 1)


def test_default_options_are_the_reference_values(lib):
    from xrsfm_amd import capi
    o = capi.match_options()
    assert (o.max_distance, o.max_ratio, o.mutual_best, o.max_features) == (np.float32(0.7), np.float32(0.8), 1, 16384)
    assert Y.DEFAULTS == dict(max_distance=0.7, max_ratio=0.8, mutual_best=1, max_features=16384)
    assert capi.match_options(mutual_best=0, max_features=100).max_features == 100
    with pytest.raises(AttributeError):
        capi.match_options(no_such_field=1)


def test_table_equals_the_yardsticks_and_decreases(lib):
    """all 262 145 entries; and the three host formulations of the issue give the same table"""
    import math
    from xrsfm_amd import capi
    got, want = capi.debug_match_table(), Y.table()
    assert got.dtype == np.float32 and got.shape == (262145,) and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.all(np.diff(got.astype(np.float64)) < 0) and got[-1] == 0.0 and got[0] == np.float32(math.acos(0.0))
    x = (np.arange(Y.TAB_MAX + 1, dtype=np.float32) * np.float32(2.0 ** -18)).astype(np.float64)
    assert np.array_equal(np.arccos(np.minimum(x, 1.0)).astype(np.float32), want)
    assert all(np.float32(math.acos(min(float(x[d]), 1.0))) == want[d] for d in range(0, Y.TAB_MAX + 1, 997))
    assert lib.xrsfm_ba_debug_match_table(None) == capi.EINVAL


class _Call:
    """A small valid call and sentinel-filled outputs for the raw C entry."""
    def __init__(self):
        F = Y.frames()
        self.frames = [F[k] for k in (4, 16, 3)]              # 17, 17 and 16 descriptors
        self.ptr = np.zeros(4, np.int64)
        self.ptr[1:] = np.cumsum([len(f) for f in self.frames])
        self.desc = np.concatenate(self.frames)
        self.pa, self.pb = np.array([0, 1, 2], np.int32), np.array([1, 2, 2], np.int32)
        self.n_frames, self.n_pairs, self.cap = 3, 3, 50
        self.out = dict(mp=np.full(4, -77, np.int64), m=np.full((50, 2), -77, np.int32), nr=np.full(3, -77, np.int32), nc=np.full(3, -77, np.int32))

    def untouched(self):
        return all(np.all(v == -77) for v in self.out.values())

    def run(self, lib, opt, null=()):
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        lp = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
        o = self.out
        a = dict(opt=C.byref(opt) if opt is not None else None, ptr=lp(self.ptr), desc=self.desc.ctypes.data_as(C.POINTER(C.c_uint8)), pa=ip(self.pa),
                 pb=ip(self.pb), mp=lp(o["mp"]), m=ip(o["m"]), nr=ip(o["nr"]), nc=ip(o["nc"]))
        for k in null:
            a[k] = None
        return lib.xrsfm_ba_match_descriptors(a["opt"], self.n_frames, a["ptr"], a["desc"], self.n_pairs, a["pa"], a["pb"], self.cap, a["mp"], a["m"],
                                              a["nr"], a["nc"])


def _einval_cases():
    def opt(**kw):
        return lambda c, o: [setattr(o, k, v) for k, v in kw.items()]

    def field(name, fn):
        return lambda c, o: fn(getattr(c, name))
    return {
        "null_opt": None, "null_match_ptr": ("mp",), "null_matches": ("m",), "null_pair_a": ("pa",), "null_pair_b": ("pb",), "null_desc_ptr": ("ptr",),
        "null_desc": ("desc",),
        "negative_pairs": lambda c, o: setattr(c, "n_pairs", -1), "negative_frames": lambda c, o: setattr(c, "n_frames", -1),
        "negative_capacity": lambda c, o: setattr(c, "cap", -1),
        "ptr_not_from_zero": field("ptr", lambda p: p.__setitem__(0, 1)), "ptr_decreasing": field("ptr", lambda p: p.__setitem__(2, int(p[1]) - 1)),
        "frame_index_high": field("pb", lambda p: p.__setitem__(1, 3)), "frame_index_negative": field("pa", lambda p: p.__setitem__(2, -1)),
        "distance_zero": opt(max_distance=0.0), "distance_negative": opt(max_distance=-0.5), "distance_nan": opt(max_distance=float("nan")),
        "distance_inf": opt(max_distance=float("inf")),
        "ratio_zero": opt(max_ratio=0.0), "ratio_above_one": opt(max_ratio=1.0000001), "ratio_negative": opt(max_ratio=-0.5), "ratio_nan": opt(max_ratio=float("nan")),
        "features_zero": opt(max_features=0), "features_above_max": opt(max_features=Y.MAX_FEATURES + 1), "features_negative": opt(max_features=-5),
    }


@pytest.mark.parametrize("name", sorted(_einval_cases()))
def test_einval_without_a_device_and_outputs_untouched(lib, name, capfd):
    from xrsfm_amd import capi
    how = _einval_cases()[name]
    c, o = _Call(), capi.match_options()
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
    assert err.count("\n") == 1 and "xrsfm_ba_match_descriptors" in err


def test_no_pairs_is_success_without_a_device(lib):
    from xrsfm_amd import capi
    c = _Call()
    c.n_pairs = 0
    assert c.run(lib, capi.match_options()) == 0 and c.untouched()
    assert c.run(lib, capi.match_options(), null=("ptr", "desc", "pa", "pb", "mp", "m", "nr", "nc")) == 0
    r = capi.match_descriptors(c.ptr, c.desc, [], [])
    assert r["match_ptr"].tolist() == [0] and r["matches"].shape == (0, 2) and len(r["num_row"]) == 0 and len(r["num_col"]) == 0


def test_valid_call_without_a_device_is_enodev(lib):
    import torch
    from xrsfm_amd import capi
    if torch.cuda.is_available() and capi.device_count() > 0:
        pytest.skip("a GPU is present")
    c = _Call()
    assert c.run(lib, capi.match_options()) == -2 and c.untouched()
    assert c.run(lib, capi.match_options(), null=("nr", "nc")) == -2 and c.untouched()
    with pytest.raises(RuntimeError, match="ENODEV"):
        capi.match_descriptors(c.ptr, c.desc, c.pa, c.pb)
    with pytest.raises(RuntimeError, match="ENODEV"):
        capi.debug_match_top2(c.frames[0], c.frames[1])


def test_matched_points_and_quantize_descriptors():
    from xrsfm_amd import capi
    kp_ptr = np.array([0, 3, 5, 9])
    xy = np.arange(18, dtype=np.float64).reshape(9, 2)
    res = dict(match_ptr=np.array([0, 2, 2, 3], np.int64), matches=np.array([[0, 1], [2, 0], [3, 1]], np.int32))
    xa, xb = capi.matched_points(res, kp_ptr, xy, [0, 1, 2], [1, 2, 0])
    assert xa.tolist() == [[0, 1], [4, 5], [16, 17]] and xb.tolist() == [[8, 9], [6, 7], [2, 3]]
    xa, xb = capi.matched_points(dict(match_ptr=np.zeros(1, np.int64), matches=np.zeros((0, 2), np.int32)), kp_ptr, xy, [], [])
    assert xa.shape == (0, 2) and xb.shape == (0, 2)
    with pytest.raises(ValueError):
        capi.matched_points(res, kp_ptr, xy, [0, 1], [1, 2])
    d = np.array([[0.0, 0.00097, 0.00098, 0.2, 0.49707, 0.3]], np.float32)
    assert capi.quantize_descriptors(d).tolist() == [[0, 0, 1, 102, 254, 154]] and capi.quantize_descriptors(d).dtype == np.uint8
    assert capi.quantize_descriptors(np.float32([0.498])).tolist() == [255]
    with pytest.raises(ValueError):
        capi.quantize_descriptors(np.float32([0.5]))
    with pytest.raises(ValueError):
        capi.quantize_descriptors(np.float32([-0.01]))


# ---------------------------------------------------------------------------------------------------- the yardstick itself
def test_the_two_formulations_agree_on_the_whole_catalogue():
    for k, e in enumerate(Y.entries()):
        r1, r2 = Y.reference(k), Y.reference(k, True)
        for f in r1:
            assert np.array_equal(r1[f], r2[f]), (e["tag"], f)


def test_synthetic_descriptors_match_as_planted():
    rng = np.random.default_rng(5)
    a = Y.sift_like(rng, 300)
    b, src = Y.related(rng, a, 350, share=200.0 / 350.0)
    r = Y.run_pair(a, b)
    planted = sorted((int(s), int(k)) for k, s in enumerate(src) if s >= 0)
    assert len(planted) == 200 and [tuple(m) for m in r["matches"].tolist()] == planted


def test_catalogue_coverage():
    F, E = Y.frames(), Y.entries()
    by = {e["tag"]: k for k, e in enumerate(E)}
    assert len(by) == len(E)
    ref = lambda tag: Y.reference(by[tag])
    shape = lambda tag: (len(F[E[by[tag]]["a"]]), len(F[E[by[tag]]["b"]]))
    for n in Y.SIZES:
        for m in Y.SIZES:
            assert shape("shape_%dx%d" % (n, m)) == (n, m)
    assert {0, 1, Y.TILE - 1, Y.TILE, Y.TILE + 1, Y.COLS - 1, Y.COLS, Y.COLS + 1, Y.STRIP - 1, Y.STRIP, Y.STRIP + 1, 2 * Y.STRIP + 1} == set(Y.SIZES)
    assert sum(len(r["matches"]) > 0 for r in (Y.reference(k) for k in Y.main_group())) >= 80
    assert len(ref("shape_257x257")["matches"]) >= 100 and ref("shape_0x17")["num_col"] == 0 and len(ref("shape_17x0")["matches"]) == 0
    # several strips, and every strip contributes a column's best somewhere
    assert shape("strips_1000x1200") == (1000, 1200) and shape("strips_300x129") == (300, 129)
    assert set((ref("strips_1000x1200")["col_top"][:, 1] // Y.STRIP).tolist()) == set(range(8))
    assert len(ref("strips_1000x1200")["matches"]) >= 500 and len(ref("strips_300x129")["matches"]) >= 50
    # best and next of row 7 in the last partial tile; of column 3 in different strips
    e = E[by["edge_300x131"]]
    S = Y.scores(F[e["a"]], F[e["b"]])
    o7, o3 = np.argsort(-S[7], kind="stable")[:2], np.argsort(-S[:, 3], kind="stable")[:2]
    assert min(o7) >= 128 and 131 % Y.TILE != 0 and o3[0] // Y.STRIP == 0 and o3[1] // Y.STRIP == 2
    r = ref("edge_300x131")
    assert r["row_top"][7].tolist() == [S[7, o7[0]], o7[0], S[7, o7[1]]] and r["col_top"][3].tolist() == [S[o3[0], 3], o3[0], S[o3[1], 3]]
    # extreme values
    e = E[by["high_40x50"]]
    assert F[e["a"]].min() >= 128 and F[e["b"]].min() >= 128 and ref("high_40x50")["row_top"][:, 0].min() > Y.TAB_MAX
    assert np.all(ref("all255_20x20")["row_top"][:, [0, 2]] == 128 * 255 * 255) and np.all(ref("all255_20x20")["row_top"][:, 1] == 0)
    assert len(ref("all255_20x20")["matches"]) == 0
    r = ref("zero_rows_66x70")
    assert r["row_top"][3].tolist() == [0, -1, 0] and r["row_top"][17].tolist() == [0, -1, 0] and r["col_top"][5].tolist() == [0, -1, 0]
    assert len(r["matches"]) >= 20
    assert np.all(ref("all_zero_17x33")["row_top"] == [0, -1, 0]) and np.all(ref("all_zero_17x33")["col_top"] == [0, -1, 0])
    # ties: the tied row is rejected, the row of a tied column is rejected under mutual_best and kept without
    tied = lambda top: np.flatnonzero((top[:, 0] == top[:, 2]) & (Y.dist(top[:, 0]) < 0.3))           # a tied best that is a close match
    rows_tied, cols_tied = (lambda r: tied(r["row_top"])), (lambda r: tied(r["col_top"]))
    r = ref("tie_row")
    assert len(rows_tied(r)) == 1 and r["row_match"][rows_tied(r)[0]] == -1
    assert ref("ratio1_tie_row")["row_match"][rows_tied(r)[0]] == -1                          # a tie fails even at max_ratio 1
    r, r0 = ref("tie_col"), ref("no_mutual_tie_col")
    j = int(cols_tied(r)[0])
    i_lo = int(r["col_top"][j, 1])
    assert len(cols_tied(r)) == 1 and r["col_match"][j] == -1 and r["row_match"][i_lo] == j
    assert i_lo not in r["matches"][:, 0] and [i_lo, j] in r0["matches"].tolist()
    assert len(r0["matches"]) == r0["num_row"] > len(r["matches"])
    # options
    assert len(ref("no_mutual_129x257")["matches"]) == ref("no_mutual_129x257")["num_row"] >= len(ref("shape_129x257")["matches"]) >= 50
    assert shape("clip100") == (130, 130) and ref("clip100")["row_top"].shape == (100, 3) and ref("clip100")["row_top"][:, 1].max() < 100
    assert not np.array_equal(ref("clip100")["matches"], ref("ab")["matches"][:len(ref("clip100")["matches"])])
    assert ref("ratio1_near")["num_row"] == ref("near_65x70")["num_row"] + 1 and len(ref("ratio1_near")["matches"]) > len(ref("near_65x70")["matches"])
    e = E[by["distance_at_best"]]
    base, r = ref("shape_129x257"), ref("distance_at_best")
    i = int(base["matches"][0][0])
    assert np.float32(e["opt"]["max_distance"]) == Y.dist(base["row_top"][i, 0]) and i not in r["matches"][:, 0] and 0 < len(r["matches"]) < len(base["matches"])
    up = Y.run_pair(F[e["a"]], F[e["b"]], Y.options(max_distance=float(np.nextafter(np.float32(e["opt"]["max_distance"]), np.float32(1)))))
    assert i in up["matches"][:, 0]
    # structure
    assert ref("self_129")["matches"].tolist() == [[i, i] for i in range(129)]
    assert ref("ba")["matches"][:, ::-1][np.argsort(ref("ba")["matches"][:, 1], kind="stable")].tolist() == ref("ab")["matches"].tolist()
    assert len(ref("ab")["matches"]) >= 60
    used = np.bincount([e["a"] for e in E] + [e["b"] for e in E if e["b"] != e["a"]])
    assert used.max() >= 20
    assert len(Y.batch257()) == 257 and len(set(Y.batch257())) >= 100
    assert len(Y.option_groups()) >= 5


# ---------------------------------------------------------------------------------------------------- the header on the host
def test_rule_header_on_the_host_reproduces_the_yardstick(tmp_path):
    """ba_match_rule.h (the update, the merge, the table, the test, the compaction) in a sequential program with scalar dot
    products, under the sanitizers: the triples, the counts and the matches of every catalogue pair equal the yardstick's."""
    exe = H.build(tmp_path)
    F, E = Y.frames(), Y.entries()
    ks = [k for k, e in enumerate(E) if not e["tag"].startswith("shape_") or len(F[e["a"]]) in (0, 17, 129, 257)]
    text = "\n".join(H.pair_input(F[E[k]["a"]], F[E[k]["b"]], Y.entry_options(E[k])) for k in ks) + "\n"
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.strip().split("\n")
    assert len(out) == len(ks) >= 70
    for k, ln in zip(ks, out):
        want = Y.reference(k)
        got = H.parse_pair(ln, len(want["row_top"]), len(want["col_top"]))
        for f in got:
            assert np.array_equal(got[f], want[f]), (E[k]["tag"], f)


def test_match_kernels_do_not_spill(tmp_path):
    """k_match_prep, k_match_dots and k_match_select of the gfx950 code object have no spilled VGPR and no private (scratch)
    segment, and the dots kernel holds the int8 matrix instruction."""
    from xrsfm_amd import _build
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    asm = tmp_path / "xba.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-Wno-unused-value",
                    "-Wno-deprecated-declarations", os.path.join(_build.CSRC, "xrsfm_ba.hip"), "-o", str(asm)], check=True, capture_output=True)
    text = asm.read_text()
    seen = set()
    for blk in text.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        m = re.search(r"k_match_(prep|dots|select)", name)
        if not m:
            continue
        seen.add(m.group(1))
        spills = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1))
        scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1))
        lds = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", blk).group(1))
        assert spills == 0 and scratch == 0 and lds <= 160 * 1024, (name, spills, scratch, lds)
    assert seen == {"prep", "dots", "select"}
    body = text[text.index("k_match_dots"):]
    assert "v_mfma_i32_16x16x64_i8" in body[:body.index(".end_amdhsa_kernel")] or "v_mfma_i32_16x16x64_i8" in body[:body.index("s_endpgm")]
