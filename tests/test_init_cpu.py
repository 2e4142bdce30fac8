"""xrsfm_ba_two_view_init without a GPU: the interface (exports, struct layout, defaults, every EINVAL, the empty call, ENODEV), the
sampler against the yardstick's, the yardstick's own checks (catalogue coverage, fragile cap, the bars for the float64 restatement,
the checks rejecting a wrong result), the headers on the host as stand-alone programs built with the address and
undefined-behaviour sanitizers (ba_init_scan.h driven with the yardstick's per-model records; ba_init_scan.h and ba_init_geom.h in a
sequential driver of whole pairs, against the same bars as the GPU), and the kernel's register / scratch figures."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import init_host_driver as H
from tests import init_yardstick as Y

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0x5A


def test_exports_and_struct_layout(lib, tmp_path):
    from xrsfm_amd import capi
    for name in ("xrsfm_ba_two_view_options_default", "xrsfm_ba_two_view_init", "xrsfm_ba_debug_two_view_samples"):
        assert name in capi.EXPORTS and getattr(lib, name) is not None
    fields = [f for f, _ in capi.CTwoViewOptions._fields_]
    src = tmp_path / "p.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "xrsfm_ba.h"\nint main(){printf("%zu", sizeof(xrsfm_ba_two_view_options));\n' +
                   "".join('printf(" %%zu", offsetof(xrsfm_ba_two_view_options, %s));\n' % f for f in fields) +
                   'printf(" %d %d\\n", XRSFM_BA_INIT_MAX_MATCHES, XRSFM_BA_INIT_MAX_TRIALS);return 0;}\n')
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "p")], check=True)
    out = [int(x) for x in subprocess.run([str(tmp_path / "p")], capture_output=True, text=True, check=True).stdout.split()]
    o = capi.CTwoViewOptions
    assert out == [C.sizeof(o)] + [getattr(o, f).offset for f in fields] + [capi.INIT_MAX_MATCHES, capi.INIT_MAX_TRIALS]
    assert (capi.INIT_MAX_MATCHES, capi.INIT_MAX_TRIALS, capi.INIT_SLOT_STRIDE) == (Y.MAX_MATCHES, Y.MAX_TRIALS, Y.SLOT_STRIDE)


def test_default_options_are_the_reference_values(lib):
    from xrsfm_amd import capi
    o, y = capi.two_view_options(), Y.Options()
    assert (o.confidence, o.max_iterations, o.seed, o.min_matches, o.max_depth, o.n_angles, o.min_front_ratio, o.min_angle_ratio, o.min_num_valid) == \
        (0.9, 50, 0, 10, 100.0, 2, 0.5, 0.5, 200)
    assert (y.confidence, y.max_iterations, y.seed, y.min_matches, y.max_depth, len(y.min_angle_rad), y.min_front_ratio, y.min_angle_ratio,
            y.min_num_valid) == (0.9, 50, 0, 10, 100.0, 2, 0.5, 0.5, 200)
    assert tuple(o.min_angle_rad)[:2] == y.min_angle_rad == (16.0 * Y.DEG, 8.0 * Y.DEG)
    assert abs(o.min_angle_rad[0] - np.deg2rad(16.0)) < 1e-15
    o2 = capi.two_view_options(min_angle_rad=[0.3, 0.2, 0.1], min_num_valid=20)
    assert o2.n_angles == 3 and tuple(o2.min_angle_rad) == (0.3, 0.2, 0.1, 0.0) and o2.min_num_valid == 20


class _Call:
    """A small valid problem and sentinel-filled outputs for the raw C call."""
    def __init__(self):
        E = Y.entries()
        idx = [k for k, e in enumerate(E) if e["tag"] in ("n10_s0_wide_v0", "n11_s0_mid_v0", "too_few")]
        ptr, xa, xb, th = Y.arrays(idx)
        self.ptr, self.xa, self.xb, self.th = ptr.copy(), xa.copy(), xb.copy(), th.copy()
        npair, n = len(idx), len(xa)
        self.n_pairs = npair
        self.seed = np.zeros(npair, np.uint32)
        self.out = dict(status=np.full(npair, SENTINEL, np.uint8), E=np.full((npair, 9), 1234.5), q=np.full((npair, 4), 1234.5), t=np.full((npair, 3), 1234.5),
                        points=np.full((n, 3), 1234.5), emask=np.full(n, SENTINEL, np.uint8), fmask=np.full(n, SENTINEL, np.uint8),
                        counts=np.full((npair, 8), -77, np.int32), accepted=np.full(npair, SENTINEL, np.uint8), ntr=np.full(npair, -77, np.int32),
                        best=np.full(npair, -77, np.int32))

    def untouched(self):
        o = self.out
        return (all(np.all(o[k] == 1234.5) for k in ("E", "q", "t", "points")) and all(np.all(o[k] == SENTINEL) for k in ("status", "emask", "fmask", "accepted"))
                and all(np.all(o[k] == -77) for k in ("counts", "ntr", "best")))

    def run(self, lib, opt, null=(), per_pair_seed=False):
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        up = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))
        o = self.out
        a = dict(opt=C.byref(opt) if opt is not None else None, ptr=ip(self.ptr), xa=dp(self.xa), xb=dp(self.xb), th=dp(self.th),
                 seed=self.seed.ctypes.data_as(C.POINTER(C.c_uint32)) if per_pair_seed else None, status=up(o["status"]), E=dp(o["E"]), q=dp(o["q"]),
                 t=dp(o["t"]), points=dp(o["points"]), emask=up(o["emask"]), fmask=up(o["fmask"]), counts=ip(o["counts"]), accepted=up(o["accepted"]),
                 ntr=ip(o["ntr"]), best=ip(o["best"]))
        for k in null:
            a[k] = None
        return lib.xrsfm_ba_two_view_init(a["opt"], self.n_pairs, a["ptr"], a["xa"], a["xb"], a["th"], a["seed"], a["status"], a["E"], a["q"], a["t"],
                                          a["points"], a["emask"], a["fmask"], a["counts"], a["accepted"], a["ntr"], a["best"])


def _einval_cases():
    def opt(**kw):
        return lambda c, o: [setattr(o, k, v) for k, v in kw.items()]

    def field(name, fn):
        return lambda c, o: fn(getattr(c, name))

    def angle(i, v):
        return lambda c, o: o.min_angle_rad.__setitem__(i, v)
    return {
        "null_opt": None, "null_status": ("status",), "null_E": ("E",), "null_q": ("q",), "null_t": ("t",), "null_points": ("points",),
        "null_essential_mask": ("emask",), "null_front_mask": ("fmask",), "null_counts": ("counts",), "null_ptr": ("ptr",), "null_threshold": ("th",),
        "null_xy_a": ("xa",), "null_xy_b": ("xb",),
        "negative_pairs": lambda c, o: setattr(c, "n_pairs", -1),
        "ptr_not_from_zero": field("ptr", lambda p: p.__setitem__(0, 1)),
        "ptr_decreasing": field("ptr", lambda p: p.__setitem__(2, int(p[1]) - 1)),
        "xy_a_nan": field("xa", lambda a: a.__setitem__((1, 0), np.nan)), "xy_b_inf": field("xb", lambda a: a.__setitem__((3, 1), np.inf)),
        "threshold_nan": field("th", lambda a: a.__setitem__(1, np.nan)), "threshold_zero": field("th", lambda a: a.__setitem__(0, 0.0)),
        "threshold_negative": field("th", lambda a: a.__setitem__(2, -0.01)),
        "confidence_nan": opt(confidence=float("nan")), "confidence_above_one": opt(confidence=1.5), "confidence_negative": opt(confidence=-0.1),
        "no_iterations": opt(max_iterations=0), "too_many_iterations": opt(max_iterations=Y.MAX_TRIALS + 1),
        "min_matches_four": opt(min_matches=4), "max_depth_zero": opt(max_depth=0.0), "max_depth_inf": opt(max_depth=float("inf")),
        "no_angles": opt(n_angles=0), "five_angles": opt(n_angles=5), "angle_negative": angle(1, -0.1), "angle_nan": angle(0, float("nan")),
        "front_ratio_negative": opt(min_front_ratio=-0.5), "angle_ratio_nan": opt(min_angle_ratio=float("nan")), "min_num_valid_negative": opt(min_num_valid=-1),
    }


@pytest.mark.parametrize("name", sorted(_einval_cases()))
def test_einval_without_a_device_and_outputs_untouched(lib, name, capfd):
    from xrsfm_amd import capi
    how = _einval_cases()[name]
    c, o = _Call(), capi.two_view_options()
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
    assert err.count("\n") == 1 and "xrsfm_ba_two_view_init" in err


def test_no_pairs_is_success_without_a_device(lib):
    from xrsfm_amd import capi
    c = _Call()
    c.n_pairs = 0
    assert c.run(lib, capi.two_view_options()) == 0 and c.untouched()
    assert c.run(lib, capi.two_view_options(), null=("ptr", "xa", "xb", "th", "status", "E", "q", "t", "points", "emask", "fmask", "counts", "accepted",
                                                     "ntr", "best")) == 0
    r = capi.two_view_init(np.zeros(1, np.int32), np.zeros((0, 2)), np.zeros((0, 2)), np.zeros(0))
    assert all(len(getattr(r, k)) == 0 for k in r.FIELDS)
    assert capi.first_accepted([1, 0, 2], [0, 2, 3]) == (2, 0) and capi.first_accepted([0, 1], [2, 2]) == (0, 1) and capi.first_accepted([0], [0]) == (-1, -1)


def test_valid_call_without_a_device_is_enodev(lib):
    import torch
    from xrsfm_amd import capi
    if torch.cuda.is_available() and capi.device_count() > 0:
        pytest.skip("a GPU is present")
    c = _Call()
    assert c.run(lib, capi.two_view_options()) == -2 and c.untouched()
    assert c.run(lib, capi.two_view_options(), per_pair_seed=True, null=("accepted", "ntr", "best")) == -2 and c.untouched()
    with pytest.raises(RuntimeError, match="ENODEV"):
        capi.two_view_init(c.ptr, c.xa, c.xb, c.th)


# ---------------------------------------------------------------------------------------------------- sampler
def test_mt19937_is_the_standard_generator():
    g = Y.MT19937(5489)
    assert [g.next() for _ in range(10000)][-1] == 4123659995          # the value the C++ standard requires of std::mt19937


@pytest.mark.parametrize("seed,n", [(0, 5), (0, 6), (0, 10), (0, 100), (1, 64), (5489, 257), (0xFFFFFFFF, 1000), (7, 8192)])
def test_debug_two_view_samples_equal_the_yardsticks_sampler(lib, seed, n):
    from xrsfm_amd import capi
    got, want = capi.debug_two_view_samples(seed, n, 64), Y.sample_quintuples(seed, n, 64)
    assert np.array_equal(got, want)
    assert got.min() >= 0 and got.max() < n and all(len(set(r)) == 5 for r in got.tolist())
    assert lib.xrsfm_ba_debug_two_view_samples(0, 4, 1, got.ctypes.data_as(C.POINTER(C.c_int32))) == capi.EINVAL
    assert lib.xrsfm_ba_debug_two_view_samples(0, 10, 65, got.ctypes.data_as(C.POINTER(C.c_int32))) == capi.EINVAL


# ---------------------------------------------------------------------------------------------------- the yardstick itself
def test_catalogue_coverage():
    main, deg = Y.catalogue()
    ext, E = Y.reference("longdouble"), Y.entries()
    assert len(main) >= 60 and {len(e["xa"]) for e in main} >= set(Y.LENGTHS)
    by = {e["tag"]: k for k, e in enumerate(E)}
    assert {r["status"] for r in ext} == {0, 1, 2, 3}
    assert ext[by["too_few"]]["status"] == 2 and ext[by["too_many"]]["status"] == 3
    acc = {r["accepted"] for r in ext[:len(main)]}
    assert acc >= {0, 2, 3}                                           # passes neither, only 8 degrees, both
    assert ext[by["accept16"]]["accepted"] == 3 and ext[by["accept8"]]["accepted"] == 2 and ext[by["reject"]]["accepted"] == 0   # at the defaults
    assert ext[by["bound_drops"]]["lowered"] and ext[by["bound_drops"]]["num_trials"] < 50
    assert ext[by["maxit1"]]["num_trials"] == 1 and ext[by["maxit64"]]["num_trials"] == 64
    assert any(r["num_trials"] == 50 for r in ext[:len(main)])
    assert any(min(r["nmodels"]) == 0 for r in Y.reference("float64") if r["nmodels"])     # a trial without a model (the overflow pair)
    assert any(max(r["nmodels"]) >= 4 for r in ext if r["nmodels"])
    assert {int(r["counts"][2]) for r in ext[:len(main)] if r["status"] == 1} == {0, 1, 2, 3}
    assert {e["tag"] for e in deg} >= {"n5", "n6", "pure_rotation", "planar", "outliers_only", "duplicated"}
    assert ext[by["n5"]]["status"] == 1 and ext[by["n5"]]["num_trials"] >= 1


def test_status_zero_and_a_trial_without_a_model():
    """status 0 both ways: an E without a point in front of any candidate, and (float64 only: the products of the coordinates
    overflow) trials without a model that leave best_E NaN"""
    E, ext, f64 = Y.entries(), Y.reference("longdouble"), Y.reference("float64")
    k = next(k for k, e in enumerate(E) if e["tag"] == "nothing_in_front")
    for r in (ext[k], f64[k]):
        assert r["status"] == 0 and r["best_trial"] >= 0 and r["E"] is not None and r["counts"][0] > 0 and not r["counts"][1:].any() and not r["front_mask"].any()
    k = next(k for k, e in enumerate(E) if e["tag"] == "overflow")
    r = f64[k]
    assert r["status"] == 0 and r["best_trial"] == -1 and r["num_trials"] == 3 and r["nmodels"] == [0, 0, 0] and r["E"] is None
    assert not r["essential_mask"].any() and not r["counts"].any()


def test_fragile_cap_and_float64_restatement_meets_every_bar():
    share = Y.fragile_share()
    print("fragile share %.3f of %d pairs" % (share, Y.n_main()))
    assert share <= Y.FRAGILE_CAP
    ext, f64, fr, E = Y.reference("longdouble"), Y.reference("float64"), Y.fragile(), Y.entries()
    checked = 0
    for k, e in enumerate(E):
        assert not Y.always_true(f64[k], e["xa"], e["xb"], e["th"]), e["tag"]
        assert not Y.always_true(ext[k], e["xa"], e["xb"], e["th"]), e["tag"]
        if fr[k] or k >= Y.n_main():
            continue
        assert Y.same_discrete(f64[k], ext[k]), e["tag"]
        if ext[k]["status"] == 1:
            checked += 1
            assert Y.loose_ok(f64[k], ext[k]), e["tag"]
    worst = Y.restatement_deviation()
    print("float64 restatement over %d pairs: %s" % (checked, {k: "%.2e" % v for k, v in worst.items()}))
    assert checked >= 55
    for k, v in worst.items():                       # the named constants are the measurement: not below it, and not inflated
        assert Y.RESTATEMENT_DEVIATION[k] / 4 <= v <= Y.RESTATEMENT_DEVIATION[k], (k, v)
        assert Y.TIGHT_BAR[k] == 16 * Y.RESTATEMENT_DEVIATION[k]


def test_the_checks_reject_a_wrong_result():
    E = Y.entries()
    k = next(k for k, e in enumerate(E) if e["tag"] == "bound_drops")
    e, r = E[k], Y.reference("longdouble")[k]
    good = dict(r, E=np.asarray(r["E"], np.float64), R=np.asarray(r["R"], np.float64), t=np.asarray(r["t"], np.float64), points=np.asarray(r["points"], np.float64))
    assert Y.loose_ok(good, r) and not Y.always_true(good, e["xa"], e["xb"], e["th"])
    assert all(v <= Y.TIGHT_BAR[name] for name, v in Y.deviations(good, r).items())
    transposed = dict(good, E=good["E"].reshape(3, 3).T.ravel().copy())
    assert not Y.loose_ok(transposed, r) and Y.always_true(transposed, e["xa"], e["xb"], e["th"])
    assert Y.deviations(transposed, r)["E"] > Y.TIGHT_BAR["E"]
    negated = dict(good, t=-good["t"])
    assert not Y.loose_ok(negated, r) and Y.deviations(negated, r)["t"] > Y.TIGHT_BAR["t"]
    flipped = dict(good, essential_mask=good["essential_mask"].copy())
    flipped["essential_mask"][0] ^= 1
    assert not Y.same_discrete(flipped, r) and Y.always_true(flipped, e["xa"], e["xb"], e["th"])


# ---------------------------------------------------------------------------------------------------- the headers on the host
def test_scan_header_reproduces_the_yardstick(tmp_path):
    """ba_init_scan.h fed the yardstick's per-model records: the same best model, bound and trial count, and it stops where the
    yardstick stops."""
    exe = H.build(tmp_path, "scan", H.SCAN_DRIVER)
    ext, E, lines, want = Y.reference("longdouble"), Y.entries(), [], []
    for k, r in enumerate(ext):
        if r["status"] >= 2:
            continue
        opt = Y.Options(**E[k]["opt"])
        lines.append("%d %d %r %d" % (r["n"], opt.max_iterations, opt.confidence, len(r["records"])))
        lines += ["%d %d %d %r" % rec for rec in r["records"]]
        want.append((r["best_trial"], r["num_trials"], int(r["counts"][0]), 0))
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    got = [tuple(int(x) for x in ln.split()) for ln in out if ln]
    assert len(got) == len(want) >= 60
    assert [(g[0], g[2], g[3], g[4]) for g in got] == want
    assert Y.bound_row(10, 0.9)[10] == 0 and Y.bound_row(10, 0.9)[0] == Y.UNBOUNDED and Y.bound_row(8192, 0.9)[1] == Y.UNBOUNDED and \
        Y.bound_row(10, 1.0)[10] == Y.UNBOUNDED and Y.bound_row(10, 0.9)[8] == 6


def run_pair_driver(exe, ks):
    E = Y.entries()
    text = "\n".join(H.pair_input(E[k]["xa"], E[k]["xb"], E[k]["th"], Y.Options(**E[k]["opt"])) for k in ks) + "\n"
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.strip().split("\n")
    assert len(out) == len(ks)
    return {k: H.parse_pair(ln, len(E[k]["xa"])) for k, ln in zip(ks, out)}


def check_against_yardstick(results, label):
    """results: catalogue index -> dict of the outputs of one implementation; the checks of DESIGN.md 5j"""
    ext, fr, E, worst, checked = Y.reference("longdouble"), Y.fragile(), Y.entries(), {k: 0.0 for k in Y.TIGHT_BAR}, 0
    for k, got in results.items():
        e = E[k]
        assert not Y.always_true(got, e["xa"], e["xb"], e["th"]), (label, e["tag"])
        if fr[k] or k >= Y.n_main():
            continue
        assert Y.same_discrete(got, ext[k]), (label, e["tag"], [(x, got[x], ext[k][x]) for x in Y.DISCRETE], list(got["counts"]), list(ext[k]["counts"]))
        if ext[k]["status"] == 1:
            checked += 1
            assert Y.loose_ok(got, ext[k]), (label, e["tag"])
            for name, v in Y.deviations(got, ext[k]).items():
                worst[name] = max(worst[name], v)
    print("%s: %d pairs, largest deviations %s; tight bars %s" % (label, checked, {k: "%.2e" % v for k, v in worst.items()},
                                                                 {k: "%.2e" % v for k, v in Y.TIGHT_BAR.items()}))
    for name, v in worst.items():
        assert v <= Y.TIGHT_BAR[name], (label, name, v)
    return checked


def test_geometry_headers_on_the_host_meet_every_bar(tmp_path):
    """The library's own arithmetic (5-point solver, eigenvalues, decomposition, triangulation, the scan) without the kernel around
    it, under the sanitizers: on every non-fragile pair the discrete outputs equal the extended yardstick's and E, R, t and the
    points meet both bars."""
    exe = H.build(tmp_path, "pairs", H.PAIR_DRIVER)
    ks = [k for k, e in enumerate(Y.entries()) if e["tag"] != "too_many"]
    assert check_against_yardstick(run_pair_driver(exe, ks), "sequential host driver") >= 55


def test_init_kernel_does_not_spill(tmp_path):
    """k_init_pairs of the gfx950 code object has no spilled VGPR and no private (scratch) segment."""
    from xrsfm_amd import _build
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    asm = tmp_path / "xba.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-Wno-unused-value",
                    "-Wno-deprecated-declarations", os.path.join(_build.CSRC, "xrsfm_ba.hip"), "-o", str(asm)], check=True, capture_output=True)
    seen = 0
    for blk in asm.read_text().split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        if "k_init_pairs" not in name:
            continue
        seen += 1
        spills = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1))
        scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1))
        assert spills == 0 and scratch == 0, (name, spills, scratch)
    assert seen == 1
