"""xrsfm_ba_verify_pairs without a GPU: the interface (exports, struct layout, defaults, every EINVAL, the empty call, ENODEV), the
sampler against the yardstick's, the yardstick's own checks (catalogue coverage, fragile cap, the bars for the float64 restatement,
the checks rejecting a wrong result), the headers on the host as stand-alone programs built with the address and
undefined-behaviour sanitizers (ba_fund_scan.h driven with the yardstick's per-model records; ba_fund_scan.h and ba_fund_geom.h in a
sequential driver of whole pairs, against the same bars as the GPU), and the kernel's register / scratch figures."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import fund_host_driver as H
from tests import fund_yardstick as Y

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0x5A


def test_exports_and_struct_layout(lib, tmp_path):
    from xrsfm_amd import capi
    for name in ("xrsfm_ba_verify_pairs_options", "xrsfm_ba_verify_pairs", "xrsfm_ba_debug_fund_samples"):
        assert name in capi.EXPORTS and getattr(lib, name) is not None
    fields = [f for f, _ in capi.CFundOptions._fields_]
    src = tmp_path / "p.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "xrsfm_ba.h"\nint main(){printf("%zu", sizeof(xrsfm_ba_fund_options));\n' +
                   "".join('printf(" %%zu", offsetof(xrsfm_ba_fund_options, %s));\n' % f for f in fields) +
                   'printf(" %d %d\\n", XRSFM_BA_FUND_MAX_MATCHES, XRSFM_BA_FUND_MAX_TRIALS);return 0;}\n')
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "p")], check=True)
    out = [int(x) for x in subprocess.run([str(tmp_path / "p")], capture_output=True, text=True, check=True).stdout.split()]
    o = capi.CFundOptions
    assert out == [C.sizeof(o)] + [getattr(o, f).offset for f in fields] + [capi.FUND_MAX_MATCHES, capi.FUND_MAX_TRIALS]
    assert (capi.FUND_MAX_MATCHES, capi.FUND_MAX_TRIALS, capi.FUND_LOCAL_BIT) == (Y.MAX_MATCHES, Y.MAX_TRIALS, Y.LOCAL_BIT)


def test_default_options_are_the_reference_values(lib):
    from xrsfm_amd import capi
    o, y = capi.verify_pairs_options(), Y.Options()
    want = (4.0, 0.999, 0.25, 100, 10000, 0, 15, 15, 0.25)
    names = ("max_error", "confidence", "min_inlier_ratio", "min_num_trials", "max_num_trials", "seed", "min_matches", "min_num_inliers", "min_accept_ratio")
    assert tuple(getattr(o, k) for k in names) == want and tuple(getattr(y, k) for k in names) == want
    assert Y.num_trials_bound(25000, 100000, 0.999) == 113174 and Y.trial_cap(y) == 10000        # the constructor's bound is above the cap
    assert Y.num_trials_bound(50, 100, 0.999) == 881 and Y.num_trials_bound(80, 100, 0.999) < 100
    assert capi.verify_pairs_options(seed=3, max_error=2.0).seed == 3
    with pytest.raises(AttributeError):
        capi.verify_pairs_options(no_such_field=1)


class _Call:
    """A small valid problem and sentinel-filled outputs for the raw C call."""
    def __init__(self):
        E = Y.entries()
        idx = [k for k, e in enumerate(E) if e["tag"] in ("n15_s0", "n16_s0.3", "too_few")]
        ptr, xa, xb = Y.arrays(idx)
        self.ptr, self.xa, self.xb = ptr.copy(), xa.copy(), xb.copy()
        npair, n = len(idx), len(xa)
        self.n_pairs = npair
        self.me = np.full(npair, 4.0)
        self.seed = np.zeros(npair, np.uint32)
        self.out = dict(status=np.full(npair, SENTINEL, np.uint8), F=np.full((npair, 9), 1234.5), mask=np.full(n, SENTINEL, np.uint8),
                        ninl=np.full(npair, -77, np.int32), ntr=np.full(npair, -77, np.int32), best=np.full(npair, -77, np.int32),
                        accepted=np.full(npair, SENTINEL, np.uint8))

    def untouched(self):
        o = self.out
        return (np.all(o["F"] == 1234.5) and all(np.all(o[k] == SENTINEL) for k in ("status", "mask", "accepted"))
                and all(np.all(o[k] == -77) for k in ("ninl", "ntr", "best")))

    def run(self, lib, opt, null=(), per_pair=False):
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        up = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))
        o = self.out
        a = dict(opt=C.byref(opt) if opt is not None else None, ptr=ip(self.ptr), xa=dp(self.xa), xb=dp(self.xb), me=dp(self.me) if per_pair else None,
                 seed=self.seed.ctypes.data_as(C.POINTER(C.c_uint32)) if per_pair else None, status=up(o["status"]), F=dp(o["F"]), mask=up(o["mask"]),
                 ninl=ip(o["ninl"]), ntr=ip(o["ntr"]), best=ip(o["best"]), accepted=up(o["accepted"]))
        for k in null:
            a[k] = None
        return lib.xrsfm_ba_verify_pairs(a["opt"], self.n_pairs, a["ptr"], a["xa"], a["xb"], a["me"], a["seed"], a["status"], a["F"], a["mask"], a["ninl"],
                                         a["ntr"], a["best"], a["accepted"])


def _einval_cases():
    def opt(**kw):
        return lambda c, o: [setattr(o, k, v) for k, v in kw.items()]

    def field(name, fn):
        return lambda c, o: fn(getattr(c, name))
    return {
        "null_opt": None, "null_status": ("status",), "null_F": ("F",), "null_mask": ("mask",), "null_ptr": ("ptr",), "null_xy_a": ("xa",),
        "null_xy_b": ("xb",),
        "negative_pairs": lambda c, o: setattr(c, "n_pairs", -1),
        "ptr_not_from_zero": field("ptr", lambda p: p.__setitem__(0, 1)),
        "ptr_decreasing": field("ptr", lambda p: p.__setitem__(2, int(p[1]) - 1)),
        "xy_a_nan": field("xa", lambda a: a.__setitem__((1, 0), np.nan)), "xy_b_inf": field("xb", lambda a: a.__setitem__((3, 1), np.inf)),
        "pair_error_nan": ("per_pair", field("me", lambda a: a.__setitem__(1, np.nan))),
        "pair_error_zero": ("per_pair", field("me", lambda a: a.__setitem__(0, 0.0))),
        "pair_error_negative": ("per_pair", field("me", lambda a: a.__setitem__(2, -1.0))),
        "max_error_zero": opt(max_error=0.0), "max_error_nan": opt(max_error=float("nan")), "max_error_inf": opt(max_error=float("inf")),
        "confidence_nan": opt(confidence=float("nan")), "confidence_above_one": opt(confidence=1.5), "confidence_negative": opt(confidence=-0.1),
        "ratio_above_one": opt(min_inlier_ratio=1.5), "ratio_negative": opt(min_inlier_ratio=-0.5), "ratio_nan": opt(min_inlier_ratio=float("nan")),
        "min_trials_negative": opt(min_num_trials=-1), "no_trials": opt(max_num_trials=0, min_num_trials=0),
        "too_many_trials": opt(max_num_trials=Y.MAX_TRIALS + 1), "min_above_max_trials": opt(min_num_trials=200, max_num_trials=150),
        "min_matches_six": opt(min_matches=6), "min_num_inliers_negative": opt(min_num_inliers=-1),
        "accept_ratio_negative": opt(min_accept_ratio=-0.5), "accept_ratio_nan": opt(min_accept_ratio=float("nan")),
    }


@pytest.mark.parametrize("name", sorted(_einval_cases()))
def test_einval_without_a_device_and_outputs_untouched(lib, name, capfd):
    from xrsfm_amd import capi
    how = _einval_cases()[name]
    c, o = _Call(), capi.verify_pairs_options()
    if how is None:
        code = c.run(lib, None)
    elif isinstance(how, tuple) and how[0] == "per_pair":
        how[1](c, o)
        code = c.run(lib, o, per_pair=True)
    elif isinstance(how, tuple):
        code = c.run(lib, o, null=how)
    else:
        how(c, o)
        code = c.run(lib, o)
    assert code == capi.EINVAL
    assert c.untouched()
    err = capfd.readouterr().err
    assert err.count("\n") == 1 and "xrsfm_ba_verify_pairs" in err


def test_no_pairs_is_success_without_a_device(lib):
    from xrsfm_amd import capi
    c = _Call()
    c.n_pairs = 0
    assert c.run(lib, capi.verify_pairs_options()) == 0 and c.untouched()
    assert c.run(lib, capi.verify_pairs_options(), null=("ptr", "xa", "xb", "status", "F", "mask", "ninl", "ntr", "best", "accepted")) == 0
    r = capi.verify_pairs(np.zeros(1, np.int32), np.zeros((0, 2)), np.zeros((0, 2)))
    assert all(len(v) == 0 for v in r.values())


def test_valid_call_without_a_device_is_enodev(lib):
    import torch
    from xrsfm_amd import capi
    if torch.cuda.is_available() and capi.device_count() > 0:
        pytest.skip("a GPU is present")
    c = _Call()
    assert c.run(lib, capi.verify_pairs_options()) == -2 and c.untouched()
    assert c.run(lib, capi.verify_pairs_options(), per_pair=True, null=("ninl", "ntr", "best", "accepted")) == -2 and c.untouched()
    with pytest.raises(RuntimeError, match="ENODEV"):
        capi.verify_pairs(c.ptr, c.xa, c.xb)


def test_verified_matches_replays_the_filter():
    from xrsfm_amd import capi
    ptr = np.array([0, 3, 5, 9], np.int32)
    res = dict(inlier_mask=np.array([1, 0, 1, 1, 1, 0, 1, 1, 0], np.uint8), accepted=np.array([1, 0, 1], np.uint8))
    matches = np.arange(18).reshape(9, 2)
    kept, rows, new_ptr = capi.verified_matches(res, ptr, matches)
    assert kept.tolist() == [0, 2] and new_ptr.tolist() == [0, 2, 4] and new_ptr.dtype == np.int32
    assert rows.tolist() == [[0, 1], [4, 5], [12, 13], [14, 15]]
    kept, rows, new_ptr = capi.verified_matches(dict(inlier_mask=res["inlier_mask"], accepted=np.zeros(3, np.uint8)), ptr, matches)
    assert len(kept) == 0 and rows.shape == (0, 2) and new_ptr.tolist() == [0]
    with pytest.raises(ValueError):
        capi.verified_matches(res, ptr[:-1], matches)


# ---------------------------------------------------------------------------------------------------- sampler
def test_mt19937_is_the_standard_generator():
    g = Y.MT19937(5489)
    assert [g.next() for _ in range(10000)][-1] == 4123659995          # the value the C++ standard requires of std::mt19937


@pytest.mark.parametrize("seed,n", [(0, 7), (0, 8), (0, 15), (0, 100), (1, 64), (5489, 257), (0xFFFFFFFF, 1000), (7, 8192)])
def test_debug_fund_samples_equal_the_yardsticks_sampler(lib, seed, n):
    from xrsfm_amd import capi
    got, want = capi.debug_fund_samples(seed, n, 200), Y.sample_tuples(seed, n, 200)       # 1400 draws: past two twists of the state
    assert np.array_equal(got, want)
    assert got.min() >= 0 and got.max() < n and all(len(set(r)) == 7 for r in got.tolist())
    assert lib.xrsfm_ba_debug_fund_samples(0, 6, 1, got.ctypes.data_as(C.POINTER(C.c_int32))) == capi.EINVAL
    assert lib.xrsfm_ba_debug_fund_samples(0, 8193, 1, got.ctypes.data_as(C.POINTER(C.c_int32))) == capi.EINVAL
    assert lib.xrsfm_ba_debug_fund_samples(0, 10, Y.MAX_TRIALS + 1, got.ctypes.data_as(C.POINTER(C.c_int32))) == capi.EINVAL


# ---------------------------------------------------------------------------------------------------- the yardstick itself
def test_catalogue_coverage():
    main, deg = Y.catalogue()
    ext, E, fr = Y.reference("longdouble"), Y.entries(), Y.fragile()
    by = {e["tag"]: k for k, e in enumerate(E)}
    solid = [k for k in range(len(main)) if not fr[k]]
    assert {len(e["xa"]) for e in main} >= {7, 8, 14, 15, 16, 63, 64, 65, 255, 256, 257, 1000, 8192, 8193}
    assert ext[by["too_few"]]["status"] == 2 and ext[by["too_many"]]["status"] == 3
    assert ext[by["n7"]]["status"] == 1 and ext[by["n8"]]["status"] == 1 and by["n7"] in solid and by["n8"] in solid
    for share in ("0", "0.3"):
        assert all(by["n%d_s%s" % (n, share)] in by.values() for n in Y.LENGTHS)
    assert ext[by["n100_s0.5"]]["num_trials"] > 500 and ext[by["n100_s0.7"]]["num_trials"] == 10000       # the cap ends the scan at the defaults
    r = ext[by["pure_noise"]]
    assert r["status"] == 0 or r["accepted"] == 0
    for mt in (63, 64, 65):                                        # the abort at the last trial of a block, the first of the next, and one in
        r = ext[by["abort%d" % mt]]
        assert r["abort_trial"] == mt and r["num_trials"] == mt + 2 and by["abort%d" % mt] in solid
    assert ext[by["n64_s0"]]["abort_trial"] == 100 == Y.Options().min_num_trials                          # an abort exactly at min_num_trials
    assert ext[by["cap70"]]["num_trials"] == 70 and "cap_reached" in ext[by["cap70"]]["flags"]
    assert ext[by["confidence1"]]["num_trials"] == 130 and "abort_dyn" not in ext[by["confidence1"]]["flags"]
    assert ext[by["early_s0"]]["num_trials"] < 10
    assert Y.all_flags() >= set(Y.BRANCHES)                       # every branch, on pairs that are not fragile
    assert any(0 in ext[k]["nmodels"] for k in solid) and any(3 in ext[k]["nmodels"] for k in solid) and 0 in ext[by["origin_match"]]["nmodels"]
    local = [bool(ext[k]["best_trial"] & Y.LOCAL_BIT) for k in solid if ext[k]["status"] == 1]
    assert any(local) and not all(local)                           # a returned 8-point model, and a returned 7-point sample model
    assert {ext[k]["accepted"] for k in solid if ext[k]["status"] == 1} == {0, 1}
    assert {e["tag"] for e in deg} >= {"planar_exact", "planar", "pure_rotation", "duplicated", "collinear", "exact"}
    assert len(main) >= 50


def test_fragile_cap_and_float64_restatement_meets_every_bar():
    share = Y.fragile_share()
    print("fragile share %.3f of %d pairs" % (share, Y.n_main()))
    assert share <= Y.FRAGILE_CAP
    ext, f64, fr, E = Y.reference("longdouble"), Y.reference("float64"), Y.fragile(), Y.entries()
    checked = 0
    for k, e in enumerate(E):
        me = Y.Options(**e["opt"]).max_error
        assert not Y.always_true(f64[k], e["xa"], e["xb"], me), e["tag"]
        assert not Y.always_true(ext[k], e["xa"], e["xb"], me), e["tag"]
        if fr[k] or k >= Y.n_main():
            continue
        assert Y.same_discrete(f64[k], ext[k]), e["tag"]
        if ext[k]["status"] == 1:
            checked += 1
            assert Y.loose_ok(f64[k]["F"], ext[k]), e["tag"]
    worst = Y.restatement_deviation()
    print("float64 restatement over %d pairs: %.2e; tight bar %.2e" % (checked, worst, Y.TIGHT_BAR))
    assert checked >= 45
    assert Y.RESTATEMENT_DEVIATION / 4 <= worst <= Y.RESTATEMENT_DEVIATION       # the named constant is the measurement: not below it, not inflated
    assert Y.TIGHT_BAR == 16 * Y.RESTATEMENT_DEVIATION


def test_the_checks_reject_a_wrong_result():
    E = Y.entries()
    k = next(k for k, e in enumerate(E) if e["tag"] == "n64_s0.3")
    e, r = E[k], Y.reference("longdouble")[k]
    good = dict(r, F=np.asarray(r["F"], np.float64))
    assert Y.loose_ok(good["F"], r) and not Y.always_true(good, e["xa"], e["xb"], 4.0) and Y.deviation(good["F"], r) <= Y.TIGHT_BAR
    transposed = dict(good, F=good["F"].reshape(3, 3).T.ravel().copy())
    assert not Y.loose_ok(transposed["F"], r) and Y.always_true(transposed, e["xa"], e["xb"], 4.0) and Y.deviation(transposed["F"], r) > Y.TIGHT_BAR
    negated = dict(good, F=-good["F"])
    assert not Y.loose_ok(negated["F"], r) and Y.always_true(negated, e["xa"], e["xb"], 4.0)
    flipped = dict(good, mask=good["mask"].copy())
    flipped["mask"][0] ^= 1
    assert not Y.same_discrete(flipped, r) and Y.always_true(flipped, e["xa"], e["xb"], 4.0)
    assert not Y.same_discrete(dict(good, num_trials=good["num_trials"] + 1), r)
    assert Y.always_true(dict(good, num_trials=0), e["xa"], e["xb"], 4.0)


# ---------------------------------------------------------------------------------------------------- the headers on the host
def test_scan_header_reproduces_the_yardstick(tmp_path):
    """ba_fund_scan.h fed the yardstick's per-model records: the same best model and trial count, a local optimisation exactly where
    the yardstick ran one, and it stops where the yardstick stops."""
    exe = H.build(tmp_path, "scan", H.SCAN_DRIVER)
    ext, E, lines, want = Y.reference("longdouble"), Y.entries(), [], []
    for k, r in enumerate(ext):
        if r["status"] >= 2:
            continue
        opt = Y.Options(**E[k]["opt"])
        lines.append("%d %d %d %r %d" % (r["scan"]["n"], Y.trial_cap(opt), opt.min_num_trials, opt.confidence, len(r["records"])))
        lines += ["%d %d %r %d %r" % tuple(rec) for rec in r["records"]]
        s = r["scan"]
        want.append((-1 if s["best_trial"] < 0 else s["best_trial"] | (Y.LOCAL_BIT if s["local"] else 0), s["num_trials"], s["success"], 0))
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    got = [tuple(int(x) for x in ln.split()) for ln in out if ln]
    assert len(got) == len(want) >= 55
    assert [(g[0], g[1], g[3], g[4]) for g in got] == want
    # a truncated record list is noticed: the scan of a pair that aborts has not stopped one record earlier
    k = next(k for k, e in enumerate(E) if e["tag"] == "abort64")
    r, opt = ext[k], Y.Options(**E[k]["opt"])
    text = "\n".join(["%d %d %d %r %d" % (r["scan"]["n"], Y.trial_cap(opt), opt.min_num_trials, opt.confidence, len(r["records"]) - 1)] +
                     ["%d %d %r %d %r" % tuple(rec) for rec in r["records"][:-1]]) + "\n"
    g = [int(x) for x in subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split()]
    assert g[1] != r["num_trials"]


def run_pair_driver(exe, ks):
    E = Y.entries()
    text = "\n".join(H.pair_input(E[k]["xa"], E[k]["xb"], Y.Options(**E[k]["opt"])) for k in ks) + "\n"
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.strip().split("\n")
    assert len(out) == len(ks)
    return {k: H.parse_pair(ln, len(E[k]["xa"])) for k, ln in zip(ks, out)}


def check_against_yardstick(results, label):
    """results: catalogue index -> dict of the outputs of one implementation; the checks of DESIGN.md 5k"""
    ext, fr, E, worst, checked = Y.reference("longdouble"), Y.fragile(), Y.entries(), 0.0, 0
    for k, got in results.items():
        e = E[k]
        assert not Y.always_true(got, e["xa"], e["xb"], Y.Options(**e["opt"]).max_error), (label, e["tag"])
        if fr[k] or k >= Y.n_main():
            continue
        assert Y.same_discrete(got, ext[k]), (label, e["tag"], [(x, got[x], ext[k][x]) for x in Y.DISCRETE])
        if ext[k]["status"] == 1:
            checked += 1
            assert Y.loose_ok(got["F"], ext[k]), (label, e["tag"])
            worst = max(worst, Y.deviation(got["F"], ext[k]))
    print("%s: %d pairs, largest deviation of F %.2e; tight bar %.2e" % (label, checked, worst, Y.TIGHT_BAR))
    assert worst <= Y.TIGHT_BAR, (label, worst)
    return checked


def test_geometry_headers_on_the_host_meet_every_bar(tmp_path):
    """The library's own arithmetic (7-point solver, cubic, 8-point model, the scan, the sampler) without the kernel around it,
    under the sanitizers: on every non-fragile pair the discrete outputs equal the extended yardstick's and F meets both bars."""
    exe = H.build(tmp_path, "pairs", H.PAIR_DRIVER)
    ks = list(range(len(Y.entries())))
    assert check_against_yardstick(run_pair_driver(exe, ks), "sequential host driver") >= 45


def test_verify_kernel_does_not_spill(tmp_path):
    """k_verify_pairs of the gfx950 code object has no spilled VGPR and no private (scratch) segment."""
    from xrsfm_amd import _build
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    asm = tmp_path / "xba.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-Wno-unused-value",
                    "-Wno-deprecated-declarations", os.path.join(_build.CSRC, "xrsfm_ba.hip"), "-o", str(asm)], check=True, capture_output=True)
    seen = 0
    for blk in asm.read_text().split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        if "k_verify_pairs" not in name:
            continue
        seen += 1
        spills = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1))
        scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1))
        assert spills == 0 and scratch == 0, (name, spills, scratch)
    assert seen == 1
