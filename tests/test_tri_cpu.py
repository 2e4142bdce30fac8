"""xrsfm_ba_triangulate_tracks without a GPU: the interface (exports, struct layout, defaults, every EINVAL, the empty call, ENODEV),
the yardstick's own checks (fragile cap, float64 against extended, catalogue coverage, the model bar for the float64 restatement),
the scan rule of xrsfm_amd/csrc/ba_tri_scan.h compiled for the host and driven with the yardstick's per-trial records, and the
resource usage of the kernel in the gfx950 code object."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import tri_yardstick as Y

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0x5A


def test_exports_and_struct_layout(lib, tmp_path):
    from xrsfm_amd import capi
    for name in ("xrsfm_ba_triangulate_options", "xrsfm_ba_triangulate_tracks"):
        assert name in capi.EXPORTS and getattr(lib, name) is not None
    src = tmp_path / "p.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "xrsfm_ba.h"\nint main(){printf("%zu %zu %zu %d\\n", '
                   'sizeof(xrsfm_ba_tri_options), offsetof(xrsfm_ba_tri_options, max_num_trials), '
                   'offsetof(xrsfm_ba_tri_options, exhaustive_threshold), XRSFM_BA_TRI_MAX_OBS);return 0;}\n')
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "p")], check=True)
    out = [int(x) for x in subprocess.run([str(tmp_path / "p")], capture_output=True, text=True, check=True).stdout.split()]
    assert out == [C.sizeof(capi.CTriOptions), capi.CTriOptions.max_num_trials.offset, capi.CTriOptions.exhaustive_threshold.offset,
                   capi.TRI_MAX_OBS]
    assert capi.TRI_MAX_OBS == Y.MAX_OBS and capi.TRI_LOCAL_BIT == Y.LOCAL_BIT


def test_default_options_are_the_reference_values(lib):
    from xrsfm_amd import capi
    o = capi.triangulate_options()
    assert (o.min_tri_angle_rad, o.max_error_rad) == (pytest.approx(math.radians(1.5), rel=1e-15), pytest.approx(math.radians(2.0), rel=1e-15))
    assert (o.confidence, o.min_inlier_ratio, o.max_num_trials, o.exhaustive_threshold) == (0.9999, 0.02, 10000, 15)
    y = Y.Options()
    assert (y.confidence, y.min_inlier_ratio, y.max_num_trials, y.exhaustive_threshold) == (0.9999, 0.02, 10000, 15)


class _Call:
    """A small valid problem and sentinel-filled outputs for the raw C call."""
    def __init__(self):
        quat, t, ptr, ocam, oxy, _ = Y.case_arrays("four")
        self.q, self.t, self.ptr, self.ocam, self.oxy = quat.copy(), t.copy(), ptr.copy(), ocam.copy(), oxy.copy()
        nt, no = len(ptr) - 1, len(ocam)
        self.points = np.full((nt, 3), 1234.5); self.status = np.full(nt, SENTINEL, np.uint8); self.mask = np.full(no, SENTINEL, np.uint8)
        self.ninl = np.full(nt, -77, np.int32); self.ntr = np.full(nt, -77, np.int32); self.best = np.full(nt, -77, np.int32)
        self.n_cams, self.n_tracks = len(quat), nt

    def untouched(self):
        return (np.all(self.points == 1234.5) and np.all(self.status == SENTINEL) and np.all(self.mask == SENTINEL) and
                np.all(self.ninl == -77) and np.all(self.ntr == -77) and np.all(self.best == -77))

    def run(self, lib, opt, null=()):
        from xrsfm_amd import capi
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        up = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))
        a = dict(opt=C.byref(opt) if opt is not None else None, q=dp(self.q), t=dp(self.t), ptr=ip(self.ptr), ocam=ip(self.ocam), oxy=dp(self.oxy),
                 points=dp(self.points), status=up(self.status), mask=up(self.mask), ninl=ip(self.ninl), ntr=ip(self.ntr), best=ip(self.best))
        for k in null:
            a[k] = None
        return lib.xrsfm_ba_triangulate_tracks(a["opt"], self.n_cams, a["q"], a["t"], self.n_tracks, a["ptr"], a["ocam"], a["oxy"], a["points"],
                                               a["status"], a["mask"], a["ninl"], a["ntr"], a["best"])


def _einval_cases():
    def opt(**kw):
        return lambda c, o: [setattr(o, k, v) for k, v in kw.items()]

    def field(name, fn):
        return lambda c, o: fn(getattr(c, name))
    cases = {
        "null_opt": None, "null_points": ("points",), "null_status": ("status",), "null_mask": ("mask",),
        "negative_tracks": lambda c, o: setattr(c, "n_tracks", -1), "negative_cams": lambda c, o: setattr(c, "n_cams", -1),
        "ptr_not_from_zero": field("ptr", lambda p: p.__setitem__(0, 1)),
        "ptr_decreasing": field("ptr", lambda p: p.__setitem__(2, int(p[1]) - 1)),
        "obs_cam_negative": field("ocam", lambda a: a.__setitem__(3, -1)),
        "obs_cam_too_large": lambda c, o: c.ocam.__setitem__(3, c.n_cams),
        "pose_q_nan": field("q", lambda a: a.__setitem__((5, 2), np.nan)), "pose_t_inf": field("t", lambda a: a.__setitem__((5, 1), np.inf)),
        "xy_nan": field("oxy", lambda a: a.__setitem__((1, 0), np.nan)),
        "opt_nan": opt(min_tri_angle_rad=float("nan")), "opt_inf": opt(max_error_rad=float("inf")),
        "max_error_zero": opt(max_error_rad=0.0), "max_error_negative": opt(max_error_rad=-0.1),
        "confidence_above_one": opt(confidence=1.5), "confidence_negative": opt(confidence=-0.1),
        "ratio_above_one": opt(min_inlier_ratio=1.01), "ratio_negative": opt(min_inlier_ratio=-1e-3),
        "no_trials": opt(max_num_trials=0), "threshold_negative": opt(exhaustive_threshold=-1), "angle_negative": opt(min_tri_angle_rad=-1e-3),
    }
    return cases


@pytest.mark.parametrize("name", sorted(_einval_cases()))
def test_einval_without_a_device_and_outputs_untouched(lib, name, capfd):
    from xrsfm_amd import capi
    how = _einval_cases()[name]
    c, o = _Call(), capi.triangulate_options()
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
    assert err.count("\n") == 1 and "xrsfm_ba_triangulate_tracks" in err


def test_no_tracks_is_success_without_a_device(lib):
    from xrsfm_amd import capi
    c = _Call()
    c.n_tracks = 0
    assert c.run(lib, capi.triangulate_options()) == 0 and c.untouched()
    assert c.run(lib, capi.triangulate_options(), null=("points", "status", "mask", "ptr", "ocam", "oxy", "q", "t")) == 0
    r = capi.triangulate_tracks(np.zeros((0, 4)), np.zeros((0, 3)), np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros((0, 2)))
    assert all(len(v) == 0 for v in r.values())


def test_valid_call_without_a_device_is_enodev(lib):
    import torch
    from xrsfm_amd import capi
    if torch.cuda.is_available() and capi.device_count() > 0:
        pytest.skip("a GPU is present")
    c = _Call()
    assert c.run(lib, capi.triangulate_options()) == -2 and c.untouched()
    quat, t, ptr, ocam, oxy, _ = Y.case_arrays("four")
    with pytest.raises(RuntimeError, match="ENODEV"):
        capi.triangulate_tracks(quat, t, ptr, ocam, oxy)


# ---------------------------------------------------------------------------------------------------- the yardstick itself
def test_catalogue_coverage():
    P, ext, by, cases = Y.pool(), Y.reference("longdouble"), Y.tags(), Y.cases()
    lengths = {len(P[k]["cams"]) for k in cases["lengths"]}
    assert lengths >= set(Y.LENGTHS)
    status_of = lambda n: {ext[k]["status"] for k in cases["lengths"] if len(P[k]["cams"]) == n}
    assert status_of(0) == {2} and status_of(1) == {2} and status_of(129) == {3}
    for n in (2, 3, 4, 11, 12, 15, 16, 17, 64, 65, 128):
        assert 1 in status_of(n), n
    for name in Y.REQUIRED:
        assert by.get(name), name
    everything = set().union(*[set(v) for v in cases.values()])
    for name in Y.REQUIRED:                       # ... and the cases run at least one track of each
        assert everything & set(by[name]), name
    one = lambda name: ext[by[name][0]]
    assert one("all_pairs_low_angle")["status"] == 0 and one("all_pairs_low_angle")["flags"] == {"low_angle_pair"}
    assert "behind_camera" in one("behind_camera")["flags"] and one("behind_camera")["status"] == 0
    assert all("zero_inlier_model" in ext[k]["flags"] for k in by["zero_inlier_model"])
    assert {ext[k]["status"] for k in by["zero_inlier_model"]} == {0, 1}        # alone, and in front of a consistent track
    e = one("inliers16_abort_after_trial_1")
    assert (e["status"], e["num_inliers"], e["num_trials"]) == (1, 16, 3) and "aborted" in e["flags"]
    e = one("long_20pct_inliers")
    assert e["status"] == 1 and e["num_inliers"] == 8 and e["num_trials"] >= 200
    assert "refit_no_model" in one("refit_no_model")["flags"]
    e, tr = one("same_camera_twice"), P[by["same_camera_twice"][0]]
    assert len(set(tr["cams"].tolist())) < len(tr["cams"]) and e["status"] == 1
    assert all(ext[k]["best_trial"] & Y.LOCAL_BIT for k in by["refit_wins"])
    assert all(ext[k]["status"] == 1 and not ext[k]["best_trial"] & Y.LOCAL_BIT and ext[k]["num_inliers"] > 2 for k in by["refit_loses"])
    assert sorted(len(v) for v in cases.values())[:3] == [1, 4, 5] and len(cases["b257"]) == 257
    assert sum("aborted" in e["flags"] for e in ext) >= 50 and sum(e["status"] == 0 for e in ext) >= 10
    # no noise-free track: every residual the scans looked at stays away from the acos guard
    assert all(e["margin"] > 0 for e in ext)


def test_fragile_cap_and_float64_agreement():
    ext, f64, fr, cases = Y.reference("longdouble"), Y.reference("float64"), Y.fragile(), Y.cases()
    for name, idx in cases.items():
        n_frag = int(fr[idx].sum())
        print(name, "tracks", len(idx), "fragile", n_frag, "smallest margin %.3g" % min(ext[k]["margin"] for k in idx))
        assert n_frag <= 0.01 * len(idx), name
    random = [k for k, tr in enumerate(Y.pool()) if tr["tag"] == "random"]
    assert not fr[random].any()                                                  # the expectation for random noisy tracks: none
    for k in np.flatnonzero(~fr):
        assert Y.same_discrete(ext[k], f64[k]), k
        if ext[k]["status"] == 1:
            assert np.allclose(np.asarray(f64[k]["point"], np.float64), np.asarray(ext[k]["point"], np.float64), rtol=1e-6, atol=1e-9)


def test_float64_restatement_meets_the_model_bar():
    quat, t, _ = Y.cameras()
    f64, worst = Y.reference("float64"), 0.0
    for k, tr in enumerate(Y.pool()):
        if f64[k]["status"] != 1:
            continue
        M, lam, m = Y.bar_matrix(quat, t, tr["cams"], tr["xy"], f64[k]["best_trial"])
        excess, bar = Y.bar_check(f64[k]["point"], M, lam, m)
        worst = max(worst, excess / bar)
        assert excess <= bar, (k, tr["tag"], excess, bar)
    print("largest excess / bar of the float64 restatement: %.3g" % worst)


def test_bar_rejects_a_sloppy_null_vector():
    """the bar is not vacuous: a model displaced by 1.4e-3 across the viewing rays (1e-4 of its depth and more) misses it"""
    quat, t, _ = Y.cameras()
    f64, missed, seen = Y.reference("float64"), 0, 0
    for k, tr in enumerate(Y.pool()):
        if f64[k]["status"] != 1 or seen >= 40:
            continue
        seen += 1
        M, lam, m = Y.bar_matrix(quat, t, tr["cams"], tr["xy"], f64[k]["best_trial"])
        X = np.asarray(f64[k]["point"], np.float64)
        excess, bar = Y.bar_check(X + 1e-3 * np.array([1.0, -1.0, 0.0]), M, lam, m)
        missed += excess > bar
    assert missed == seen == 40, (missed, seen)


# ---------------------------------------------------------------------------------------------------- the scan header on the host
_SCAN_DRIVER = r"""
#include <cstdio>
#include <vector>
#include "ba_tri_scan.h"
// per track: "n max_num_trials min_inlier_ratio confidence exhaustive_threshold R", then R records "has count sum refit_count refit_sum"
// (refit_count -2: the yardstick made no refit, -1: its refit had no model); one line "best_trial local num_trials success used err"
int main() {
    int n, cap, thr, R;
    double ratio, conf;
    while (std::scanf("%d %d %lf %lf %d %d", &n, &cap, &ratio, &conf, &thr, &R) == 6) {
        std::vector<int32_t> row(n + 1);
        for (int k = 0; k <= n; ++k) row[k] = xtri::tri_dyn_trials(k, n, conf);
        const int32_t ratio_cap = xtri::tri_ratio_trials(ratio, conf);
        xtri::Scan sc(row.data(), n, cap < ratio_cap ? cap : ratio_cap, thr);
        int used = 0, err = 0;
        bool stopped = false;
        for (int t = 0; t < R; ++t) {
            int has, cnt, rc;
            double sum, rs;
            if (std::scanf("%d %d %lf %d %lf", &has, &cnt, &sum, &rc, &rs) != 5) return 1;
            if (stopped) continue;
            if (t >= sc.max_trials) { err |= 4; continue; }
            ++used;
            const xtri::Offer o = sc.offer(t, has != 0, cnt, sum);
            if (o == xtri::kNewBestRefit) {
                if (rc == -2) err |= 1;
                else if (rc >= 0) sc.offer_local(rc, rs);
            } else if (rc != -2) err |= 2;
            stopped = sc.after_trial(t);
        }
        if (!stopped && used != sc.max_trials) err |= 8;
        std::printf("%d %d %d %d %d %d\n", sc.best_trial, (int)sc.best_local, sc.num_trials, (int)sc.finish(), used, err);
    }
    return 0;
}
"""


@pytest.mark.parametrize("opt_items", [(), (("max_num_trials", 7), ("exhaustive_threshold", 0), ("confidence", 0.99))], ids=["defaults", "capped"])
def test_scan_header_reproduces_the_yardstick(tmp_path, opt_items):
    """ba_tri_scan.h, compiled for the host with the address and undefined-behaviour sanitizers (a stand-alone program), fed the
    yardstick's per-trial records of the whole catalogue: the same best trial, local flag, trial count and success, and it stops
    at the trial the yardstick stops at."""
    from xrsfm_amd import _build
    src, exe = tmp_path / "scan.cc", tmp_path / "scan"
    src.write_text(_SCAN_DRIVER)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", _build.CSRC, str(src),
                    "-o", str(exe)], check=True)
    opt, ext = Y.Options(**dict(opt_items)), Y.reference("longdouble", opt_items)
    lines, want = [], []
    for e in ext:
        if "scan" not in e:
            continue
        s = e["scan"]
        lines.append("%d %d %r %r %d %d" % (s["n"], opt.max_num_trials, opt.min_inlier_ratio, opt.confidence, opt.exhaustive_threshold, len(e["records"])))
        lines += ["%d %d %r %d %r" % tuple(r) for r in e["records"]]
        want.append((s["best_trial"], s["local"], s["num_trials"], s["success"], len(e["records"]), 0))
    out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    got = [tuple(int(x) for x in ln.split()) for ln in out if ln]
    assert len(got) == len(want) > 200
    assert got == want
    assert xtri_bounds_are_the_reference_values()


def xtri_bounds_are_the_reference_values():
    return Y.num_trials_bound(2000, 100000, 0.9999) == 23022 and Y.num_trials_bound(16, 16, 0.9999) == 1 and \
        Y.num_trials_bound(0, 16, 0.9999) == Y.UNBOUNDED and Y.num_trials_bound(8, 16, 1.0) == Y.UNBOUNDED


def test_combination_order_is_lexicographic():
    import itertools
    for n in (2, 3, 4, 7, 12, 65, 128):
        i, j = Y.pairs_of(n)
        assert list(zip(i.tolist(), j.tolist())) == list(itertools.combinations(range(n), 2))


# ---------------------------------------------------------------------------------------------------- the kernel's code object
def test_tri_kernels_do_not_spill(tmp_path):
    """Every kernel of the gfx950 code object whose name contains k_tri has no spilled VGPR and no private (scratch) segment."""
    from xrsfm_amd import _build
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    asm = tmp_path / "xba.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-Wno-unused-value",
                    "-Wno-deprecated-declarations", os.path.join(_build.CSRC, "xrsfm_ba.hip"), "-o", str(asm)], check=True, capture_output=True)
    seen = 0
    for blk in asm.read_text().split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        if "k_tri" not in name:
            continue
        seen += 1
        spills = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1))
        scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1))
        lds = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", blk).group(1))
        assert spills == 0 and scratch == 0, (name, spills, scratch)
        assert lds <= 80 * 1024, (name, lds)             # two workgroups per compute unit of 160 KiB
    assert seen >= 1
