"""xrsfm_ba_absolute_pose without a GPU: the interface (exports, struct layout, defaults, every EINVAL, the empty call, ENODEV), the
sampler against the yardstick's, the yardstick's own checks (MT19937, fragile cap, catalogue coverage, the bars for the float64
restatement), and the headers on the host: ba_pnp_scan.h driven with the yardstick's per-model records, and ba_pnp_geom.h with it in
a sequential driver of whole frames, both as stand-alone programs built with the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import pose_yardstick as Y

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0x5A


def test_exports_and_struct_layout(lib, tmp_path):
    from xrsfm_amd import capi
    for name in ("xrsfm_ba_absolute_pose_options", "xrsfm_ba_absolute_pose", "xrsfm_ba_debug_pose_samples"):
        assert name in capi.EXPORTS and getattr(lib, name) is not None
    src = tmp_path / "p.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "xrsfm_ba.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu %d %d\\n", '
                   'sizeof(xrsfm_ba_pose_options), offsetof(xrsfm_ba_pose_options, confidence), offsetof(xrsfm_ba_pose_options, min_inlier_ratio), '
                   'offsetof(xrsfm_ba_pose_options, min_num_trials), offsetof(xrsfm_ba_pose_options, max_num_trials), '
                   'offsetof(xrsfm_ba_pose_options, seed), XRSFM_BA_POSE_MAX_CORR, XRSFM_BA_POSE_MAX_TRIALS);return 0;}\n')
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "p")], check=True)
    out = [int(x) for x in subprocess.run([str(tmp_path / "p")], capture_output=True, text=True, check=True).stdout.split()]
    o = capi.CPoseOptions
    assert out == [C.sizeof(o), o.confidence.offset, o.min_inlier_ratio.offset, o.min_num_trials.offset, o.max_num_trials.offset, o.seed.offset,
                   capi.POSE_MAX_CORR, capi.POSE_MAX_TRIALS]
    assert (capi.POSE_MAX_CORR, capi.POSE_MAX_TRIALS, capi.POSE_LOCAL_BIT) == (Y.MAX_CORR, Y.MAX_TRIALS, Y.LOCAL_BIT)


def test_default_options_are_the_reference_values(lib):
    from xrsfm_amd import capi
    o, y = capi.absolute_pose_options(), Y.Options()
    for got in (o, y):
        assert (got.max_error, got.confidence, got.min_inlier_ratio, got.min_num_trials, got.max_num_trials, got.seed) == \
            (8.0 / 800.0, 0.9999, 0.25, 100, 16384, 0)
    assert Y.trial_cap(y) == 585                        # the constructor's bound from min_inlier_ratio


class _Call:
    """A small valid problem and sentinel-filled outputs for the raw C call."""
    def __init__(self):
        idx = [k for k, f in enumerate(Y.pool()) if f["tag"] in ("len5", "len20", "two")]
        ptr, xy, X = Y.arrays(idx)
        self.ptr, self.xy, self.X = ptr.copy(), xy.copy(), X.copy()
        nf, n = len(idx), len(xy)
        self.q = np.full((nf, 4), 1234.5); self.t = np.full((nf, 3), 1234.5); self.status = np.full(nf, SENTINEL, np.uint8)
        self.mask = np.full(n, SENTINEL, np.uint8)
        self.ninl = np.full(nf, -77, np.int32); self.ntr = np.full(nf, -77, np.int32); self.best = np.full(nf, -77, np.int32)
        self.fme = np.full(nf, 0.01); self.fseed = np.zeros(nf, np.uint32)
        self.n_frames = nf

    def untouched(self):
        return (np.all(self.q == 1234.5) and np.all(self.t == 1234.5) and np.all(self.status == SENTINEL) and np.all(self.mask == SENTINEL) and
                np.all(self.ninl == -77) and np.all(self.ntr == -77) and np.all(self.best == -77))

    def run(self, lib, opt, null=(), per_frame=False):
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        up = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))
        a = dict(opt=C.byref(opt) if opt is not None else None, ptr=ip(self.ptr), xy=dp(self.xy), X=dp(self.X),
                 fme=dp(self.fme) if per_frame else None, fseed=self.fseed.ctypes.data_as(C.POINTER(C.c_uint32)) if per_frame else None,
                 q=dp(self.q), t=dp(self.t), status=up(self.status), mask=up(self.mask), ninl=ip(self.ninl), ntr=ip(self.ntr), best=ip(self.best))
        for k in null:
            a[k] = None
        return lib.xrsfm_ba_absolute_pose(a["opt"], self.n_frames, a["ptr"], a["xy"], a["X"], a["fme"], a["fseed"], a["q"], a["t"], a["status"],
                                          a["mask"], a["ninl"], a["ntr"], a["best"])


def _einval_cases():
    def opt(**kw):
        return lambda c, o: [setattr(o, k, v) for k, v in kw.items()]

    def field(name, fn, per_frame=False):
        f = lambda c, o: fn(getattr(c, name))
        f.per_frame = per_frame
        return f
    return {
        "null_opt": None, "null_q": ("q",), "null_t": ("t",), "null_status": ("status",), "null_mask": ("mask",),
        "negative_frames": lambda c, o: setattr(c, "n_frames", -1),
        "ptr_not_from_zero": field("ptr", lambda p: p.__setitem__(0, 1)),
        "ptr_decreasing": field("ptr", lambda p: p.__setitem__(2, int(p[1]) - 1)),
        "xy_nan": field("xy", lambda a: a.__setitem__((1, 0), np.nan)), "xy_inf": field("xy", lambda a: a.__setitem__((3, 1), np.inf)),
        "point_nan": field("X", lambda a: a.__setitem__((2, 2), np.nan)), "point_inf": field("X", lambda a: a.__setitem__((0, 0), -np.inf)),
        "max_error_nan": opt(max_error=float("nan")), "max_error_inf": opt(max_error=float("inf")),
        "max_error_zero": opt(max_error=0.0), "max_error_negative": opt(max_error=-0.1),
        "frame_max_error_nan": field("fme", lambda a: a.__setitem__(1, np.nan), True),
        "frame_max_error_zero": field("fme", lambda a: a.__setitem__(2, 0.0), True),
        "frame_max_error_negative": field("fme", lambda a: a.__setitem__(0, -1.0), True),
        "confidence_nan": opt(confidence=float("nan")), "confidence_above_one": opt(confidence=1.5), "confidence_negative": opt(confidence=-0.1),
        "ratio_inf": opt(min_inlier_ratio=float("inf")), "ratio_above_one": opt(min_inlier_ratio=1.01), "ratio_negative": opt(min_inlier_ratio=-1e-3),
        "min_trials_negative": opt(min_num_trials=-1), "no_trials": opt(max_num_trials=0, min_num_trials=0),
        "too_many_trials": opt(max_num_trials=Y.MAX_TRIALS + 1), "min_above_max": opt(min_num_trials=11, max_num_trials=10),
    }


@pytest.mark.parametrize("name", sorted(_einval_cases()))
def test_einval_without_a_device_and_outputs_untouched(lib, name, capfd):
    from xrsfm_amd import capi
    how = _einval_cases()[name]
    c, o = _Call(), capi.absolute_pose_options()
    if how is None:
        code = c.run(lib, None)
    elif isinstance(how, tuple):
        code = c.run(lib, o, null=how)
    else:
        how(c, o)
        code = c.run(lib, o, per_frame=getattr(how, "per_frame", False))
    assert code == capi.EINVAL
    assert c.untouched()
    err = capfd.readouterr().err
    assert err.count("\n") == 1 and "xrsfm_ba_absolute_pose" in err


def test_no_frames_is_success_without_a_device(lib):
    from xrsfm_amd import capi
    c = _Call()
    c.n_frames = 0
    assert c.run(lib, capi.absolute_pose_options()) == 0 and c.untouched()
    assert c.run(lib, capi.absolute_pose_options(), null=("ptr", "xy", "X", "q", "t", "status", "mask", "ninl", "ntr", "best")) == 0
    r = capi.absolute_pose(np.zeros(1, np.int32), np.zeros((0, 2)), np.zeros((0, 3)))
    assert all(len(v) == 0 for v in r.values())


def test_valid_call_without_a_device_is_enodev(lib):
    import torch
    from xrsfm_amd import capi
    if torch.cuda.is_available() and capi.device_count() > 0:
        pytest.skip("a GPU is present")
    c = _Call()
    assert c.run(lib, capi.absolute_pose_options()) == -2 and c.untouched()
    assert c.run(lib, capi.absolute_pose_options(), per_frame=True) == -2 and c.untouched()
    with pytest.raises(RuntimeError, match="ENODEV"):
        capi.absolute_pose(c.ptr, c.xy, c.X)


# ---------------------------------------------------------------------------------------------------- sampler
def test_mt19937_is_the_standard_generator():
    g = Y.MT19937(5489)
    assert [g.next() for _ in range(10000)][-1] == 4123659995          # the value the C++ standard requires of std::mt19937


@pytest.mark.parametrize("seed,n", [(0, 3), (0, 4), (0, 5), (0, 100), (1, 64), (5489, 257), (0xFFFFFFFF, 1000), (7, 8192)])
def test_debug_pose_samples_equal_the_yardsticks_sampler(lib, seed, n):
    from xrsfm_amd import capi
    got, want = capi.debug_pose_samples(seed, n, 600), Y.sample_triples(seed, n, 600)
    assert np.array_equal(got, want)
    assert got.min() >= 0 and got.max() < n and all(len(set(r)) == 3 for r in got.tolist())
    assert lib.xrsfm_ba_debug_pose_samples(0, 2, 1, got.ctypes.data_as(C.POINTER(C.c_int32))) == capi.EINVAL


# ---------------------------------------------------------------------------------------------------- the yardstick itself
def test_catalogue_coverage():
    P, ext = Y.pool(), Y.reference("longdouble")
    by = {}
    for k, f in enumerate(P):
        by.setdefault(f["tag"], []).append(k)
    assert {len(P[k]["xy"]) for k in range(len(P))} >= set(Y.LENGTHS) | {2, Y.MAX_CORR + 1}
    assert {e["status"] for e in ext.values()} == {0, 1, 2, 3}
    st = lambda tag: ext[by[tag][0]]["status"]
    assert (st("two"), st("empty"), st("too_long"), st("one_point_only")) == (2, 2, 3, 0)
    assert all(st("len%d" % n) == 1 for n in Y.LENGTHS) and all(st("share%g" % s) == 1 for s in (0.0, 0.3, 0.6, 0.8))
    flags = Y.all_flags()
    for name in Y.BRANCHES:
        assert name in flags, name
    assert "cap_reached" in ext[by["share0.8"][0]]["flags"] and ext[by["share0.8"][0]]["num_trials"] == 585
    assert "local_no_model" in ext[by["planar"][0]]["flags"] and not ext[by["planar"][0]]["best_trial"] & Y.LOCAL_BIT
    e, f = ext[by["behind_camera"][0]], P[by["behind_camera"][0]]
    depth = (f["X"] @ np.asarray(e["P"][:, :3], np.float64).T + np.asarray(e["t"], np.float64))[:, 2]
    assert (depth < 0).sum() == 10 and not e["mask"][depth < 0].any()
    assert "trial_without_model" in ext[by["repeated_point"][0]]["flags"]
    # the option sets: an abort inside the first block, and the cap inside, at and just past a block
    assert all(e["num_trials"] < 64 for k, e in Y.reference("longdouble", "early").items() if P[k]["tag"] != "share0.6")
    for name, cap in (("cap7", 7), ("cap64", 64), ("cap65", 65)):
        assert {e["num_trials"] for e in Y.reference("longdouble", name).values()} == {cap}


def test_fragile_cap_and_float64_restatement_meets_every_bar():
    share, worst = Y.fragile_share(), 0.0
    print("fragile share %.3f" % share)
    assert share <= Y.FRAGILE_CAP
    for name in Y.OPTION_SETS:
        ext, f64, fr, P = Y.reference("longdouble", name), Y.reference("float64", name), Y.fragile(name), Y.pool()
        for k, e in ext.items():
            d = f64[k]
            if d["status"] == 1:
                assert np.isfinite(np.asarray(d["P"], np.float64)).all() and abs(float((d["q"] ** 2).sum()) - 1.0) <= 8 * 2.0 ** -53
                assert d["num_inliers"] == int(d["mask"].sum())
                assert Y.mask_check(np.asarray(d["q"], np.float64), np.asarray(d["t"], np.float64), P[k]["xy"], P[k]["X"], Y.Options().max_error, d["mask"])
            if fr[k]:
                continue
            assert Y.same_discrete(d, e), (name, k)
            if e["status"] == 1:
                R, t = np.asarray(d["P"][:, :3], np.float64), np.asarray(d["t"], np.float64)
                assert np.allclose(R, np.asarray(e["P"][:, :3], np.float64), rtol=1e-6, atol=1e-9)
                assert np.allclose(t, np.asarray(e["t"], np.float64), rtol=1e-6, atol=1e-9)
                worst = max(worst, Y.deviation(R, t, e))
    print("float64 restatement: largest deviation %.3e, tight bar %.3e" % (worst, Y.TIGHT_BAR))
    assert worst == Y.restatement_deviation()
    # the named constant is the measurement: not below it, and not inflated
    assert Y.RESTATEMENT_DEVIATION / 4 <= worst <= Y.RESTATEMENT_DEVIATION
    assert Y.TIGHT_BAR == Y.TIGHT_FACTOR * Y.RESTATEMENT_DEVIATION and Y.TIGHT_FACTOR == 16


def test_quaternion_and_mask_check_reject_a_wrong_pose():
    """the self-consistency check is not vacuous: a pose rotated by 0.04 rad (four times max_error) no longer reproduces the mask"""
    k = next(k for k, f in enumerate(Y.pool()) if f["tag"] == "share0.3")
    e, f = Y.reference("longdouble")[k], Y.pool()[k]
    q, t = np.asarray(e["q"], np.float64), np.asarray(e["t"], np.float64)
    assert Y.mask_check(q, t, f["xy"], f["X"], Y.MAX_ERROR, e["mask"])
    assert np.allclose(np.asarray(Y.quat_to_mat(q), np.float64), np.asarray(e["P"][:, :3], np.float64), atol=1e-15) and q[3] >= 0
    q2 = q + np.array([2e-2, 0, 0, 0])
    assert not Y.mask_check(q2 / np.linalg.norm(q2), t, f["xy"], f["X"], Y.MAX_ERROR, e["mask"])


# ---------------------------------------------------------------------------------------------------- the headers on the host
def _build_host(tmp_path, name, text):
    from xrsfm_amd import _build
    src, exe = tmp_path / (name + ".cc"), tmp_path / name
    src.write_text(text)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", _build.CSRC, str(src),
                    "-o", str(exe)], check=True)
    return str(exe)


_SCAN_DRIVER = r"""
#include <cstdio>
#include <vector>
#include "ba_pnp_scan.h"
// per frame: "n max_num_trials min_num_trials min_inlier_ratio confidence R", then R records "trial count sum local_count local_sum" in
// the order the models were offered (local_count -2: the yardstick made no local optimisation, -1: it had no model); one line
// "best_trial local num_trials success used err"
int main() {
    int n, cap, mint, R;
    double ratio, conf;
    while (std::scanf("%d %d %d %lf %lf %d", &n, &cap, &mint, &ratio, &conf, &R) == 6) {
        std::vector<int32_t> row(n + 1);
        for (int k = 0; k <= n; ++k) row[k] = xpnp::pnp_dyn_trials(k, n, conf);
        const int32_t ratio_cap = xpnp::pnp_ratio_trials(ratio, conf);
        xpnp::Scan sc(row.data(), cap < ratio_cap ? cap : ratio_cap, mint);
        int used = 0, err = 0;
        bool stopped = false;
        for (int i = 0; i < R; ++i) {
            int t, cnt, lc;
            double sum, ls;
            if (std::scanf("%d %d %lf %d %lf", &t, &cnt, &sum, &lc, &ls) != 5) return 1;
            if (stopped) { err |= 16; continue; }
            if (t >= sc.max_trials) { err |= 4; continue; }
            ++used;
            const xpnp::Offer o = sc.offer(t, cnt, sum);
            if (o == xpnp::kNewBestLocal) {
                if (lc == -2) err |= 1;
                else if (lc >= 0) sc.offer_local(lc, ls);
            } else if (lc != -2) err |= 2;
            stopped = sc.after_model(t);
        }
        std::printf("%d %d %d %d %d %d\n", sc.best_trial, (int)sc.best_local, sc.num_trials, (int)sc.finish(), used, err);
    }
    return 0;
}
"""


@pytest.mark.parametrize("opt_name", sorted(Y.OPTION_SETS))
def test_scan_header_reproduces_the_yardstick(tmp_path, opt_name):
    """ba_pnp_scan.h fed the yardstick's per-model records: the same best trial, local flag, trial count and success, and it stops at
    the model the yardstick stops at (a record after the stop would be an error)."""
    exe = _build_host(tmp_path, "scan", _SCAN_DRIVER)
    opt, ext = Y.Options(**dict(Y.OPTION_SETS[opt_name])), Y.reference("longdouble", opt_name)
    lines, want = [], []
    for e in ext.values():
        if "scan" not in e:
            continue
        s = e["scan"]
        lines.append("%d %d %d %r %r %d" % (s["n"], opt.max_num_trials, opt.min_num_trials, opt.min_inlier_ratio, opt.confidence, len(e["records"])))
        lines += ["%d %d %r %d %r" % tuple(r) for r in e["records"]]
        want.append((s["best_trial"], s["local"], s["num_trials"], s["success"], len(e["records"]), 0))
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    got = [tuple(int(x) for x in ln.split()) for ln in out if ln]
    assert len(got) == len(want) >= 5
    assert got == want
    assert Y.num_trials_bound(25000, 100000, 0.9999) == 585 and Y.num_trials_bound(0, 16, 0.9999) == Y.UNBOUNDED and \
        Y.num_trials_bound(16, 16, 0.9999) == 1 and Y.num_trials_bound(8, 16, 1.0) == Y.UNBOUNDED


_FRAME_DRIVER = r"""
#include <cstdio>
#include <vector>
#include "ba_pnp_geom.h"
// ba_pnp_scan.h and ba_pnp_geom.h in a sequential driver of whole frames (every sum over the inliers in index order).
// per frame: "n cap min_trials confidence seed max_error", then n lines "x y X Y Z"; one line per frame:
// "status num_inliers num_trials best_trial P[12] mask"
using namespace xpnp;
static bool local_model(Epnp& w, const std::vector<unsigned char>& inl, const std::vector<double>& xy, const std::vector<double>& X, int n, double* P) {
    int first = -1;
    for (int k = 0; k < n && first < 0; ++k) if (inl[k]) first = k;
#define SUM(M, TERM) { double acc[M]; for (int e = 0; e < M; ++e) acc[e] = 0.0; \
        for (int k = 0; k < n; ++k) if (inl[k]) { const double* Xk = &X[3 * k]; const double x = xy[2 * k], y = xy[2 * k + 1]; (void)x; (void)y; TERM; } \
        for (int e = 0; e < M; ++e) w.red[e] = acc[e]; }
    SUM(4, (acc[0] += Xk[0], acc[1] += Xk[1], acc[2] += Xk[2], acc[3] += 1.0))
    epnp_stage_centroid(w);
    SUM(6, epnp_terms1(w, Xk, acc))
    if (!epnp_stage_control(w)) return false;
    SUM(40, epnp_terms2(w, Xk, x, y, acc))
    epnp_stage_solve(w, &X[3 * first]);
    SUM(9, epnp_terms3(w, Xk, acc))
    epnp_stage_means(w);
    SUM(27, epnp_terms4(w, Xk, acc))
    epnp_stage_rt(w);
    SUM(3, epnp_terms5(w, Xk, x, y, acc))
    return epnp_stage_pick(w, P);
#undef SUM
}
static void support(const double* P, const std::vector<double>& xy, const std::vector<double>& X, int n, double mr, int& c, double& s,
                    std::vector<unsigned char>* inl) {
    c = 0; s = 0.0;
    for (int k = 0; k < n; ++k) {
        const double r = residual(P, &X[3 * k], xy[2 * k], xy[2 * k + 1]);
        const bool in = r <= mr;
        if (in) { ++c; s += r; }
        if (inl) (*inl)[k] = in;
    }
}
int main() {
    int n, cap, mint; double conf, me; unsigned seed;
    while (std::scanf("%d %d %d %lf %u %lf", &n, &cap, &mint, &conf, &seed, &me) == 6) {
        std::vector<double> xy(2 * n), X(3 * n);
        for (int k = 0; k < n; ++k)
            if (std::scanf("%lf %lf %lf %lf %lf", &xy[2 * k], &xy[2 * k + 1], &X[3 * k], &X[3 * k + 1], &X[3 * k + 2]) != 5) return 1;
        std::vector<int32_t> row(n + 1), idx(n), tri(3 * (size_t)cap);
        for (int k = 0; k <= n; ++k) row[k] = pnp_dyn_trials(k, n, conf);
        pnp_sample_triples(seed, n, cap, idx.data(), tri.data());
        Scan sc(row.data(), cap, mint);
        const double mr = me * me;
        double best[12] = {0}, local[12], models[48];
        std::vector<unsigned char> inl(n);
        static Epnp w;
        for (int t = 0; t < cap && !sc.abort; ++t) {
            double sxy[6], sX[9];
            for (int k = 0; k < 3; ++k) {
                const int i = tri[3 * t + k];
                sxy[2 * k] = xy[2 * i]; sxy[2 * k + 1] = xy[2 * i + 1];
                for (int r = 0; r < 3; ++r) sX[3 * k + r] = X[3 * i + r];
            }
            const int nm = p3p_models(sxy, sX, models);
            for (int s = 0; s < nm; ++s) {
                int c; double sum;
                support(models + 12 * s, xy, X, n, mr, c, sum, nullptr);
                const Offer o = sc.offer(t, c, sum);
                if (o != kIgnored) {
                    for (int k = 0; k < 12; ++k) best[k] = models[12 * s + k];
                    if (o == kNewBestLocal) {
                        support(best, xy, X, n, mr, c, sum, &inl);
                        if (local_model(w, inl, xy, X, n, local)) {
                            int lc; double ls;
                            support(local, xy, X, n, mr, lc, ls, nullptr);
                            if (sc.offer_local(lc, ls)) for (int k = 0; k < 12; ++k) best[k] = local[k];
                        }
                    }
                }
                if (sc.after_model(t)) break;
            }
        }
        const bool ok = sc.finish() && all_finite(best, 12);
        int fc = 0; double fs;
        if (ok) support(best, xy, X, n, mr, fc, fs, &inl);
        std::printf("%d %d %d %d", ok ? 1 : 0, ok ? fc : 0, ok ? sc.num_trials : 0, ok ? sc.best_trial_code() : -1);
        for (int k = 0; k < 12; ++k) std::printf(" %.17g", ok ? best[k] : 0.0);
        std::printf(" m");
        for (int k = 0; k < n; ++k) std::printf("%d", ok ? (int)inl[k] : 0);
        std::printf("\n");
    }
    return 0;
}
"""


def test_geometry_headers_on_the_host_meet_every_bar(tmp_path):
    """The library's own arithmetic (P3P, root finder, rigid fit, the EPnP stages, the scan) without the kernel around it: on every
    non-fragile frame of the catalogue the discrete outputs equal the extended yardstick's and the pose meets both bars."""
    exe = _build_host(tmp_path, "frames", _FRAME_DRIVER)
    P, worst, checked = Y.pool(), 0.0, 0
    for name, items in Y.OPTION_SETS.items():
        opt, ext, fr = Y.Options(**dict(items)), Y.reference("longdouble", name), Y.fragile(name)
        ks = [k for k in ext if 3 <= len(P[k]["xy"]) <= Y.MAX_CORR]
        lines = []
        for k in ks:
            lines.append("%d %d %d %r %d %r" % (len(P[k]["xy"]), Y.trial_cap(opt), opt.min_num_trials, opt.confidence, opt.seed, opt.max_error))
            lines += ["%r %r %r %r %r" % (float(a[0]), float(a[1]), float(b[0]), float(b[1]), float(b[2])) for a, b in zip(P[k]["xy"], P[k]["X"])]
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.strip().split("\n")
        assert len(out) == len(ks)
        for k, ln in zip(ks, out):
            w = ln.split()
            got = dict(status=int(w[0]), num_inliers=int(w[1]), num_trials=int(w[2]), best_trial=int(w[3]), mask=np.array([int(c) for c in w[16][1:]], np.uint8))
            Pm = np.array([float(x) for x in w[4:16]]).reshape(3, 4)
            assert np.isfinite(Pm).all() and got["num_inliers"] == int(got["mask"].sum())
            if fr[k]:
                continue
            e = ext[k]
            assert Y.same_discrete(got, e), (name, k, P[k]["tag"])
            if e["status"] == 1:
                checked += 1
                assert np.allclose(Pm[:, :3], np.asarray(e["P"][:, :3], np.float64), rtol=1e-6, atol=1e-9)
                assert np.allclose(Pm[:, 3], np.asarray(e["t"], np.float64), rtol=1e-6, atol=1e-9)
                worst = max(worst, Y.deviation(Pm[:, :3], Pm[:, 3], e))
    print("sequential host driver: %d poses, largest deviation %.3e, tight bar %.3e" % (checked, worst, Y.TIGHT_BAR))
    assert checked >= 50 and worst <= Y.TIGHT_BAR
