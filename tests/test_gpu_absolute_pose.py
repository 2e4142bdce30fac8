"""xrsfm_ba_absolute_pose on the GPU against the extended-precision yardstick (tests/pose_yardstick.py), on every case of the
catalogue and every option set: exact discrete outputs on the non-fragile frames, self-consistency on every frame, the two pose bars,
the kernel's invariances, untouched outputs, and the hand-over to xrsfm_ba_refine_pose."""
import ctypes as C

import numpy as np
import pytest

from tests import pose_yardstick as Y

pytestmark = pytest.mark.gpu

_RESULTS = {}


def run_batch(opt_name, idx):
    """one library call per (option set, frames), shared by the tests"""
    from xrsfm_amd import capi
    key = (opt_name, tuple(idx))
    if key not in _RESULTS:
        ptr, xy, X = Y.arrays(idx)
        _RESULTS[key] = (capi.absolute_pose(ptr, xy, X, capi.absolute_pose_options(**dict(Y.OPTION_SETS[opt_name]))), ptr)
    return _RESULTS[key]


def frame_outputs(r, ptr, j):
    """everything the call returns for frame j, as bytes"""
    return (int(r["status"][j]), r["q"][j].tobytes(), r["t"][j].tobytes(), r["inlier_mask"][ptr[j]:ptr[j + 1]].tobytes(), int(r["num_inliers"][j]),
            int(r["num_trials"][j]), int(r["best_trial"][j]))


@pytest.mark.parametrize("opt_name", sorted(Y.OPTION_SETS))
def test_matches_the_yardstick(lib, opt_name):
    assert Y.fragile_share() <= Y.FRAGILE_CAP
    ext, fr, P = Y.reference("longdouble", opt_name), Y.fragile(opt_name), Y.pool()
    idx = Y.frames_of(opt_name)
    r, ptr = run_batch(opt_name, idx)
    opt = Y.Options(**dict(Y.OPTION_SETS[opt_name]))
    assert np.isfinite(r["q"]).all() and np.isfinite(r["t"]).all()
    worst = 0.0
    for j, k in enumerate(idx):
        e, sl = ext[k], slice(ptr[j], ptr[j + 1])
        got = dict(status=int(r["status"][j]), num_inliers=int(r["num_inliers"][j]), num_trials=int(r["num_trials"][j]),
                   best_trial=int(r["best_trial"][j]), mask=r["inlier_mask"][sl])
        where = (opt_name, j, k, P[k]["tag"])
        # self-consistency, on every frame
        assert got["num_inliers"] == int(got["mask"].sum()), where
        if got["status"] == 1:
            assert abs(float((r["q"][j] ** 2).sum()) - 1.0) <= 8 * 2.0 ** -53 and r["q"][j][3] >= 0, where
            assert Y.mask_check(r["q"][j], r["t"][j], P[k]["xy"], P[k]["X"], opt.max_error, got["mask"]), where
        else:
            assert got["status"] in (0, 2, 3) and not got["mask"].any() and (got["num_inliers"], got["num_trials"], got["best_trial"]) == (0, 0, -1), where
            assert not r["q"][j].any() and not r["t"][j].any(), where
        if fr[k]:
            continue
        # discrete outputs and the two pose bars
        assert Y.same_discrete(got, e), (where, {q: got[q] for q in Y.DISCRETE}, {q: e[q] for q in Y.DISCRETE})
        if e["status"] == 1:
            R = np.asarray(Y.quat_to_mat(r["q"][j]), np.float64)
            assert np.allclose(R, np.asarray(e["P"][:, :3], np.float64), rtol=1e-6, atol=1e-9), where
            assert np.allclose(r["t"][j], np.asarray(e["t"], np.float64), rtol=1e-6, atol=1e-9), where
            dev = Y.deviation(R, r["t"][j], e)
            worst = max(worst, dev)
            assert dev <= Y.TIGHT_BAR, (where, dev, Y.TIGHT_BAR)
    print(opt_name, "frames", len(idx), "library: largest deviation %.3e, restatement %.3e, tight bar %.3e" % (worst, Y.RESTATEMENT_DEVIATION, Y.TIGHT_BAR))


def test_outputs_do_not_depend_on_the_batch(lib):
    """a frame's outputs are bit-identical alone, among all frames, in a batch of 257 frames, in reversed order, and across two calls"""
    from xrsfm_amd import capi
    cases, seen = Y.cases(), {}
    for name in ("all", "b257"):
        r, ptr = run_batch("defaults", cases[name])
        for j, k in enumerate(cases[name]):
            out = frame_outputs(r, ptr, j)
            assert seen.setdefault(k, out) == out, (name, j, k)
    assert len(cases["b257"]) == 257
    for k in cases["one"] + [k for k, f in enumerate(Y.pool()) if f["tag"] in ("len3", "share0.8", "planar", "one_point_only", "two")]:
        r, ptr = run_batch("defaults", [k])
        assert frame_outputs(r, ptr, 0) == seen[k], k
    ptr, xy, X = Y.arrays(cases["b257"])
    again = capi.absolute_pose(ptr, xy, X)
    first = run_batch("defaults", cases["b257"])[0]
    assert all(np.array_equal(first[q].view(np.uint8), again[q].view(np.uint8)) for q in first)
    rev = cases["b257"][::-1]
    ptr, xy, X = Y.arrays(rev)
    r2 = capi.absolute_pose(ptr, xy, X)
    for j, k in enumerate(rev):
        assert frame_outputs(r2, ptr, j) == seen[k], (j, k)


def test_per_frame_max_error_and_seed(lib):
    """arrays equal to the scalar options change nothing; unequal entries give each frame its own single-call result"""
    from xrsfm_amd import capi
    idx = [k for k, f in enumerate(Y.pool()) if f["tag"] in ("len20", "len65", "share0.6", "random")][:8]
    ptr, xy, X = Y.arrays(idx)
    base = run_batch("defaults", idx)[0]
    o = capi.absolute_pose_options()
    same = capi.absolute_pose(ptr, xy, X, o, frame_max_error=np.full(len(idx), o.max_error), frame_seed=np.full(len(idx), o.seed, np.uint32))
    assert all(np.array_equal(base[q].view(np.uint8), same[q].view(np.uint8)) for q in base)
    fme = np.array([0.01, 0.02, 0.005, 0.01, 0.015, 0.02, 0.01, 0.0075])[:len(idx)]
    fseed = np.array([0, 1, 2, 0xFFFFFFFF, 5489, 0, 7, 8], np.uint32)[:len(idx)]
    mixed = capi.absolute_pose(ptr, xy, X, o, frame_max_error=fme, frame_seed=fseed)
    differs = 0
    for j, k in enumerate(idx):
        p1, xy1, X1 = Y.arrays([k])
        alone = capi.absolute_pose(p1, xy1, X1, capi.absolute_pose_options(max_error=float(fme[j]), seed=int(fseed[j])))
        assert frame_outputs(mixed, ptr, j) == frame_outputs(alone, p1, 0), (j, k)
        differs += frame_outputs(mixed, ptr, j) != frame_outputs(base, ptr, j)
    assert differs >= 4                                 # the per-frame values are really used


def test_untouched_poses_and_optional_outputs(lib):
    """q and t of frames without a pose keep the caller's values; the three count arrays may be NULL"""
    from xrsfm_amd import capi
    idx = Y.cases()["all"]
    ptr, xy, X = Y.arrays(idx)
    nf = len(idx)
    q = np.full((nf, 4), 1234.5); t = np.full((nf, 3), 1234.5); status = np.full(nf, 9, np.uint8); mask = np.full(len(xy), 9, np.uint8)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    o = capi.absolute_pose_options()
    assert lib.xrsfm_ba_absolute_pose(C.byref(o), nf, ptr.ctypes.data_as(C.POINTER(C.c_int32)), dp(xy), dp(X), None, None, dp(q), dp(t),
                                      status.ctypes.data_as(C.POINTER(C.c_uint8)), mask.ctypes.data_as(C.POINTER(C.c_uint8)), None, None, None) == 0
    r = run_batch("defaults", idx)[0]
    assert np.array_equal(status, r["status"]) and np.array_equal(mask, r["inlier_mask"])
    assert set(status.tolist()) == {0, 1, 2, 3}
    found = status == 1
    assert np.array_equal(q[found], r["q"][found]) and np.array_equal(t[found], r["t"][found])
    assert np.all(q[~found] == 1234.5) and np.all(t[~found] == 1234.5)


def test_absolute_pose_then_refine_pose_recovers_the_generating_pose(lib):
    """end to end: SolvePnP_colmap's flattening, the RANSAC pose, xrsfm_ba_refine_pose on the returned inliers (pnp.cc:29-71); the
    refined pose ends within the refinement tests' tolerance (1e-5) of the pose that generated the noise-free inliers"""
    from xrsfm_amd import capi
    rng = np.random.default_rng(11)
    f, cx, cy, n = 400.0, 320.0, 240.0, 150
    fr = Y._frame(rng, n, 0.25, "e2e", noise=0.0)
    uv = fr["xy"] * f + [cx, cy]                                        # SIMPLE_RADIAL (model 2) without distortion
    r = capi.absolute_pose([0, n], (uv - [cx, cy]) / f, fr["X"], capi.absolute_pose_options(max_error=8.0 / f))
    assert r["status"][0] == 1 and r["num_inliers"][0] >= int(0.75 * n) - 2
    q, t, s = capi.refine_pose(2, [f, cx, cy, 0.0], fr["X"], uv, r["q"][0], r["t"][0], inlier_mask=r["inlier_mask"])
    q_true = np.asarray(Y.quat_of(np.concatenate([fr["R"], fr["t"][:, None]], 1)), np.float64)
    assert min(np.abs(q - q_true).max(), np.abs(q + q_true).max()) < 1e-5 and np.abs(t - fr["t"]).max() < 1e-5
