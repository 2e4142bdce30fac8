"""XRSFM_BA_SOLVER_RESIDENT (xrsfm_amd/csrc/ba_lba.h): the whole LM loop in one launch of one workgroup, for problems whose
reduced camera system is one tile.

Tolerances are the project's own (BASELINE.json north_star, tests/test_gpu_parity.py::test_full_solve_parity): equal step
counts, reference-style RMSE within 1e-6 px, camera parameters within 1e-5 — against the oracle and against the engine
(XRSFM_BA_SOLVER_CHOLESKY); between covariances the 1e-8 relative of tests/test_gpu_covariance.py (kernel path vs fallback).
Differences actually observed: profiles/lba_resident.md.

Seeds named by the corner tests were picked with oracle/ba_oracle.py on the CPU:
  unsuccessful step: H.make(7, 150, 4, seed=13) with the quaternions displaced by 0.04 * N(0,1) (rng 5) and renormalised,
                     max_iterations 6: the oracle accepts 5 steps and rejects 1;
  tolerance exit:    H.make(7, 150, 4, seed=12), function_tolerance 1e-2, max_iterations 50: the oracle stops on a tolerance.
Both are asserted on the oracle's summary inside the tests.
"""
import math
import os

import numpy as np
import pytest

from oracle import ba_oracle as bo
from tests import helpers as H

pytestmark = pytest.mark.gpu

LBA_OPT = dict(max_iterations=5, function_tolerance=1e-4, parameter_tolerance=1e-5)


def _variant(name):
    arr = H.make(10, 400, 4, seed=103)            # 10 cameras = 60 of the tile's 64 rows
    kw = {}
    if name == "models":
        arr = H.with_models(arr, seed=4)
    if name == "structure_only":
        arr["cam_const"][:] = 3
    if name == "lba":
        kw = dict(LBA_OPT)
        seen = np.zeros(arr["points"].shape[0], bool); seen[arr["obs_pt"][arr["obs_cam"] == 9]] = True
        arr["point_const"][:] = (~seen).astype(np.uint8)
    if name == "golden":
        z = np.load(os.path.join(os.path.dirname(__file__), "golden", "lba.npz"))
        arr = {k[3:]: np.array(z[k], copy=True) for k in z.files if k.startswith("in_")}
        mi, ft, pt, rad = z["opt"]
        kw = dict(max_iterations=int(mi), function_tolerance=float(ft), parameter_tolerance=float(pt), initial_radius=float(rad))
    return arr, kw


_CACHE = {}


def _solved(name):
    """(arr, kw, oracle problem after its solve, oracle summary, engine (q, t, P, summary), resident (q, t, P, summary)): once."""
    if name not in _CACHE:
        from xrsfm_amd import capi
        arr, kw = _variant(name)
        pr = H.to_oracle(arr)
        s_ref = bo.solve(pr, bo.Options(**kw))
        out = {}
        for solver in (capi.SOLVER_CHOLESKY, capi.SOLVER_RESIDENT):
            ctx = capi.Context(H.to_product(arr))
            s = ctx.run(capi.default_options(linear_solver=solver, **kw))
            out[solver] = ctx.download() + (s,)
            ctx.close()
        _CACHE[name] = (arr, kw, pr, s_ref, out[capi.SOLVER_CHOLESKY], out[capi.SOLVER_RESIDENT])
    return _CACHE[name]


def _rmse(cost, arr):
    return math.sqrt(cost / (2 * arr["obs_cam"].shape[0]))


VARIANTS = ["lba", "kitti", "models", "structure_only", "golden"]


@pytest.mark.parametrize("name", VARIANTS)
def test_oracle_parity(lib, name):
    from xrsfm_amd import capi
    arr, kw, pr, s_ref, _, (q, t, P, s) = _solved(name)
    print(f"{name}: steps {s.n_successful}+{s.n_unsuccessful} (oracle {s_ref.n_successful}+{s_ref.n_unsuccessful}) "
          f"|d rmse| {abs(_rmse(s.final_cost, arr) - _rmse(s_ref.final_cost, arr)):.3e} "
          f"|d cam| {max(np.abs(q - pr.cam_q).max(), np.abs(t - pr.cam_t).max()):.3e}")
    assert s.linear_solver_used == capi.SOLVER_RESIDENT == 3
    assert s.n_successful == s_ref.n_successful and s.n_unsuccessful == s_ref.n_unsuccessful
    assert abs(_rmse(s.final_cost, arr) - _rmse(s_ref.final_cost, arr)) < 1e-6
    assert np.abs(q - pr.cam_q).max() < 1e-5 and np.abs(t - pr.cam_t).max() < 1e-5
    assert s.num_residuals == s_ref.num_residuals and s.num_effective_params == s_ref.num_effective_params


def _same_as_engine(arr, se, sr, eng, res):
    assert (sr.n_successful, sr.n_unsuccessful, sr.termination, sr.termination_reason, sr.lm_steps_attempted) == \
           (se.n_successful, se.n_unsuccessful, se.termination, se.termination_reason, se.lm_steps_attempted)
    d_rmse = abs(_rmse(sr.final_cost, arr) - _rmse(se.final_cost, arr))
    d_init = abs(_rmse(sr.initial_cost, arr) - _rmse(se.initial_cost, arr))
    d_cam = max(np.abs(res[0] - eng[0]).max(), np.abs(res[1] - eng[1]).max())
    d_pt = np.abs(res[2] - eng[2]).max()
    print(f"vs engine: |d rmse| {d_rmse:.3e} |d rmse0| {d_init:.3e} |d cam| {d_cam:.3e} |d points| {d_pt:.3e}")
    assert d_rmse < 1e-6 and d_init < 1e-6 and d_cam < 1e-5 and d_pt < 1e-5


@pytest.mark.parametrize("name", VARIANTS)
def test_against_engine(lib, name):
    arr, kw, _, _, eng, res = _solved(name)
    _same_as_engine(arr, eng[3], res[3], eng, res)


def _both(arr, **kw):
    from xrsfm_amd import capi
    out = []
    for solver in (capi.SOLVER_CHOLESKY, capi.SOLVER_RESIDENT):
        ctx = capi.Context(H.to_product(arr))
        s = ctx.run(capi.default_options(linear_solver=solver, **kw))
        out.append(ctx.download() + (s,))
        ctx.close()
    return out


def _corner(name):
    kw = dict(LBA_OPT)
    if name in ("cams1", "cams2", "cams7"):
        n = int(name[4:])
        arr = H.make(n, 97, min(n, 4), seed=120 + n)          # 97 tracks: an observation count that is no multiple of 64 / 512
        if n == 1:
            arr["point_const"][:] = 0
    elif name == "ragged":       # tracks of one observation next to tracks of 10
        rng = np.random.default_rng(3)
        tracks = [list(range(10)) if i % 2 == 0 else [int(rng.integers(10))] for i in range(61)]
        arr = H.make_tracks(10, tracks, seed=7)
    elif name == "behind":
        arr = H.make(8, 300, 4, seed=101)
        arr["points"][::7] += np.array([0.0, 0.0, -60.0])
    elif name == "consts":
        arr = H.make(8, 300, 4, seed=101)
        arr["cam_const"][:] = 0; arr["cam_const"][2] = 3; arr["cam_const"][5] = 1; arr["cam_const"][6] = 2
        arr["point_const"][::3] = 1
    elif name == "point_const_most":
        arr = H.make(7, 200, 4, seed=130)
        arr["point_const"][:] = 1; arr["point_const"][::9] = 0
    elif name == "unsuccessful":
        arr = H.make(7, 150, 4, seed=13)
        arr["cam_q"] = arr["cam_q"] + 0.04 * np.random.default_rng(5).standard_normal(arr["cam_q"].shape)
        arr["cam_q"] /= np.linalg.norm(arr["cam_q"], axis=1, keepdims=True)
        kw = dict(max_iterations=6)
    elif name == "tolerance_exit":
        arr = H.make(7, 150, 4, seed=12)
        kw = dict(max_iterations=50, function_tolerance=1e-2)
    elif name == "max_iterations_0":
        arr = H.make(7, 150, 4, seed=13)
        kw = dict(max_iterations=0)
    return arr, kw


CORNERS = ["cams1", "cams2", "cams7", "ragged", "behind", "consts", "point_const_most", "unsuccessful", "tolerance_exit", "max_iterations_0"]


@pytest.mark.parametrize("name", CORNERS)
def test_kernel_corners(lib, name):
    arr, kw = _corner(name)
    pr = H.to_oracle(arr)
    s_ref = bo.solve(pr, bo.Options(**kw))
    if name == "unsuccessful":
        assert s_ref.n_unsuccessful >= 1
    if name == "tolerance_exit":
        assert s_ref.n_successful + s_ref.n_unsuccessful < kw["max_iterations"]
    eng, res = _both(arr, **kw)
    s = res[3]
    print(f"{name}: steps {s.n_successful}+{s.n_unsuccessful} (oracle {s_ref.n_successful}+{s_ref.n_unsuccessful}), termination {s.termination}/{s.termination_reason}")
    assert s.linear_solver_used == 3
    assert (s.n_successful, s.n_unsuccessful) == (s_ref.n_successful, s_ref.n_unsuccessful)
    assert abs(_rmse(s.final_cost, arr) - _rmse(s_ref.final_cost, arr)) < 1e-6
    assert np.abs(res[0] - pr.cam_q).max() < 1e-5 and np.abs(res[1] - pr.cam_t).max() < 1e-5
    _same_as_engine(arr, eng[3], s, eng, res)
    if name == "max_iterations_0":
        assert s.n_successful == 0 and s.lm_steps_attempted == 0 and s.termination_reason == 5
        assert np.array_equal(res[0], arr["cam_q"]) and np.array_equal(res[2], arr["points"])


def _summary_tuple(s):
    return (s.initial_cost, s.final_cost, s.n_successful, s.n_unsuccessful, s.termination, s.termination_reason, s.lm_steps_attempted)


def test_state_reset_is_bit_reproducible(lib):
    from xrsfm_amd import capi
    arr, kw = _variant("lba")
    opt = capi.default_options(linear_solver=capi.SOLVER_RESIDENT, **kw)
    ctx = capi.Context(H.to_product(arr))
    s1 = ctx.run(opt); d1 = ctx.download()
    ctx.reset()
    s2 = ctx.run(opt); d2 = ctx.download()
    ctx.close()
    assert _summary_tuple(s1) == _summary_tuple(s2)
    assert all(np.array_equal(a, b) for a, b in zip(d1, d2))


def test_state_continues_like_the_engine(lib):
    from xrsfm_amd import capi
    arr = H.make(9, 300, 4, seed=140)
    first = dict(max_iterations=2)
    runs = {}
    for solver in (capi.SOLVER_CHOLESKY, capi.SOLVER_RESIDENT):
        ctx = capi.Context(H.to_product(arr))
        sa = ctx.run(capi.default_options(linear_solver=solver, **first))
        sb = ctx.run(capi.default_options(linear_solver=capi.SOLVER_CHOLESKY, max_iterations=20))
        runs[solver] = (sa, sb, ctx.download())
        ctx.close()
    (ea, eb, ed), (ra, rb, rd) = runs[capi.SOLVER_CHOLESKY], runs[capi.SOLVER_RESIDENT]
    assert (ra.n_successful, ra.n_unsuccessful) == (ea.n_successful, ea.n_unsuccessful)
    assert (rb.n_successful, rb.n_unsuccessful, rb.termination_reason) == (eb.n_successful, eb.n_unsuccessful, eb.termination_reason)
    assert abs(_rmse(rb.final_cost, arr) - _rmse(eb.final_cost, arr)) < 1e-6
    assert max(np.abs(rd[0] - ed[0]).max(), np.abs(rd[1] - ed[1]).max()) < 1e-5


def test_state_covariance_after_resident_run(lib):
    from xrsfm_amd import capi
    from tests import cov_yardstick as Y
    arr, kw = _variant("kitti")
    arr = Y.fix_gauge(arr)               # (the undamped reduced system is singular with a free gauge: xrsfm_ba_covariance needs one)
    covs = []
    for solver in (capi.SOLVER_CHOLESKY, capi.SOLVER_RESIDENT):
        ctx = capi.Context(H.to_product(arr))
        ctx.run(capi.default_options(linear_solver=solver, **kw))
        covs.append(ctx.covariance([1, 4, 9]))
        ctx.close()
    rel = np.abs(covs[1] - covs[0]).max(axis=(1, 2)) / np.abs(covs[0]).max(axis=(1, 2))
    print(f"covariance after resident vs engine run: max rel {rel.max():.3e}")
    assert (rel <= 1e-8).all(), float(rel.max())


def _refused(ctx, arr):
    from xrsfm_amd import capi
    with pytest.raises(RuntimeError, match="EINVAL"):
        ctx.run(capi.default_options(linear_solver=capi.SOLVER_RESIDENT, **LBA_OPT))
    q, t, P = ctx.download()
    assert np.array_equal(q, arr["cam_q"]) and np.array_equal(t, arr["cam_t"]) and np.array_equal(P, arr["points"])


@pytest.mark.parametrize("case", ["cams11", "bal9", "hook", "duplicate"])
def test_refusals(lib, case):
    from xrsfm_amd import capi
    if case == "cams11":
        arr = H.make(11, 200, 4, seed=150)
    elif case == "bal9":
        arr = H.make_bal9(8, 200, 4, seed=5)
    else:
        arr = H.make(7, 150, 4, seed=151)
    if case == "duplicate":          # the first track is observed twice by its first camera
        i = int(np.flatnonzero(arr["obs_pt"] == arr["obs_pt"][0])[0])
        for k in ("obs_cam", "obs_pt"):
            arr[k] = np.concatenate([arr[k], arr[k][i:i + 1]])
        arr["obs_uv"] = np.concatenate([arr["obs_uv"], arr["obs_uv"][i:i + 1] + 0.5])
    ctx = capi.Context(H.to_product(arr))
    if case == "hook":
        ctx.comm_hook(1, 0, lambda a, op: None)
    _refused(ctx, arr)
    ctx.close()


def test_auto_never_picks_resident(lib):
    from xrsfm_amd import capi
    arr, kw = _variant("lba")
    s = capi.solve(H.to_product(arr), capi.default_options(linear_solver=capi.SOLVER_AUTO, **kw))
    assert s.linear_solver_used == capi.SOLVER_CHOLESKY


def test_one_shot_solve_accepts_resident(lib):
    from xrsfm_amd import capi
    arr, kw, _, _, _, res = _solved("lba")
    prod = H.to_product(arr)
    s = capi.solve(prod, capi.default_options(linear_solver=capi.SOLVER_RESIDENT, **kw))
    assert s.linear_solver_used == 3 and _summary_tuple(s) == _summary_tuple(res[3])
    assert np.array_equal(prod.cam_q, res[0]) and np.array_equal(prod.points, res[2])


def test_profile_lists_one_launch(lib):
    from xrsfm_amd import capi
    arr, kw = _variant("lba")
    ctx = capi.Context(H.to_product(arr))
    ctx.run(capi.default_options(linear_solver=capi.SOLVER_RESIDENT, profile=1, **kw))
    launched = {k: v for k, v in ctx.profile().items() if v[1] > 0}
    ctx.close()
    assert list(launched) == ["k_lba_resident"] and launched["k_lba_resident"][1] == 1


def test_adapter_lba_with_the_environment_switch(lib, tmp_path, monkeypatch):
    """BASolver::LBA through tests/shim in a fresh child process, once with XRSFM_BA_LBA_RESIDENT=1 and once without: the first
    runs the resident solver (the call trace says solver 3), the second today's call, and the maps agree within the bounds of
    test_against_engine."""
    from tests import test_adapter as TA
    import subprocess
    subprocess.run(["make", "-C", TA.SHIM], check=True, capture_output=True)
    i, z, arr, fr, i1, i2 = list(TA._lba_cases())[0]
    arr = H.with_models(arr, seed=2)
    monkeypatch.setenv("XRSFM_BA_TRACE_CALLS", "1")
    (tmp_path / "a").mkdir(); (tmp_path / "b").mkdir()
    st0, q0, t0, P0, _, err0 = TA._run(TA.EXE, arr, tmp_path / "a", "lba", fr, i1, i2)
    monkeypatch.setenv("XRSFM_BA_LBA_RESIDENT", "1")
    st1, q1, t1, P1, _, err1 = TA._run(TA.EXE, arr, tmp_path / "b", "lba", fr, i1, i2)
    assert st0 == 0 and st1 == 0, (err0, err1)
    assert " solver 1 " in err0 and " solver 3 " in err1, (err0, err1)
    d_cam = max(np.abs(q1 - q0).max(), np.abs(t1 - t0).max())
    print(f"adapter LBA, resident vs default: |d cam| {d_cam:.3e} |d points| {np.abs(P1 - P0).max():.3e}")
    assert d_cam < 1e-5 and np.abs(P1 - P0).max() < 1e-5
