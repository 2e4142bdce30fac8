"""J-free linearisation (the Cholesky path's default): k_linearize stores no residual / Jacobian per observation, k_schur_pairs
and k_backsub recompute them from the state and uv with the same arithmetic.  XRSFM_BA_JFREE=0 keeps them stored: both ways the
linearisation diagnostics, the reduced camera matrix, its solve and a full run must be BIT-identical."""
import os

import numpy as np
import pytest

from tests import helpers as H


def _case(name):
    if name == "models":
        return H.with_models(H.make(40, 2000, 4, seed=211), seed=3)
    if name == "behind":         # clamp branch: residual (12, 12), J = 0
        arr = H.make(40, 2000, 4, seed=212)
        arr["points"][::7] += np.array([0.0, 0.0, -60.0])
        return arr
    if name == "outliers":       # Huber weights < 1 on a fifth of the observations
        return H.make(40, 2000, 4, seed=213, outlier_frac=0.2)
    if name == "consts":
        arr = H.make(40, 2000, 4, seed=214)
        arr["cam_const"][:] = 0; arr["cam_const"][2] = 3; arr["cam_const"][5] = 1; arr["cam_const"][9] = 2
        arr["point_const"][::3] = 1
        return arr
    if name == "long":           # tracks of 70 observations: long items (several tiles per track)
        return H.make(80, 40, 70, seed=215, min_tri_angle_deg=0.5, mode="unordered")
    if name == "wide":           # regular tiles of 14-camera tracks (not Gram tiles: more than 10 cameras)
        return H.make(32, 300, 14, seed=219)
    if name == "ragged":         # ragged Gram tiles next to non-Gram tiles
        return H.make(300, 20000, 8, seed=216, dropout=0.35)
    raise ValueError(name)


def _solve_all(arr):
    from xrsfm_amd import capi
    ctx = capi.Context(H.to_product(arr))
    try:
        lin = ctx.debug_linearize(5.99, True)
        stored_lin = ctx.debug_stored_j()
        y, S = ctx.debug_cholesky_solve(2e3, want_S=True)
        ctx.reset()
        s = ctx.run(capi.default_options(max_iterations=8, linear_solver=capi.SOLVER_CHOLESKY))
        q, t, P = ctx.download()
    finally:
        ctx.close()
    assert stored_lin == (os.environ.get("XRSFM_BA_JFREE") == "0")      # the A/B compares the two paths, not one path twice
    return lin, y, S, (s.n_successful, s.n_unsuccessful, s.initial_cost, s.final_cost), q, t, P


def _both(monkeypatch, fn):
    out = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("XRSFM_BA_JFREE", flag)
        out[flag] = fn()
    monkeypatch.delenv("XRSFM_BA_JFREE")
    return out["1"], out["0"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["models", "behind", "outliers", "consts", "long", "wide", "ragged"])
def test_jfree_equals_stored_j(lib, monkeypatch, case):
    arr = _case(case)
    a, b = _both(monkeypatch, lambda: _solve_all(arr))
    for k in a[0]:
        assert np.array_equal(a[0][k], b[0][k]), k
    assert np.abs(b[2]).max() > 0 and np.all(np.isfinite(b[1]))
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert a[3] == b[3] and b[3][0] > 0
    for x, y in zip(a[4:], b[4:]):
        assert np.array_equal(x, y)
    if case == "behind":
        assert (np.abs(b[0]["r"]).max(axis=1) > 1.0).sum() > 10


@pytest.mark.gpu
def test_jfree_two_hook_ranks(lib, monkeypatch):
    from xrsfm_amd import capi
    from tests.test_multirank_gpu import _run_ranks
    arr = H.make(60, 4000, 4, seed=217)
    a, b = _both(monkeypatch, lambda: _run_ranks(2, arr, capi.SOLVER_CHOLESKY, dict(max_iterations=8)))
    for ra, rb in zip(a, b):
        for k in ("q", "t", "P", "stat", "cost"):
            assert np.array_equal(ra[k], rb[k]), k


@pytest.mark.gpu
def test_jfree_context_alternates_cholesky_and_pcg(lib, monkeypatch):
    """One context serves both solvers: the J buffers come with the first PCG run, a later Cholesky run goes J-free again; a
    PCG product after a J-free linearisation reads J materialised from it."""
    from xrsfm_amd import capi
    arr = H.make(40, 2000, 4, seed=218)
    x = np.random.default_rng(0).normal(size=(40, 6))

    def seq():
        ctx = capi.Context(H.to_product(arr))
        res = []
        try:
            ctx.debug_linearize(5.99, True)
            res += list(ctx.debug_schur_product(1e3, x))
            res += list(ctx.debug_cholesky_solve(1e3))[:1]
            for solver in (capi.SOLVER_CHOLESKY, capi.SOLVER_PCG, capi.SOLVER_CHOLESKY):
                ctx.reset()
                s = ctx.run(capi.default_options(max_iterations=6, linear_solver=solver))
                res.append(np.array([s.n_successful, s.n_unsuccessful, s.final_cost]))
                res += list(ctx.download())
        finally:
            ctx.close()
        return res

    a, b = _both(monkeypatch, seq)
    assert len(a) == len(b)
    for x1, x2 in zip(a, b):
        assert np.array_equal(x1, x2)


@pytest.mark.gpu
def test_jfree_mode_of_a_run(lib, monkeypatch):
    """Which path a Cholesky run takes: J-free on a map of Gram tiles while its steps are accepted; stored J when the plan has
    long-track items, after the first rejected step, below the size floor (1 M slots) unless XRSFM_BA_JFREE=1 drops it, and
    with XRSFM_BA_JFREE=0."""
    from xrsfm_amd import capi

    def mode(arr, iters):
        ctx = capi.Context(H.to_product(arr))
        try:
            s = ctx.run(capi.default_options(max_iterations=iters, linear_solver=capi.SOLVER_CHOLESKY))
            return ctx.debug_stored_j(), s.n_unsuccessful
        finally:
            ctx.close()

    arr = _case("models")
    assert mode(arr, 2)[0]                        # (8 000 observations: below the size floor)
    monkeypatch.setenv("XRSFM_BA_JFREE", "1")
    stored, rejected = mode(arr, 2)
    assert rejected > 0 or not stored
    stored, rejected = mode(arr, 30)
    assert stored == (rejected > 0)
    assert mode(_case("long"), 2)[0]
    monkeypatch.setenv("XRSFM_BA_JFREE", "0")
    assert mode(arr, 2)[0]
