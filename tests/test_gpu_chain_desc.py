"""The flattened index chains of the reduced-camera chain (ba_plan.h: ChainDesc, the default) against the lists they were built
from (XRSFM_BA_CHAIN_DESC=0), bit for bit: the records only change where an address comes from, not one value, product or sum.

Per problem, once with the switch off and once with the default, compared as uint64 views: xrsfm_ba_debug_cholesky_solve
(solution and the dense S the tile fill materialises: k_tile_fill_rec against k_tile_fill) and an 8-iteration run (cameras,
points, final cost: k_lv_factor<true, true> and k_lv_factor<false, true> against the list walkers).  The default runs twice in a
row in one context and must repeat itself, which covers the epoch / ticket state of k_lv_bwd_all.
Every case asserts the facts of its plan (xrsfm_ba_debug_chol_plan), so that it cannot silently test another path:
  c100      level schedule, 4 levels of which 2 split, one-launch backward substitution, 25 tiles composed by trailing workgroups
  c320      5 levels, 3 split, 73 trailing tiles
  c8        one tile column: the first level is the last, backward solve inside the factor launch
  c40       panel schedule (push-form backward substitution): same kernels, lists of one column per level
  ragged    test_gpu_hardening.py's ragged band (missed detections, 8 observations per track): 7 levels, 5 split
  closures  its band with hub cameras (loop closures): 8 levels, 6 split
  bal9      its bal9 problem: 9 unknowns per camera, 7 cameras per tile (k9_tile_fill composes the tiles; the factor records apply)
  packed    c100 with XRSFM_BA_PACKED=1: the records name the packed tiles themselves (no tile-map read)"""
import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu

RADIUS = 2e3
SUMMARY_KEYS = ("initial_cost", "final_cost", "n_successful", "n_unsuccessful", "termination", "lm_steps_attempted", "linear_solver_used")


def _synth(**kw):
    from xrsfm_amd import capi, synth
    d = synth.make_problem(**kw)
    return {k: d[k] for k in capi.ProblemArrays.FIELDS}


def _bal9():
    from xrsfm_amd import capi, synth
    d = synth.to_bal9(synth.make_problem(n_cams=200, n_points=12000, k_obs=4, seed=913))
    return {k: d[k] for k in capi.ProblemArrays.FIELDS}


# name -> (problem, environment of the case, facts of its plan)
CASES = {
    "c100": (lambda: _synth(n_cams=100, n_points=5000, k_obs=4, seed=1), {},
             dict(schedule="level", levels=4, split_levels=2, bwd="all", fill_rest=25, packed=False, cw=6)),
    "c320": (lambda: _synth(n_cams=320, n_points=16000, k_obs=4, seed=1), {},
             dict(schedule="level", levels=5, split_levels=3, bwd="all", fill_rest=73, packed=False, cw=6)),
    "c8": (lambda: _synth(n_cams=8, n_points=400, k_obs=4, seed=1), {},
           dict(T=1, levels=1, bwd="fused", fill_rest=0, cw=6)),
    "c40": (lambda: _synth(n_cams=40, n_points=2000, k_obs=4, seed=1), {},
            dict(schedule="panel", T=4, levels=4, bwd="push", cw=6)),
    "ragged": (lambda: H.make(300, 20000, 8, seed=911, dropout=0.35), {},
               dict(schedule="level", levels=7, split_levels=5, bwd="all", fill_rest=99, cw=6)),
    "closures": (lambda: _synth(n_cams=500, n_points=30000, k_obs=4, seed=912, n_hubs=24, hub_tracks=10), {},
                 dict(schedule="level", levels=8, split_levels=6, bwd="all", fill_rest=91, cw=6)),
    "bal9": (_bal9, {}, dict(schedule="level", levels=5, split_levels=3, bwd="all", cw=9, T=45)),
    "packed": (lambda: _synth(n_cams=100, n_points=5000, k_obs=4, seed=1), {"XRSFM_BA_PACKED": "1"},
               dict(schedule="level", levels=4, split_levels=2, bwd="all", fill_rest=25, packed=True, cw=6)),
}


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _snapshot(arr, wide, runs):
    """A fresh context under the current environment: one debug solve, then `runs` 8-iteration runs (a reset before each)."""
    from xrsfm_amd import capi
    out = {}
    ctx = capi.Context(H.to_product(arr))
    try:
        if wide:
            out["y"] = ctx.debug_wide(5.99, RADIUS)["y"]
        else:
            ctx.debug_linearize(5.99, False)
            out["y"], out["S"] = ctx.debug_cholesky_solve(RADIUS, want_S=True)
            assert np.abs(out["S"]).max() > 0
        assert np.isfinite(out["y"]).all() and np.abs(out["y"]).max() > 0       # the comparison is not of zeros
        for r in range(runs):
            ctx.reset()
            s = ctx.run(capi.default_options(max_iterations=8, linear_solver=capi.SOLVER_CHOLESKY))
            q, t, P = ctx.download()
            out[f"run{r}"] = {k: getattr(s, k) for k in SUMMARY_KEYS}
            out[f"q{r}"], out[f"t{r}"], out[f"P{r}"] = q.copy(), t.copy(), P.copy()
    finally:
        ctx.close()
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_records_equal_lists(lib, monkeypatch, name):
    from xrsfm_amd import capi
    make, env, want = CASES[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    arr = make()
    facts = capi.debug_chol_plan(H.to_product(arr))["facts"]
    assert {k: facts[k] for k in want} == want, (name, facts)
    wide = facts["cw"] == 9
    monkeypatch.setenv("XRSFM_BA_CHAIN_DESC", "0")
    ref = _snapshot(arr, wide, 1)
    monkeypatch.delenv("XRSFM_BA_CHAIN_DESC")
    got = _snapshot(arr, wide, 2)
    assert ref["run0"]["n_successful"] > 0 and ref["run0"]["linear_solver_used"] == capi.SOLVER_CHOLESKY, ref["run0"]
    for k in ("y",) if wide else ("y", "S"):
        assert np.array_equal(_bits(ref[k]), _bits(got[k])), (name, k, int((ref[k] != got[k]).sum()), float(np.abs(ref[k] - got[k]).max()))
    for r in range(2):          # the lists against both runs of the default, i.e. the second run repeats the first
        assert ref["run0"] == got[f"run{r}"], (name, r, ref["run0"], got[f"run{r}"])
        for k in ("q", "t", "P"):
            assert np.array_equal(_bits(ref[f"{k}0"]), _bits(got[f"{k}{r}"])), (name, r, k)
