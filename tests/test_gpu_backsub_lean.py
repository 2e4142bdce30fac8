"""The 5-wave back-substitution kernels (k_backsub<PREP, YP> + k_backsub_long<PREP>, the default) against k_backsub_parent
(XRSFM_BA_BACKSUB_LEAN=0), bit for bit: the restructuring moves loads and splits the launch, the expression trees are the parent's.

Compared per problem, with XRSFM_BA_JFREE=1 (recomputed F, E) and =0 (stored J): the outputs of one debug_backsub after a
debug_linearize + debug_cholesky_solve (candidate points and cameras, point_step, per-item model-decrease and step-norm partials),
then the summary and the final state of an 8-iteration run.  The problems are the smallest that reach every branch of the kernels:
  regular   full regular tiles of tracks of length 2, 3 and 4 (same camera tuple through a tile), next to mixed tiles
  ragged    missed detections: tiles with empty lanes and 5-8 cameras
  long      one track of 70 and one of 135 observations (items of 2 and 3 tiles: k_backsub_long) — 140 cameras, because a track
            of more than 128 observations needs as many cameras; every other problem has at most 40
  consts    constant points, constant rotations, constant translations, both, and a camera without observations
  robust    observations on the Huber branch (gross outliers) and on the depth clamp (points behind their cameras)
  models    every camera model of tests/helpers.py::with_models
  pcg       the PCG solver with stored point inverses (k_backsub<false>, stored J)
  rerun     a context that is run, reset and run again (the kernels' LDS between launches)
A plain run no longer stores point_step; the only entry that reads it (debug_backsub) launches the kernel again with the store on,
so "a run leaves point_step untouched" has no read path and is not tested here; the write bytes are in profiles/r09_backsub_waves.md."""
import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu

HUBER_A = 5.99
RADIUS = 1e4
DEBUG_KEYS = ("part_model", "part_step2", "cand_points", "point_step", "cand_cam_q", "cand_cam_t")
SUMMARY_KEYS = ("initial_cost", "final_cost", "n_successful", "n_unsuccessful", "termination", "lm_steps_attempted", "linear_solver_used")


def _regular():
    rng = np.random.default_rng(3)
    tracks = [np.array([0, 1])] * 64 + [np.array([2, 3, 4])] * 64 + [np.array([5, 6, 7, 8])] * 48
    tracks += [np.sort(rng.choice(12, int(n), replace=False)) for n in rng.integers(2, 5, 150)]
    return H.make_tracks(12, tracks, seed=21)


def _ragged():
    return H.make(40, 2000, 8, seed=33, dropout=0.35)


def _long():
    rng = np.random.default_rng(5)
    tracks = [np.sort(np.unique(np.arange(c, c + 4) % 140)) for c in rng.integers(0, 140, 300)]
    tracks += [np.sort(rng.choice(140, 70, replace=False)), np.sort(rng.choice(140, 135, replace=False))]
    return H.make_tracks(140, tracks, seed=5)


def _consts():
    arr = H.make(12, 500, 4, seed=41)
    arr["point_const"] = (np.arange(500) % 5 == 0).astype(np.uint8)
    cc = np.zeros(12, np.uint8); cc[2] = 3; cc[5] = 1; cc[7] = 2
    arr["cam_const"] = cc
    keep = arr["obs_cam"] != 9                       # camera 9 keeps its place and loses its observations
    for k in ("obs_cam", "obs_pt", "obs_uv"):
        arr[k] = np.ascontiguousarray(arr[k][keep])
    return arr


def _robust():
    arr = H.make(12, 500, 4, seed=43, outlier_frac=0.1)
    arr["points"] = np.array(arr["points"], copy=True)
    arr["points"][3::29] += np.array([0.0, 0.0, -60.0])          # behind their cameras: the clamp branch
    return arr


def _models():
    return H.with_models(H.make(15, 500, 4, seed=47), seed=3)


PROBLEMS = {"regular": _regular, "ragged": _ragged, "long": _long, "consts": _consts, "robust": _robust, "models": _models}
_ARR = {}


def _problem(name):
    if name not in _ARR:
        _ARR[name] = PROBLEMS[name]()
    return _ARR[name]


def _snapshot(arr, solver=None, runs=1):
    """One debug back-substitution and `runs` 8-iteration runs (a reset between them) of a fresh context under the current environment."""
    from xrsfm_amd import capi
    out = {}
    ctx = capi.Context(H.to_product(arr))
    try:
        ctx.debug_linearize(HUBER_A, True)
        y, _ = ctx.debug_cholesky_solve(RADIUS)
        assert np.isfinite(y).all()
        dbg = ctx.debug_backsub()
        out.update({k: np.array(dbg[k], copy=True) for k in DEBUG_KEYS})
        lay = ctx.debug_backsub_layout()
        out["step_prep"], out["stored_j"], out["item_tiles"] = lay["step_prep"], lay["stored_j"], lay["item_tiles"]
        kw = dict(max_iterations=8)
        if solver is not None:
            kw["linear_solver"] = solver
        for r in range(runs):
            ctx.reset()
            s = ctx.run(capi.default_options(**kw))
            q, t, P = ctx.download()
            out[f"run{r}"] = {k: getattr(s, k) for k in SUMMARY_KEYS}
            out[f"q{r}"], out[f"t{r}"], out[f"P{r}"] = q, t, P
    finally:
        ctx.close()
    return out


def _same_bits(a, b):
    a = np.ascontiguousarray(a, np.float64); b = np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and bool((a.view(np.uint64) == b.view(np.uint64)).all())


def _compare(monkeypatch, arr, what, solver=None, runs=1, want=None):
    monkeypatch.setenv("XRSFM_BA_BACKSUB_LEAN", "0")
    ref = _snapshot(arr, solver, runs)
    monkeypatch.delenv("XRSFM_BA_BACKSUB_LEAN")
    got = _snapshot(arr, solver, runs)
    if want is not None:
        assert (got["step_prep"], got["stored_j"]) == want == (ref["step_prep"], ref["stored_j"]), "the variant under test did not run"
    assert np.isfinite(ref["part_model"]).all() and np.isfinite(ref["cand_points"]).all()
    assert np.abs(ref["point_step"]).max() > 0 and ref["part_model"].sum() != 0       # a step was taken: the comparison is not of zeros
    for k in DEBUG_KEYS:
        assert _same_bits(ref[k], got[k]), (what, k, int((ref[k] != got[k]).sum()), float(np.nanmax(np.abs(ref[k] - got[k]))))
    for r in range(runs):
        assert ref[f"run{r}"] == got[f"run{r}"], (what, r, ref[f"run{r}"], got[f"run{r}"])
        assert ref[f"run{r}"]["n_successful"] > 0
        for k in ("q", "t", "P"):
            assert _same_bits(ref[f"{k}{r}"], got[f"{k}{r}"]), (what, r, k)
    return ref, got


@pytest.mark.parametrize("jfree", ["1", "0"])
@pytest.mark.parametrize("name", list(PROBLEMS))
def test_lean_equals_parent(lib, monkeypatch, name, jfree):
    monkeypatch.setenv("XRSFM_BA_JFREE", jfree)
    _, got = _compare(monkeypatch, _problem(name), (name, jfree), want=(True, jfree == "0"))
    tiles = got["item_tiles"][:, 1]
    assert sorted(tiles[tiles > 1].tolist()) == ([2, 3] if name == "long" else [])


def test_lean_equals_parent_pcg(lib, monkeypatch):
    """k_backsub<false> on the inverses k_point_prep stored, stored J, and a run of the PCG solver."""
    from xrsfm_amd import capi
    monkeypatch.setenv("XRSFM_BA_PREP_FUSED", "0")
    monkeypatch.setenv("XRSFM_BA_JFREE", "0")
    ref, _ = _compare(monkeypatch, _problem("ragged"), "pcg", solver=capi.SOLVER_PCG, want=(False, True))
    assert ref["run0"]["linear_solver_used"] == capi.SOLVER_PCG


@pytest.mark.parametrize("jfree", ["1", "0"])
def test_lean_equals_parent_run_reset_run(lib, monkeypatch, jfree):
    monkeypatch.setenv("XRSFM_BA_JFREE", jfree)
    ref, got = _compare(monkeypatch, _problem("ragged"), ("rerun", jfree), runs=2)
    assert got["run0"] == got["run1"] and _same_bits(got["P0"], got["P1"]) and _same_bits(got["q0"], got["q1"])
