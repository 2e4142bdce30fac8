"""Camera records staged in LDS once per tile (the default) against every lane gathering its camera's operands itself
(XRSFM_BA_CAM_STAGE=0), bit for bit: staging changes where the operands are read from, not one expression tree.

Compared per problem as uint64 views, with XRSFM_BA_JFREE=1 (recomputed F, E) and =0 (stored J): the outputs of debug_linearize and
debug_lin_scalars, debug_reduced_system(radius) (blocks, right-hand side, solution), debug_backsub (per-item partials, candidate
points and cameras, point_step), then the summary and the final state of an 8-iteration run.  debug_cam_stage() reports how many
tiles take each route (k_backsub and the merged k_schur_pairs launch evaluate one predicate): the staged count is
positive by default and zero with the switch off, so the variant under test ran.
The problems are the smallest that reach every branch:
  regular   12 cameras: full tiles of one tuple each (lengths 2, 3, 4; one tuple holds camera 0 and the last camera) next to
            mixed tiles; the last tile has a few occupied lanes
  ragged    missed detections: 5-8 cameras per tile and empty lanes (both staging passes)
  bound1    one-tile shapes of 9 and 10 cameras (Gram tiles past the bound of 8) and of 13 cameras (a per-pair tile) next to
            staged tiles of 4 and 8: both routes in one launch
  long      one track of 70 and one of 135 observations (items of 2 and 3 tiles: the long-item kernels), 140 cameras; the short
            tracks see scattered cameras (per-pair tiles) but for one regular tile
  consts    constant points, constant rotation / translation / both (zero sq / st through LDS), a camera without observations
  robust    Huber-branch outliers and points behind their cameras (the depth clamp)
  models    every camera model of tests/helpers.py::with_models (each reads another part of intr)
  pcg       the PCG solver on the ragged problem (stored J, stored point inverses)
  rerun     run, reset, run in one context (the wave's LDS between launches): the two runs are identical too"""
import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu

HUBER_A = 5.99
RADIUS = 1e4
LIN_KEYS = ("r", "Jc", "Jp", "Hpp", "gp", "Hcc_diag", "gc")
BACKSUB_KEYS = ("part_model", "part_step2", "cand_points", "point_step", "cand_cam_q", "cand_cam_t")
SUMMARY_KEYS = ("initial_cost", "final_cost", "n_successful", "n_unsuccessful", "termination", "lm_steps_attempted", "linear_solver_used")


def _regular():
    rng = np.random.default_rng(3)
    tracks = [np.array([0, 1])] * 64 + [np.array([0, 11])] * 32 + [np.array([2, 3, 4])] * 42 + [np.array([5, 6, 7, 8])] * 48
    tracks += [np.sort(rng.choice(12, int(n), replace=False)) for n in rng.integers(2, 5, 150)]
    return H.make_tracks(12, tracks, seed=21)


def _ragged():
    return H.make(40, 2000, 8, seed=33, dropout=0.35)


BOUND1_CELLS = [(4, 16, False), (8, 4, True), (9, 3, False), (9, 5, True), (10, 2, True), (13, 3, True)]


def _bound1():
    """One tile per cell of BOUND1_CELLS (C cameras, T tracks, ragged), laid out like tests/helpers.py::shape_problems."""
    rng = np.random.default_rng(4242)
    shape_tracks, base = [], 5
    for C, T, ragged in BOUND1_CELLS:
        tr, nxt = H.shape_group(base, C, T, ragged, rng, span=max(10, C + 1))
        shape_tracks += tr
        base = nxt - 3
    n_cams = base + 3
    tracks = [np.array([0, 1, c]) for c in range(2, n_cams) for _ in range(6)]
    tracks += [np.arange(1, 5) for _ in range(16)]
    return H.make_tracks(n_cams, tracks + shape_tracks, seed=100)


def _long():
    rng = np.random.default_rng(5)
    tracks = [np.sort(np.unique(np.arange(c, c + 4) % 140)) for c in rng.integers(0, 140, 300)]
    tracks += [np.arange(10, 14)] * 16              # one regular tile, so that the staged route runs next to the long items
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


PROBLEMS = {"regular": _regular, "ragged": _ragged, "bound1": _bound1, "long": _long, "consts": _consts, "robust": _robust,
            "models": _models}
_ARR = {}


def _problem(name):
    if name not in _ARR:
        _ARR[name] = PROBLEMS[name]()
    return _ARR[name]


def _snapshot(arr, solver=None, runs=1):
    """The debug entries once and `runs` 8-iteration runs (a reset before each) of a fresh context under the current environment."""
    from xrsfm_amd import capi
    out = {}
    ctx = capi.Context(H.to_product(arr))
    try:
        lin = ctx.debug_linearize(HUBER_A, True)
        out.update({k: np.array(lin[k], copy=True) for k in LIN_KEYS})
        out["cost"] = np.array([lin["cost"]])
        sc = ctx.debug_lin_scalars()
        out["scalars"] = np.array([sc[k] for k in ("sum_rho", "xnorm2_pts", "gradmax_pts", "gradmax_cams")])
        red = ctx.debug_reduced_system(RADIUS)
        S = red["S"].tocsr(); S.sort_indices()
        out["S_data"], out["S_indices"], out["S_indptr"], out["b"], out["y"] = S.data, S.indices, S.indptr, red["b"], red["y"]
        y, _ = ctx.debug_cholesky_solve(RADIUS)
        assert np.isfinite(y).all()
        dbg = ctx.debug_backsub()
        out.update({k: np.array(dbg[k], copy=True) for k in BACKSUB_KEYS})
        out["routes"] = ctx.debug_cam_stage()
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


def _compare(monkeypatch, arr, what, solver=None, runs=1):
    monkeypatch.setenv("XRSFM_BA_CAM_STAGE", "0")
    ref = _snapshot(arr, solver, runs)
    monkeypatch.delenv("XRSFM_BA_CAM_STAGE")
    got = _snapshot(arr, solver, runs)
    print("ROUTES", what, "switch off", ref["routes"], "default", got["routes"])
    assert ref["routes"][0] == 0 and ref["routes"][1] > 0, "XRSFM_BA_CAM_STAGE=0 must send every tile down the gather route"
    assert got["routes"][0] > 0, "the variant under test did not run"
    assert sum(got["routes"]) == sum(ref["routes"])
    assert np.isfinite(ref["part_model"]).all() and np.isfinite(ref["cand_points"]).all()
    assert np.abs(ref["point_step"]).max() > 0 and ref["part_model"].sum() != 0       # a step was taken: the comparison is not of zeros
    for k in ("S_indices", "S_indptr"):
        assert np.array_equal(ref[k], got[k]), (what, k)
    for k in LIN_KEYS + ("cost", "scalars", "S_data", "b", "y") + BACKSUB_KEYS:
        assert _same_bits(ref[k], got[k]), (what, k, int((ref[k] != got[k]).sum()), float(np.nanmax(np.abs(ref[k] - got[k]))))
    for r in range(runs):
        assert ref[f"run{r}"] == got[f"run{r}"], (what, r, ref[f"run{r}"], got[f"run{r}"])
        assert ref[f"run{r}"]["n_successful"] > 0
        for k in ("q", "t", "P"):
            assert _same_bits(ref[f"{k}{r}"], got[f"{k}{r}"]), (what, r, k)
    return ref, got


def test_bound1_has_tiles_on_both_sides_of_the_bound():
    """The problem itself (no kernel runs): Gram tiles of 9 and 10 cameras, a per-pair tile, and Gram tiles within the bound."""
    tiles, _ = H.tiles_of(_problem("bound1"))
    gram = sorted({C for C, _, _, _, klass in tiles if klass == "gram"})
    assert {4, 8, 9, 10} <= set(gram), gram
    assert any(klass == "pair" and C > 10 for C, _, _, _, klass in tiles), tiles


@pytest.mark.parametrize("jfree", ["1", "0"])
@pytest.mark.parametrize("name", list(PROBLEMS))
def test_staged_equals_gather(lib, monkeypatch, name, jfree):
    monkeypatch.setenv("XRSFM_BA_JFREE", jfree)
    _, got = _compare(monkeypatch, _problem(name), (name, jfree))
    if name == "bound1":
        assert got["routes"][1] > 0, "tiles past the bound must gather in the same launch"


def test_staged_equals_gather_pcg(lib, monkeypatch):
    """k_backsub<false> on the inverses k_point_prep stored, stored J, and a run of the PCG solver."""
    from xrsfm_amd import capi
    monkeypatch.setenv("XRSFM_BA_PREP_FUSED", "0")
    monkeypatch.setenv("XRSFM_BA_JFREE", "0")
    ref, _ = _compare(monkeypatch, _problem("ragged"), "pcg", solver=capi.SOLVER_PCG)
    assert ref["run0"]["linear_solver_used"] == capi.SOLVER_PCG


@pytest.mark.parametrize("jfree", ["1", "0"])
def test_staged_equals_gather_run_reset_run(lib, monkeypatch, jfree):
    monkeypatch.setenv("XRSFM_BA_JFREE", jfree)
    _, got = _compare(monkeypatch, _problem("ragged"), ("rerun", jfree), runs=2)
    assert got["run0"] == got["run1"] and _same_bits(got["P0"], got["P1"]) and _same_bits(got["q0"], got["q1"])
    assert _same_bits(got["t0"], got["t1"])
