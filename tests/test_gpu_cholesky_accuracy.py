"""Accuracy of the tile Cholesky step on every schedule: the damped reduced system S y = b exactly as the factorisation reads it
(xrsfm_ba_debug_reduced_system) against the solution the same factorisation returns — backward error in extended precision,
forward error against an iteratively refined LAPACK / SuperLU solution — at trust-region radii from a solve's start (1e4) to
its cap (1e16).  The cases are chosen so that together they realise every schedule fact and pivot-tile height
(test_catalogue_covers_every_schedule, CPU only)."""
import os

import numpy as np
import pytest

from tests import helpers as H

RADII = (1e4, 1e8, 1e12, 1e16)
# Backward error bar, about 22 eps.  Measured on an MI355X over every case, context and radius: at most 3.6e-16 up to 1 380
# unknowns, 1.3e-15 on the 2400-photo collection (14 400 unknowns; LAPACK / SuperLU on the same systems: <= 1.8e-16).  The results
# are bit-reproducible (fixed-order sums), so the bar keeps 4x headroom over the largest measured value.  It does not separate a
# pivot rsqrt with one Newton step instead of two (ba_chol.h: potrf_panel4 chains): that raises eta by 1.6x on average (81 % of the
# values grow, at most 21x: 8.1e-17 -> 2.3e-16 on one camera), to at most 1.2e-15, inside the spread of the correct build.
ETA_BAR = 5e-15
FWD_FLOOR = 1e-14      # forward error floor next to 10 x that of the plain LAPACK solve


def _band(n_cams, k_obs, seed, **kw):
    return lambda: H.make(n_cams, 30 * n_cams, k_obs, seed=seed, min_tri_angle_deg=0.5, **kw)


def _const_blocks():
    arr = H.make(48, 1500, 4, seed=311, min_tri_angle_deg=0.5)
    cc = np.zeros(48, np.uint8)
    cc[0] = 3; cc[17] = 1; cc[30] = 2          # fixed camera, fixed rotation, fixed translation
    arr["cam_const"] = cc
    pc = np.zeros(arr["points"].shape[0], np.uint8)
    pc[::7] = 1
    arr["point_const"] = pc
    return arr


def _unordered(n_cams, seed):
    return lambda: H.make(n_cams, 40 * n_cams, 5, seed=seed, mode="unordered")


def _collection(n_cams, n_points, seed, per):
    def f():
        from xrsfm_amd import capi, synth
        d = synth.make_collection(n_cams=n_cams, n_points=n_points, seed=seed, cams_per_cluster=per)
        return {k: d[k] for k in capi.ProblemArrays.FIELDS}
    return f


def _bal9(n_cams, k_obs, seed):
    return lambda: H.make_bal9(n_cams, 30 * n_cams, k_obs, seed=seed, min_tri_angle_deg=0.5)


# name -> (problem factory, [environment per context], use_scaling).  Each environment is one context (the plan and the schedule
# switches are read when the context sets up its factorisation); every context runs all radii.
_C2400 = _collection(2400, 100000, 4, 60)
CASES = {
    "one_camera": (lambda: H.make_pose_problem(200, seed=3), [{}], True),
    "two_cameras": (lambda: H.make(2, 150, 2, seed=301), [{}], True),
    "ten_cameras": (lambda: H.make(10, 400, 3, seed=302), [{}], True),
    "eleven_cameras": (lambda: H.make(11, 400, 3, seed=303), [{}], True),
    **{f"band_k{k}": (_band(40 + 8 * k, k, 320 + k), [{}], True) for k in range(2, 12)},
    "band_k4_unscaled": (_band(60, 4, 340), [{}], False),
    "band_hubs": (lambda: H.make(240, 7200, 4, seed=341, min_tri_angle_deg=0.5, n_hubs=24, hub_tracks=20),
                  [{}, {"XRSFM_BA_BWD_ALL": "0"}, {"XRSFM_BA_PACKED": "1"}], True),
    "ragged": (lambda: H.make(120, 4800, 8, seed=342, min_tri_angle_deg=0.5, dropout=0.35), [{}], True),
    "const_blocks": (_const_blocks, [{}], True),
    **{f"unordered_T{(n + 9) // 10}": (_unordered(n, 350 + n), [{}], True) for n in (13, 24, 37, 46, 59, 68, 75)},
    "unordered_T13_macro": (_unordered(125, 363), [{"XRSFM_BA_PANEL_MACRO": "1", "XRSFM_BA_PANEL_COLS": c, "XRSFM_BA_LOOKAHEAD": "0"}
                                                   for c in ("2", "4", "6")], True),
    "unordered_T8_packed": (_unordered(75, 425), [{"XRSFM_BA_PACKED": "1"}], True),
    "collection_600": (_collection(600, 30000, 5, 60), [{}], True),
    "collection_2400": (_C2400, [{}] + [{"XRSFM_BA_LA_DEPTH": d} for d in ("0", "1", "3")]
                        + [{"XRSFM_BA_BWD_ALL": "0"}, {"XRSFM_BA_BWD_ALL": "0", "XRSFM_BA_BWD_CHUNK": "0"}], True),
    **{f"bal9_k{k}_n{n}": (_bal9(n, k, 370 + k), [{}], True) for k, n in ((2, 42), (3, 49), (3, 53), (4, 54))},
}
_ORACLE_MAX_CAMS = 300
# the schedule switches of the photo collection (one context each: 14 400 unknowns) run at a solve's start and near convergence;
# its default context runs every radius
_SWITCH_RADII = {"collection_2400": (1e4, 1e12)}


class _Env:
    """Set environment variables for one context's set-up, restore them afterwards."""
    def __init__(self, env):
        self.env, self.old = env, {}

    def __enter__(self):
        for k, v in self.env.items():
            self.old[k] = os.environ.get(k)
            os.environ[k] = v

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _plan_facts(arr, env):
    from xrsfm_amd import capi
    with _Env(env):
        return capi.debug_chol_plan(H.to_product(arr))["facts"]


_PLANS = {}


def _all_plans():
    if not _PLANS:
        for name, (make, envs, _) in CASES.items():
            arr = make()
            _PLANS[name] = [_plan_facts(arr, env) for env in envs]
    return _PLANS


def test_catalogue_covers_every_schedule(lib):
    """CPU: the cases realise every schedule fact of the factorisation, every pivot-tile height on the level schedule and on
    the panel schedules (6 .. 60 rows; 9 .. 63 in bal9 mode), one tile, two tiles with a one-camera last tile, and the smallest
    look-ahead plan (T = 8)."""
    plans = _all_plans()
    facts = [f for fs in plans.values() for f in fs]
    assert {f["schedule"] for f in facts} == {"level", "panel", "lookahead"}
    assert {f["bwd"] for f in facts} == {"fused", "per_level", "all", "chunk", "push"}
    assert {f["ordering"] for f in facts} == {0, 1, 2, 3}
    assert {f["la_depth"] for f in facts if f["schedule"] == "level"} >= {0, 1, 2, 3}
    assert any(f["la_depth"] > 0 and f["schedule"] == "level" for f in facts)
    assert any(f["macro_levels"] > 0 for f in facts) and any(f["split_levels"] > 0 for f in facts)
    assert any(f["rest_apart"] for f in facts) and any(f["fill_rest"] > 0 and not f["rest_apart"] and f["schedule"] == "level" for f in facts)
    assert any(f["fill_rest"] > 0 and f["schedule"] == "lookahead" for f in facts)
    assert any(f["packed"] and f["schedule"] == "level" for f in facts) and any(f["packed"] and f["schedule"] == "lookahead" for f in facts)
    six = [f for f in facts if f["cw"] == 6]
    lv = set().union(*(f["heights"] for f in six if f["schedule"] == "level"))
    pn = set().union(*(f["heights"] for f in six if f["schedule"] != "level"))
    assert lv >= set(range(6, 61, 6)), sorted(set(range(6, 61, 6)) - lv)
    assert pn >= set(range(6, 61, 6)), sorted(set(range(6, 61, 6)) - pn)
    b9 = [f for f in facts if f["cw"] == 9]
    assert b9 and all(f["schedule"] == "level" for f in b9)
    h9 = set().union(*(f["heights"] for f in b9))
    assert h9 >= set(range(9, 64, 9)), sorted(set(range(9, 64, 9)) - h9)
    assert plans["one_camera"][0]["T"] == 1 and plans["one_camera"][0]["bwd"] == "fused"
    f11 = plans["eleven_cameras"][0]
    assert f11["T"] == 2 and 6 in f11["heights"] and 60 in f11["heights"]
    assert plans["unordered_T8"][0]["schedule"] == "lookahead" and plans["unordered_T8"][0]["T"] == 8
    assert plans["unordered_T7"][0]["schedule"] == "panel"
    assert all(f["macro_levels"] > 0 for f in plans["unordered_T13_macro"])


_REF = {}


def _reference(key, S, b):
    """Reference solve, shared by the contexts of one problem whose S and b are bit-identical."""
    hit = _REF.get(key)
    if hit is not None and hit[0].shape == S.shape and (hit[0] != S).nnz == 0 and np.array_equal(hit[1], b):
        return hit[2]
    ref = H.reference_solve(S, b.reshape(-1))
    _REF.clear()
    _REF[key] = (S, b.copy(), ref)
    return ref


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_step_backward_error(lib, case):
    """Per context and radius: (1) the solution of the plain path (what a run executes: tiles composed inside the first factor
    launch) equals that of the materialised path bit for bit; (2) it is finite with a backward error <= ETA_BAR at radius <= 1e8,
    and either non-finite (the controller rejects such a step) or as accurate at 1e12 / 1e16; (3) where the refinement of the
    reference converges, the forward error is <= max(10 x that of a plain LAPACK / SuperLU solve, 1e-14); (4) up to 300
    cameras, S and b equal the oracle's to 1e-11."""
    from xrsfm_amd import capi
    make, envs, use_scaling = CASES[case]
    arr = make()
    bal9 = bool((np.asarray(arr["cam_const"]) & 4).any())       # (9-wide camera blocks: XRSFM_BA_INTR_VARIABLE)
    fails, rows = [], []
    for env in envs:
        tag = ",".join(f"{k[9:]}={v}" for k, v in env.items()) or "default"
        with _Env(env):
            plan = capi.debug_chol_plan(H.to_product(arr))["facts"]
            ctx = capi.Context(H.to_product(arr))
            try:
                if not bal9:
                    ctx.debug_linearize(5.99, use_scaling)
                for radius in (RADII if env is envs[0] else _SWITCH_RADII.get(case, RADII)):
                    if bal9:
                        y_plain = ctx.debug_wide(radius=radius)["y"]
                    else:
                        y_plain, _ = ctx.debug_cholesky_solve(radius)
                    out = ctx.debug_reduced_system(radius)
                    S, b, y, f = out["S"], out["b"], out["y"], out["facts"]
                    where = f"{tag} r={radius:.0e}"
                    if f != plan:
                        fails.append(f"{where}: context facts {f} != plan facts {plan}")
                    if not np.array_equal(y_plain.view(np.uint64), y.view(np.uint64)):
                        fails.append(f"{where}: plain and materialised solutions differ (max {np.abs(y_plain - y).max():.3e})")
                    finite = bool(np.isfinite(y).all())
                    eta = H.backward_error(S, y, b) if finite else float("nan")
                    ref = _reference(case, S, b)
                    fwd = H.rel_err(y.reshape(-1), ref["y"]) if finite else float("nan")
                    rows.append(f"[eta] {case:22s} {tag:32s} r={radius:.0e} T={f['T']:3d} {f['schedule']:9s} bwd={f['bwd']:9s} "
                                f"eta_gpu={eta:.2e} eta_lapack={ref['eta0']:.2e} fwd_gpu={fwd:.2e} fwd_lapack={ref['err0']:.2e} "
                                f"refined={int(ref['converged'])}")
                    if radius <= 1e8 and not finite:
                        fails.append(f"{where}: non-finite step")
                    if finite and not eta <= ETA_BAR:
                        fails.append(f"{where}: backward error {eta:.3e} > {ETA_BAR:.0e} (LAPACK {ref['eta0']:.3e})")
                    if finite and ref["converged"] and not fwd <= max(10 * ref["err0"], FWD_FLOOR):
                        fails.append(f"{where}: forward error {fwd:.3e} > max(10 x {ref['err0']:.3e}, {FWD_FLOOR:.0e})")
                    if not bal9 and arr["cam_q"].shape[0] <= _ORACLE_MAX_CAMS and env is envs[0]:
                        S_ref, b_ref = H.reduced_system_oracle(arr, radius, use_scaling)
                        eS, eb = H.rel_err(S.toarray(), S_ref), H.rel_err(b, b_ref)
                        if not (eS < 1e-11 and eb < 1e-11):
                            fails.append(f"{where}: S / b against the oracle {eS:.3e} / {eb:.3e}")
            finally:
                ctx.close()
    print("\n" + "\n".join(rows))
    assert not fails, "\n".join(fails)
