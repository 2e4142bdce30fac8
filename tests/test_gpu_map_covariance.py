"""xrsfm_ba_map_covariance on the GPU: every camera and point block against the dense CPU inverses (tests/cov_map_yardstick.py: route A
of the camera and of the point yardstick, tolerance 50 x eps_ref + 1e-12 per block), against the selected calls, the fallback, dense
against packed tiles, repeatability, relabelling, status values and special cases, errors, side effects, and the call at size (config L;
the 20 000-camera sequential shape on packed tiles)."""
import ctypes as C
import os
import subprocess
import sys
import textwrap
import time

import numpy as np
import pytest

from tests import cov_map_yardstick as M
from tests import cov_point_yardstick as P
from tests import cov_yardstick as Y
from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL_FIXTURES = [n for n, (_, want) in M.FIXTURES.items() if want in ("level", "single")]      # the fixtures the kernels serve
SELECTED_MS_PER_CHUNK_L = 1.23          # xrsfm_ba_point_covariance, 21 points on config L (profiles/cov_timing.md)
_YARD = {}


def _yard(name):
    if name not in _YARD:
        _YARD[name] = M.yard(name)
    return _YARD[name]


def _ctx(arr):
    from xrsfm_amd import capi
    return capi.Context(H.to_product(arr))


def _map(arr):
    ctx = _ctx(arr)
    try:
        return ctx.map_covariance()
    finally:
        ctx.close()


def _raw(ctx, fill=7.0):
    p = ctx.problem
    cc, pc = np.full((p.n_cams, 6, 6), fill), np.full((p.n_points, 3, 3), fill)
    cs, ps = np.full(p.n_cams, 7, np.uint8), np.full(p.n_points, 7, np.uint8)
    dp, bp = C.POINTER(C.c_double), C.POINTER(C.c_uint8)
    rc = ctx.lib.xrsfm_ba_map_covariance(ctx._h, 5.99, cc.ctypes.data_as(dp), pc.ctypes.data_as(dp), cs.ctypes.data_as(bp), ps.ctypes.data_as(bp))
    return rc, cc, pc, cs, ps


def _untouched(out):
    _, cc, pc, cs, ps = out
    return (cc == 7.0).all() and (pc == 7.0).all() and (cs == 7).all() and (ps == 7).all()


def _expected_cam_status(arr):
    return np.where((np.asarray(arr["cam_const"]) & 3) == 3, 1, 0).astype(np.uint8)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(M.FIXTURES))
def test_against_dense_inverse(lib, name):
    arr, Ac, ec, Ap, ep = _yard(name)
    want = M.FIXTURES[name][1]
    if want is not None:
        assert Y.schedule_of(arr) == want          # asserted with xrsfm_ba_debug_chol_plan, not assumed
    if name == "deep3":
        assert M.is_deep3(arr), M.deep3_facts(arr)
    G = _map(arr)
    Gc, Gp = G["cam_cov"], G["pt_cov"]
    rc, rp = Y.rel_blocks(Gc, Ac), P.rel_blocks(Gp, Ap)
    print(f"{name}: schedule {Y.schedule_of(arr)}; cameras eps_ref {ec:.3e}, GPU max rel {rc.max():.3e} = {rc.max() / max(ec, 1e-300):.2f} x eps_ref; "
          f"points eps_ref {ep:.3e}, GPU max rel {rp.max():.3e} = {rp.max() / max(ep, 1e-300):.2f} x eps_ref")
    assert np.isfinite(Gc).all() and np.isfinite(Gp).all()
    assert (Gc == np.swapaxes(Gc, 1, 2)).all() and (Gp == np.swapaxes(Gp, 1, 2)).all()
    assert (rc <= Y.tolerance(ec)).all(), (name, float(rc.max()), ec)
    assert (rp <= P.tolerance(ep)).all(), (name, float(rp.max()), ep)
    assert (G["cam_status"] == _expected_cam_status(arr)).all()
    assert (G["cam_status"] == 1).any()                      # the gauge camera: fully constant, a zero block
    assert (Gc[G["cam_status"] == 1] == 0).all()
    assert (G["pt_status"] == 0).all()                       # every point of a fixture is observed and free
    if name == "long70":
        n_obs = np.bincount(arr["obs_pt"])
        assert sorted(n_obs[list(M.LONG70_POINTS)]) == [66, 70] and np.sort(n_obs)[-3] <= 64          # the two tracks of the workgroup kernel
        assert (rp[list(M.LONG70_POINTS)] <= P.tolerance(ep)).all() and (np.linalg.eigvalsh(Gp[list(M.LONG70_POINTS)]) > 0).all()
    if name == "const_q":
        g = Gc[Y.CONST_Q_CAM]
        assert (g[:3] == 0).all() and (g[:, :3] == 0).all() and (np.diag(g)[3:] > 0).all() and G["cam_status"][Y.CONST_Q_CAM] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(KERNEL_FIXTURES))
def test_against_selected_calls(lib, name):
    """The forward-substitution calls over all cameras and all observed points: the same blocks by another computation."""
    arr, Ac, ec, Ap, ep = _yard(name)
    ctx = _ctx(arr)
    try:
        G = ctx.map_covariance()
        Sc = ctx.covariance(np.arange(arr["cam_q"].shape[0]))
        sel = P.observed_points(arr)
        Sp = ctx.point_covariance(sel)
        only_c = ctx.map_covariance(points=False)
        only_p = ctx.map_covariance(cameras=False)
    finally:
        ctx.close()
    rc, rp = Y.rel_blocks(G["cam_cov"], Sc), P.rel_blocks(G["pt_cov"][sel], Sp)
    print(f"{name}: whole map vs selected calls: cameras max rel {rc.max():.3e} (eps_ref {ec:.3e}), points {rp.max():.3e} (eps_ref {ep:.3e})")
    assert (rc <= 50.0 * ec).all() and (rp <= 50.0 * ep).all()
    if name in ("level40", "deep3"):
        assert (G["cam_cov"] != Sc).any() and (G["pt_cov"][sel] != Sp).any()          # two different computations
    assert set(only_c) == {"cam_cov", "cam_status"} and set(only_p) == {"pt_cov", "pt_status"}
    assert (only_c["cam_cov"] == G["cam_cov"]).all() and (only_p["pt_cov"] == G["pt_cov"]).all()


_CHILD = textwrap.dedent("""
    import sys, numpy as np
    sys.path.insert(0, %r)
    import torch  # noqa: F401
    from tests import cov_map_yardstick as M
    from tests import helpers as H
    from xrsfm_amd import capi
    out = {}
    for name in sys.argv[2:]:
        arr = M.FIXTURES[name][0]()
        ctx = capi.Context(H.to_product(arr))
        G = ctx.map_covariance()
        ctx.close()
        for k, v in G.items():
            out[name + "/" + k] = v
    np.savez(sys.argv[1], **out)
""")


@pytest.mark.gpu
def test_kernel_against_fallback(lib, tmp_path):
    """A/B: XRSFM_BA_COV_FALLBACK=1 in a fresh child process (the selected calls' own fallback over everything in the program)."""
    names = sorted(KERNEL_FIXTURES)
    assert "level40" in names and "ring10" in names and "deep3" in names
    env = dict(os.environ)
    env["XRSFM_BA_COV_FALLBACK"] = "1"
    out = str(tmp_path / "fallback.npz")
    r = subprocess.run([sys.executable, "-c", _CHILD % ROOT, out] + names, capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    fb = np.load(out)
    assert os.environ.get("XRSFM_BA_COV_FALLBACK", "0") == "0"
    for name in names:
        arr, Ac, ec, Ap, ep = _yard(name)
        G = _map(arr)
        rc, rp = Y.rel_blocks(fb[name + "/cam_cov"], G["cam_cov"]), P.rel_blocks(fb[name + "/pt_cov"], G["pt_cov"])
        print(f"{name}: kernel vs fallback: cameras max rel {rc.max():.3e} (eps_ref {ec:.3e}), points {rp.max():.3e} (eps_ref {ep:.3e})")
        if name in ("level40", "deep3"):
            assert (fb[name + "/cam_cov"] != G["cam_cov"]).any() and (fb[name + "/pt_cov"] != G["pt_cov"]).any()      # the switch did switch
        assert (rc <= 50.0 * ec).all() and (rp <= 50.0 * ep).all()
        assert (fb[name + "/cam_status"] == G["cam_status"]).all() and (fb[name + "/pt_status"] == G["pt_status"]).all()
        assert (Y.rel_blocks(fb[name + "/cam_cov"], Ac) <= Y.tolerance(ec)).all() and (P.rel_blocks(fb[name + "/pt_cov"], Ap) <= P.tolerance(ep)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["deep3", "level40"])
def test_dense_and_packed_tiles_agree_bit_for_bit(lib, name, monkeypatch):
    from xrsfm_amd import capi
    arr = _yard(name)[0]
    got = {}
    for packed in ("1", "0"):
        monkeypatch.setenv("XRSFM_BA_PACKED", packed)          # (read when the context sets the factorisation up)
        assert capi.debug_chol_plan(H.to_product(arr))["facts"]["packed"] == (packed == "1")
        got[packed] = _map(arr)
    for k in ("cam_cov", "pt_cov", "cam_status", "pt_status"):
        assert (got["1"][k] == got["0"][k]).all(), k


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["deep3", "ring12"])
def test_repeatable(lib, name):
    """Two calls are bit-identical (kernel path and fallback path), on one context and on a fresh one."""
    arr = _yard(name)[0]
    ctx = _ctx(arr)
    try:
        G1, G2 = ctx.map_covariance(), ctx.map_covariance()
    finally:
        ctx.close()
    G3 = _map(arr)
    for k in G1:
        assert (G1[k] == G2[k]).all() and (G1[k] == G3[k]).all(), k


@pytest.mark.gpu
def test_relabelled_points_permute_the_rows(lib):
    """helpers.relabel_points changes the order of every per-camera sum, so the rows agree within the tolerance rule, not bit for bit."""
    arr, Ac, ec, Ap, ep = _yard("deep3")
    G = _map(arr)
    rel, perm = H.relabel_points(arr, seed=4)
    R = _map(rel)
    rc, rp = Y.rel_blocks(R["cam_cov"], G["cam_cov"]), P.rel_blocks(R["pt_cov"], G["pt_cov"][perm])
    print(f"deep3 relabelled: cameras max rel {rc.max():.3e}, points {rp.max():.3e}")
    assert (rc <= Y.tolerance(ec)).all() and (rp <= P.tolerance(ep)).all()
    assert (P.rel_blocks(R["pt_cov"], Ap[perm]) <= P.tolerance(ep)).all()


@pytest.mark.gpu
def test_constant_point(lib):
    base = _yard("deep3")[0]
    arr = dict(base)
    j, k = 5, 6
    pc = np.array(base["point_const"], np.uint8, copy=True)
    pc[j] = 1
    arr["point_const"] = pc
    A, B = P.route_a(arr), P.route_b(arr)
    G = _map(arr)
    assert G["pt_status"][j] == 1 and (G["pt_cov"][j] == 0).all()
    assert G["pt_status"][k] == 0 and (np.delete(G["pt_status"], j) == 0).all()
    assert (P.rel_blocks(G["pt_cov"], A) <= P.tolerance(P.eps_ref(A, B))).all()


@pytest.mark.gpu
def test_point_seen_by_constant_cameras_only(lib):
    base = _yard("deep3")[0]
    j = 40
    arr = P.lba_shaped(base, j)
    A, B = P.route_a(arr), P.route_b(arr)
    eps = P.eps_ref(A, B)
    G = _map(arr)
    rel = P.rel_blocks(G["pt_cov"][j:j + 1], P.point_hinv(arr, j)[None])[0]
    print(f"deep3: point {j} under constant cameras: rel {rel:.3e} against inv(E^T E), eps_ref {eps:.3e}")
    assert rel <= P.tolerance(eps) and G["pt_status"][j] == 0
    cams = np.unique(arr["obs_cam"][arr["obs_pt"] == j])
    assert (G["cam_status"][cams] == 1).all() and (G["cam_cov"][cams] == 0).all()
    assert (P.rel_blocks(G["pt_cov"], A) <= P.tolerance(eps)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["deep3", "ring12"])
def test_unobserved_point_and_camera_are_reported(lib, name):
    """An appended point without an observation (and a camera without one): status 2, zero blocks, every other block bit-equal."""
    arr = _yard(name)[0]
    G = _map(arr)
    ext = dict(arr)
    j = arr["points"].shape[0]
    ext["points"] = np.concatenate([arr["points"], arr["points"][:1] + 0.1])
    ext["point_const"] = np.concatenate([arr["point_const"], np.zeros(1, np.uint8)])
    E = _map(ext)
    assert E["pt_status"][j] == 2 and (E["pt_cov"][j] == 0).all() and (E["pt_status"][:j] == 0).all()
    assert (E["pt_cov"][:j] == G["pt_cov"]).all() and (E["cam_cov"] == G["cam_cov"]).all() and (E["cam_status"] == G["cam_status"]).all()
    n = arr["cam_q"].shape[0]
    for k in ("cam_q", "cam_t", "cam_const", "cam_intr"):
        ext[k] = np.concatenate([ext[k], ext[k][-1:]])
    E = _map(ext)
    assert E["cam_status"][n] == 2 and (E["cam_cov"][n] == 0).all()
    # (one more camera can move the tile layout: the tolerance rule, not bit equality)
    _, Ac, ec, Ap, ep = _yard(name)
    assert (Y.rel_blocks(E["cam_cov"][:n], Ac) <= Y.tolerance(ec)).all() and (P.rel_blocks(E["pt_cov"][:j], Ap) <= P.tolerance(ep)).all()


@pytest.mark.gpu
def test_errors_leave_the_outputs_untouched(lib, capfd):
    arr = _yard("ring12")[0]
    # a free point with one observation
    ext = dict(arr)
    j = arr["points"].shape[0]
    ext["points"] = np.concatenate([arr["points"], arr["points"][:1] + 0.1])
    ext["point_const"] = np.concatenate([arr["point_const"], np.zeros(1, np.uint8)])
    o = int(np.nonzero(arr["obs_pt"] == 0)[0][0])
    ext["obs_cam"] = np.concatenate([arr["obs_cam"], arr["obs_cam"][o:o + 1]])
    ext["obs_pt"] = np.concatenate([arr["obs_pt"], np.array([j], np.int32)])
    ext["obs_uv"] = np.concatenate([arr["obs_uv"], arr["obs_uv"][o:o + 1] + 3.0])
    ctx = _ctx(ext)
    try:
        out = _raw(ctx)
        assert out[0] == -8 and _untouched(out)
        assert f"caller point {j}" in capfd.readouterr().err
    finally:
        ctx.close()
    ctx = _ctx(arr)
    try:
        assert ctx.lib.xrsfm_ba_map_covariance(ctx._h, 5.99, None, None, None, None) == 0
        out = _raw(ctx)
        assert out[0] == 0 and np.isfinite(out[1]).all() and (out[3] <= 1).all()
        ctx.comm_hook(1, 0, lambda buf, op: None)          # a context with the test transport attached counts as multi-rank
        out = _raw(ctx)
        assert out[0] == -1 and _untouched(out)
    finally:
        ctx.close()
    b9 = _ctx(H.make_bal9(12, 300, 4, seed=5))
    try:
        out = _raw(b9)
        assert out[0] == -1 and _untouched(out)
        with pytest.raises(RuntimeError, match="EINVAL"):
            b9.map_covariance()
    finally:
        b9.close()
    dup = dict(arr)          # a track observed twice by one camera
    dup["obs_cam"] = np.concatenate([arr["obs_cam"], arr["obs_cam"][:1]])
    dup["obs_pt"] = np.concatenate([arr["obs_pt"], arr["obs_pt"][:1]])
    dup["obs_uv"] = np.concatenate([arr["obs_uv"], arr["obs_uv"][:1] + 0.5])
    ctx = _ctx(dup)
    try:
        out = _raw(ctx)
        assert out[0] == -1 and _untouched(out)
    finally:
        ctx.close()


@pytest.mark.gpu
def test_side_effect_free(lib):
    from xrsfm_amd import capi
    arr = _yard("deep3")[0]

    def summary(s):
        return (s.initial_cost, s.final_cost, s.n_successful, s.n_unsuccessful, s.termination, s.termination_reason, s.lm_steps_attempted)

    ctx = _ctx(arr)
    try:
        s0 = ctx.run(capi.default_options(linear_solver=capi.SOLVER_CHOLESKY))
        ref = ctx.download()
    finally:
        ctx.close()
    ctx = _ctx(arr)
    try:
        G0 = ctx.map_covariance()
        s1 = ctx.run(capi.default_options(linear_solver=capi.SOLVER_CHOLESKY))
        got = ctx.download()
        assert summary(s1) == summary(s0)
        for a, b in zip(got, ref):
            assert (a == b).all()
        G1 = ctx.map_covariance()          # after the run: the refined state
        assert (G1["pt_cov"] != G0["pt_cov"]).any()
        state = dict(arr)
        state["cam_q"], state["cam_t"], state["points"] = got
        A1, B1 = P.route_a(state), P.route_b(state)
        assert (P.rel_blocks(G1["pt_cov"], A1) <= P.tolerance(P.eps_ref(A1, B1))).all()
        Gc = ctx.covariance([5, 17, 33])          # the selected calls of the same context are not disturbed
        ctx.map_covariance()
        assert (ctx.covariance([5, 17, 33]) == Gc).all()
        ctx.reset()
        ctx.map_covariance()
        s2 = ctx.run(capi.default_options(linear_solver=capi.SOLVER_CHOLESKY))
        assert summary(s2) == summary(s0)
        for a, b in zip(ctx.download(), ref):
            assert (a == b).all()
    finally:
        ctx.close()


def _spread(arr, m):
    """m observed points whose first observing cameras are spread evenly over the cameras."""
    first = np.full(arr["points"].shape[0], arr["cam_q"].shape[0], np.int64)
    np.minimum.at(first, arr["obs_pt"], arr["obs_cam"])
    n_cams = arr["cam_q"].shape[0]
    order = np.argsort(first, kind="stable")
    order = order[first[order] < n_cams]
    return order[np.linspace(0, order.shape[0] - 1, m).astype(int)].astype(np.int32)


def _at_size(arr, n_pts_sel, want_packed, capfd):
    """Every point block finite, exactly symmetric and positive definite; spread points and 10 cameras within 1e-8 relative of the
    selected calls on the same context (the bound of the neighbours at size).  Prints the time of the call and how many 21-point
    chunks of the selected call on config L it costs (no time bound is asserted)."""
    from xrsfm_amd import capi
    arr = Y.fix_gauge(arr)
    plan = capi.debug_chol_plan(H.to_product(arr))
    assert plan["level_schedule"] == 1 and plan["facts"]["packed"] == want_packed, plan["facts"]
    sel = _spread(arr, n_pts_sel)
    assert np.unique(sel).shape[0] == n_pts_sel
    n_cams = arr["cam_q"].shape[0]
    cams = np.linspace(2, n_cams - 1, 10).astype(np.int32)
    ctx = _ctx(arr)
    try:
        ctx.map_covariance(points=False)          # (first call: the set-up of the factorisation)
        os.environ["XRSFM_BA_COV_TIMING"] = "1"
        try:
            capfd.readouterr()
            t0 = time.perf_counter()
            G = ctx.map_covariance()
            dt = 1e3 * (time.perf_counter() - t0)
            line = [ln for ln in capfd.readouterr().err.splitlines() if "map_covariance:" in ln]
        finally:
            del os.environ["XRSFM_BA_COV_TIMING"]
        Sc = ctx.covariance(cams)
        Sp = ctx.point_covariance(sel)
    finally:
        ctx.close()
    Gp, Gc = G["pt_cov"], G["cam_cov"]
    n_obs_pts = np.unique(arr["obs_pt"]).shape[0]
    print(f"T {plan['tiles']}, levels {plan['levels']}, packed {plan['facts']['packed']}: {n_cams} cameras, {n_obs_pts} points: {dt:.1f} ms per call "
          f"= {dt / SELECTED_MS_PER_CHUNK_L:.0f} chunks of the selected point call on config L ({SELECTED_MS_PER_CHUNK_L} ms per 21 points); {line}")
    assert np.isfinite(Gp).all() and np.isfinite(Gc).all()
    assert (Gp == np.swapaxes(Gp, 1, 2)).all() and (Gc == np.swapaxes(Gc, 1, 2)).all()
    est = G["pt_status"] == 0
    assert est.sum() == n_obs_pts
    assert np.linalg.eigvalsh(Gp[est]).min() > 0
    rp, rc = P.rel_blocks(Gp[sel], Sp), Y.rel_blocks(Gc[cams], Sc)
    print(f"    whole map vs selected calls: {n_pts_sel} points max rel {rp.max():.3e}, 10 cameras {rc.max():.3e}")
    assert (rp <= 1e-8).all() and (rc <= 1e-8).all(), (float(rp.max()), float(rc.max()))


@pytest.mark.gpu
def test_config_L_whole_map(lib, capfd):
    from xrsfm_amd import synth
    d = synth.make_problem(**synth.CONFIGS["L"])
    _at_size({k: d[k] for k in H.FIELDS}, 21, False, capfd)


@pytest.mark.gpu
def test_packed_storage_20000_cameras(lib, capfd):
    """The 20 000-camera sequential shape of the selected calls' tests (every 2000th frame constant: see there)."""
    arr = H.make(20000, 400000, 4, seed=13)
    cc = arr["cam_const"].copy()
    cc[::2000] |= 3
    arr["cam_const"] = cc
    _at_size(arr, 8, True, capfd)
