"""xrsfm_ba_point_covariance on the GPU against a dense CPU inverse (tests/cov_point_yardstick.py: route A; tolerance
50 x eps_ref + 1e-12 per point, eps_ref = disagreement of the two CPU routes on that fixture), the panel kernel against the
fallback, repeatability, special points, argument errors, side effects, and the call at size (config L; the 20 000-camera
sequential shape on packed tiles)."""
import ctypes as C
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from tests import cov_point_yardstick as P
from tests import cov_yardstick as Y
from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_YARD = {}


def _yard(name):
    """(arr, A, eps_ref) of a fixture, computed once per session."""
    if name not in _YARD:
        arr = P.FIXTURES[name][0]()
        A, B = P.route_a(arr), P.route_b(arr)
        _YARD[name] = (arr, A, P.eps_ref(A, B))
    return _YARD[name]


def _ctx(arr):
    from xrsfm_amd import capi
    return capi.Context(H.to_product(arr))


def _raw(ctx, sel, fill=7.0):
    sel = np.ascontiguousarray(sel, np.int32)
    cov = np.full((max(1, sel.shape[0]), 3, 3), fill)
    rc = ctx.lib.xrsfm_ba_point_covariance(ctx._h, 5.99, sel.shape[0], sel.ctypes.data_as(C.POINTER(C.c_int32)), cov.ctypes.data_as(C.POINTER(C.c_double)))
    return rc, cov


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(P.FIXTURES))
def test_against_dense_inverse(lib, name):
    arr, A, eps = _yard(name)
    want = P.FIXTURES[name][1]
    if want is not None:
        assert P.schedule_of(arr) == want          # asserted with xrsfm_ba_debug_chol_plan, not assumed
    sel = P.observed_points(arr)
    assert sel.shape[0] == arr["points"].shape[0]          # all points: every point of a fixture has an observation
    ctx = _ctx(arr)
    try:
        G = ctx.point_covariance(sel)
        rel = P.rel_blocks(G, A[sel])
        print(f"{name}: schedule {P.schedule_of(arr)}, point eps_ref {eps:.3e}, GPU max rel {rel.max():.3e} = {rel.max() / max(eps, 1e-300):.2f} x eps_ref")
        assert np.isfinite(G).all()
        assert (rel <= P.tolerance(eps)).all(), (name, float(rel.max()), eps)
        assert (G == np.swapaxes(G, 1, 2)).all()
        # a 5-point subset in scrambled order: exactly the rows of the all-points call
        n = sel.shape[0]
        sub = np.array([n - 3, 2, n // 2, 77, n // 3])
        Gs = ctx.point_covariance(sel[sub])
        assert (Gs == G[sub]).all()
    finally:
        ctx.close()


_CHILD = textwrap.dedent("""
    import sys, numpy as np
    sys.path.insert(0, %r)
    import torch  # noqa: F401
    from tests import cov_point_yardstick as P
    from tests import helpers as H
    from xrsfm_amd import capi
    out = {}
    for name in sys.argv[2:]:
        arr = P.FIXTURES[name][0]()
        ctx = capi.Context(H.to_product(arr))
        out[name] = ctx.point_covariance(P.observed_points(arr)[::7])
        ctx.close()
    np.savez(sys.argv[1], **out)
""")


@pytest.mark.gpu
def test_kernel_against_fallback(lib, tmp_path):
    """A/B: XRSFM_BA_COV_FALLBACK=1 in a fresh child process (3 full solves per point with the run path's factor-and-solve;
    every 7th point of a fixture) against the panel kernel in this process, on the fixtures the kernel serves."""
    names = [n for n, (_, want) in P.FIXTURES.items() if want in ("level", "single")]
    assert "level40" in names and "ring10" in names
    env = dict(os.environ)
    env["XRSFM_BA_COV_FALLBACK"] = "1"
    out = str(tmp_path / "fallback.npz")
    r = subprocess.run([sys.executable, "-c", _CHILD % ROOT, out] + names, capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    fb = np.load(out)
    assert os.environ.get("XRSFM_BA_COV_FALLBACK", "0") == "0"
    for name in names:
        arr, A, eps = _yard(name)
        sel = P.observed_points(arr)[::7]
        ctx = _ctx(arr)
        try:
            G = ctx.point_covariance(sel)
        finally:
            ctx.close()
        rel = P.rel_blocks(fb[name], G)
        print(f"{name}: kernel vs fallback max rel {rel.max():.3e}, point eps_ref {eps:.3e}")
        if name == "level40":
            assert (fb[name] != G).any()          # two different computations: the switch did switch
        assert (rel <= 50.0 * eps).all(), (name, float(rel.max()), eps)
        assert (P.rel_blocks(fb[name], A[sel]) <= P.tolerance(eps)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["level40", "ring12"])
def test_repeatable(lib, name):
    """Two calls are bit-identical (kernel path and fallback path), and the order of pt_sel has no say."""
    arr, _, _ = _yard(name)
    sel = P.observed_points(arr)[:: (1 if name == "level40" else 25)]
    ctx = _ctx(arr)
    try:
        G1 = ctx.point_covariance(sel)
        G2 = ctx.point_covariance(sel)
        perm = np.random.default_rng(0).permutation(sel.shape[0])
        G3 = ctx.point_covariance(sel[perm])
    finally:
        ctx.close()
    assert (G1 == G2).all()
    assert (G3 == G1[perm]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["level40", "ring12"])
def test_constant_point_is_zero(lib, name):
    base, _, _ = _yard(name)
    arr = dict(base)
    obs = P.observed_points(base)
    j, k = int(obs[5]), int(obs[6])
    pc = np.array(base["point_const"], np.uint8, copy=True)
    pc[j] = 1
    arr["point_const"] = pc
    A, B = P.route_a(arr), P.route_b(arr)
    ctx = _ctx(arr)
    try:
        G = ctx.point_covariance([k, j])
        assert (G[1] == 0).all()
        assert P.rel_blocks(G[:1], A[k:k + 1])[0] <= P.tolerance(P.eps_ref(A, B))
        assert (ctx.point_covariance([j]) == 0).all()          # nothing but constant points selected
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["level40", "ring12"])
def test_point_seen_by_constant_cameras_only(lib, name):
    """LBA-shaped: every camera that observes the point is constant, so its block is inv(E^T E) of the oracle Jacobian."""
    base, _, _ = _yard(name)
    j = int(P.observed_points(base)[40])
    arr = P.lba_shaped(base, j)
    A, B = P.route_a(arr), P.route_b(arr)
    eps = P.eps_ref(A, B)
    want = P.point_hinv(arr, j)
    others = P.observed_points(arr)[:30]
    others = others[others != j]
    ctx = _ctx(arr)
    try:
        G = ctx.point_covariance([j])
        Gm = ctx.point_covariance(np.concatenate([others, [j]]))
    finally:
        ctx.close()
    rel = P.rel_blocks(G, want[None])[0]
    print(f"{name}: point {j} under constant cameras: rel {rel:.3e} against inv(E^T E), eps_ref {eps:.3e}")
    assert rel <= P.tolerance(eps)
    assert (Gm[-1] == G[0]).all()
    assert (P.rel_blocks(Gm[:-1], A[others]) <= P.tolerance(eps)).all()


@pytest.mark.gpu
def test_unobserved_point_is_singular(lib):
    arr, _, _ = _yard("ring12")
    ext = dict(arr)
    j = arr["points"].shape[0]
    ext["points"] = np.concatenate([arr["points"], arr["points"][:1] + 0.1])
    ext["point_const"] = np.concatenate([arr["point_const"], np.zeros(1, np.uint8)])
    ctx = _ctx(ext)
    try:
        rc, cov = _raw(ctx, [3, j])
        assert rc == -8 and (cov == 7.0).all()
        with pytest.raises(RuntimeError, match="ESINGULAR"):
            ctx.point_covariance([j])
        G = ctx.point_covariance([3])          # the others are unaffected by a point that is not in the program
    finally:
        ctx.close()
    ctx = _ctx(arr)
    try:
        assert (ctx.point_covariance([3]) == G).all()
    finally:
        ctx.close()


@pytest.mark.gpu
def test_singular_track_anywhere_is_an_error(lib, capfd):
    """A free point with one observation anywhere in the problem (not selected): ESINGULAR, cov untouched, the point named on stderr."""
    arr, _, _ = _yard("ring12")
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
        rc, cov = _raw(ctx, [4])
        assert rc == -8 and (cov == 7.0).all()
        err = capfd.readouterr().err
        assert "1 free point" in err and f"caller point {j}" in err, err
        rc, cov = _raw(ctx, [j])
        assert rc == -8 and (cov == 7.0).all()
    finally:
        ctx.close()
    # held constant, the same point is harmless and has a zero block
    ext["point_const"] = ext["point_const"].copy()
    ext["point_const"][j] = 1
    ctx = _ctx(ext)
    try:
        G = ctx.point_covariance([4, j])
    finally:
        ctx.close()
    A, B = P.route_a(ext), P.route_b(ext)
    assert (G[1] == 0).all()
    assert P.rel_blocks(G[:1], A[4:5])[0] <= P.tolerance(P.eps_ref(A, B))


@pytest.mark.gpu
def test_argument_errors(lib):
    arr, _, _ = _yard("ring12")
    n = arr["points"].shape[0]
    ctx = _ctx(arr)
    try:
        for bad in ([n], [-1], [2, 5, 2]):
            with pytest.raises(RuntimeError, match="EINVAL"):
                ctx.point_covariance(bad)
        cov = np.full((2, 3, 3), 7.0)
        sel = np.array([1, 2], np.int32)
        ip, dp = sel.ctypes.data_as(C.POINTER(C.c_int32)), cov.ctypes.data_as(C.POINTER(C.c_double))
        f = ctx.lib.xrsfm_ba_point_covariance
        assert f(ctx._h, 5.99, -1, ip, dp) == -1
        assert f(ctx._h, 5.99, 2, None, dp) == -1
        assert f(ctx._h, 5.99, 2, ip, None) == -1
        assert f(ctx._h, 5.99, 0, ip, dp) == 0
        assert f(ctx._h, 5.99, 0, None, None) == 0
        assert (cov == 7.0).all()
        # a context with the test transport attached counts as multi-rank
        ctx.comm_hook(1, 0, lambda buf, op: None)
        with pytest.raises(RuntimeError, match="EINVAL"):
            ctx.point_covariance([1])
    finally:
        ctx.close()
    b9 = _ctx(H.make_bal9(12, 300, 4, seed=5))
    try:
        with pytest.raises(RuntimeError, match="EINVAL"):
            b9.point_covariance([1])
    finally:
        b9.close()
    # a track observed twice by one camera
    dup = dict(arr)
    dup["obs_cam"] = np.concatenate([arr["obs_cam"], arr["obs_cam"][:1]])
    dup["obs_pt"] = np.concatenate([arr["obs_pt"], arr["obs_pt"][:1]])
    dup["obs_uv"] = np.concatenate([arr["obs_uv"], arr["obs_uv"][:1] + 0.5])
    ctx = _ctx(dup)
    try:
        with pytest.raises(RuntimeError, match="EINVAL"):
            ctx.point_covariance([1])
    finally:
        ctx.close()


@pytest.mark.gpu
def test_side_effect_free(lib):
    from xrsfm_amd import capi
    arr, A, eps = _yard("level40")
    sel = P.observed_points(arr)

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
        G0 = ctx.point_covariance(sel)
        s1 = ctx.run(capi.default_options(linear_solver=capi.SOLVER_CHOLESKY))
        got = ctx.download()
        assert summary(s1) == summary(s0)
        for a, b in zip(got, ref):
            assert (a == b).all()
        # after the run: the refined state
        G1 = ctx.point_covariance(sel)
        assert (G1 != G0).any()
        state = dict(arr)
        state["cam_q"], state["cam_t"], state["points"] = got
        A1, B1 = P.route_a(state), P.route_b(state)
        eps1 = P.eps_ref(A1, B1)
        rel = P.rel_blocks(G1, A1[sel])
        print(f"after run: point eps_ref {eps1:.3e}, GPU max rel {rel.max():.3e}; before: {P.rel_blocks(G0, A[sel]).max():.3e} (eps_ref {eps:.3e})")
        assert (rel <= P.tolerance(eps1)).all(), (float(rel.max()), eps1)
        # the camera call of the same context is not disturbed by a point call either (one shared front half)
        Gc = ctx.covariance([5, 17, 33])
        ctx.point_covariance(sel[:30])
        assert (ctx.covariance([5, 17, 33]) == Gc).all()
        # ... and a second run from the restored state is the first one again
        ctx.reset()
        ctx.point_covariance(sel[:30])
        s2 = ctx.run(capi.default_options(linear_solver=capi.SOLVER_CHOLESKY))
        assert summary(s2) == summary(s0)
        for a, b in zip(ctx.download(), ref):
            assert (a == b).all()
    finally:
        ctx.close()


def _at_size(arr, sel, want_packed):
    """finite, exactly symmetric, positive definite, equal within 1e-8 relative to the fallback on the same context and not
    bit-equal to it (the bounds of the camera test at size)."""
    from xrsfm_amd import capi
    arr = Y.fix_gauge(arr)
    plan = capi.debug_chol_plan(H.to_product(arr))
    assert plan["level_schedule"] == 1 and plan["facts"]["packed"] == want_packed, plan["facts"]
    ctx = _ctx(arr)
    try:
        G = ctx.point_covariance(sel)
        os.environ["XRSFM_BA_COV_FALLBACK"] = "1"          # (read per call)
        try:
            F = ctx.point_covariance(sel)
        finally:
            del os.environ["XRSFM_BA_COV_FALLBACK"]
        G2 = ctx.point_covariance(sel)
    finally:
        ctx.close()
    assert np.isfinite(G).all() and (G2 == G).all()
    for g in G:
        assert (g == g.T).all()
        assert np.linalg.eigvalsh(g).min() > 0
    rel = P.rel_blocks(F, G)
    print(f"T {plan['tiles']}, levels {plan['levels']}, packed {plan['facts']['packed']}: {len(sel)} points, kernel vs fallback max rel {rel.max():.3e}")
    assert (F != G).any()
    assert (rel <= 1e-8).all(), float(rel.max())


def _spread(arr, m):
    """m observed points whose first observing cameras are spread evenly over the cameras."""
    first = np.full(arr["points"].shape[0], arr["cam_q"].shape[0], np.int64)
    np.minimum.at(first, arr["obs_pt"], arr["obs_cam"])
    n_cams = arr["cam_q"].shape[0]
    order = np.argsort(first, kind="stable")
    order = order[first[order] < n_cams]
    return order[np.linspace(0, order.shape[0] - 1, m).astype(int)].astype(np.int32)


@pytest.mark.gpu
def test_config_L_21_points(lib):
    from xrsfm_amd import synth
    d = synth.make_problem(**synth.CONFIGS["L"])
    arr = {k: d[k] for k in H.FIELDS}
    sel = _spread(arr, 21)
    assert np.unique(sel).shape[0] == 21
    _at_size(arr, sel, False)


@pytest.mark.gpu
def test_packed_storage_20000_cameras(lib):
    """The 20 000-camera sequential shape of the camera test (every 2000th frame constant: see there), 8 points spread over the loop."""
    arr = H.make(20000, 400000, 4, seed=13)
    cc = arr["cam_const"].copy()
    cc[::2000] |= 3
    arr["cam_const"] = cc
    sel = _spread(arr, 8)
    assert np.unique(sel).shape[0] == 8
    _at_size(arr, sel, True)
