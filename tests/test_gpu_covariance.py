"""xrsfm_ba_covariance on the GPU against a dense CPU inverse (tests/cov_yardstick.py: route A; tolerance 50 x eps_ref + 1e-12
per camera, eps_ref = disagreement of the two CPU routes on that fixture), the panel kernel against the fallback, side effects,
singular systems, argument errors, and the call at size (config L; the 20 000-camera sequential shape on packed tiles)."""
import ctypes as C
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from tests import cov_yardstick as Y
from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_YARD = {}


def _yard(name):
    """(arr, A, eps_ref) of a fixture, computed once per session."""
    if name not in _YARD:
        arr = Y.FIXTURES[name][0]()
        A, B = Y.route_a(arr), Y.route_b(arr)
        _YARD[name] = (arr, A, Y.eps_ref(A, B))
    return _YARD[name]


def _ctx(arr):
    from xrsfm_amd import capi
    return capi.Context(H.to_product(arr))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(Y.FIXTURES))
def test_against_dense_inverse(lib, name):
    arr, A, eps = _yard(name)
    want = Y.FIXTURES[name][1]
    if want is not None:
        assert Y.schedule_of(arr) == want          # asserted with xrsfm_ba_debug_chol_plan, not assumed
    n = arr["cam_q"].shape[0]
    ctx = _ctx(arr)
    try:
        G = ctx.covariance(np.arange(n))
        rel = Y.rel_blocks(G, A)
        print(f"{name}: schedule {Y.schedule_of(arr)}, eps_ref {eps:.3e}, GPU max rel {rel.max():.3e} = {rel.max() / max(eps, 1e-300):.2f} x eps_ref")
        assert np.isfinite(G).all()
        assert (rel <= Y.tolerance(eps)).all(), (name, float(rel.max()), eps)
        assert (G == np.swapaxes(G, 1, 2)).all()
        # constant blocks: exactly zero rows and columns
        cc = arr["cam_const"]
        for c in range(n):
            if cc[c] & 1:
                assert (G[c, :3, :] == 0).all() and (G[c, :, :3] == 0).all()
            if cc[c] & 2:
                assert (G[c, 3:, :] == 0).all() and (G[c, :, 3:] == 0).all()
        if name == "const_q":
            c = Y.CONST_Q_CAM
            assert (G[c, 3:, 3:] != 0).all()
            assert np.linalg.norm(G[c, 3:, 3:] - A[c, 3:, 3:]) <= Y.tolerance(eps) * np.linalg.norm(A[c, 3:, 3:])
        # a 3-camera subset in scrambled order: exactly the blocks of the all-camera call
        sub = np.array([n - 3, 2, n // 2])
        Gs = ctx.covariance(sub)
        assert (Gs == G[sub]).all()
    finally:
        ctx.close()


_CHILD = textwrap.dedent("""
    import sys, numpy as np
    sys.path.insert(0, %r)
    import torch  # noqa: F401
    from tests import cov_yardstick as Y
    from tests import helpers as H
    from xrsfm_amd import capi
    out = {}
    for name in sys.argv[2:]:
        arr = Y.FIXTURES[name][0]()
        ctx = capi.Context(H.to_product(arr))
        out[name] = ctx.covariance(np.arange(arr["cam_q"].shape[0]))
        ctx.close()
    np.savez(sys.argv[1], **out)
""")


@pytest.mark.gpu
def test_kernel_against_fallback(lib, tmp_path):
    """A/B: XRSFM_BA_COV_FALLBACK=1 in a fresh child process (6 full solves per camera with the run path's factor-and-solve)
    against the panel kernel in this process, on the fixtures the kernel serves; two calls in one process are bit-identical."""
    names = [n for n, (_, want) in Y.FIXTURES.items() if want in ("level", "single")]
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
        ctx = _ctx(arr)
        try:
            n = arr["cam_q"].shape[0]
            G1 = ctx.covariance(np.arange(n))
            G2 = ctx.covariance(np.arange(n))
        finally:
            ctx.close()
        assert (G1 == G2).all()
        rel = Y.rel_blocks(fb[name], G1)
        print(f"{name}: kernel vs fallback max rel {rel.max():.3e}, eps_ref {eps:.3e}")
        if Y.FIXTURES[name][1] == "level":
            # two different computations: the switch did switch.  (On a single tile column the two paths add the same products
            # in the same order — Linv_k^T (Linv_k e_j) against the Gram of the columns of Linv_k — and agree bit for bit.)
            assert (fb[name] != G1).any()
        assert (rel <= 50.0 * eps).all(), (name, float(rel.max()), eps)


@pytest.mark.gpu
def test_side_effect_free(lib):
    from xrsfm_amd import capi
    arr, A, eps = _yard("level40")
    n = arr["cam_q"].shape[0]

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
        G0 = ctx.covariance(np.arange(n))
        s1 = ctx.run(capi.default_options(linear_solver=capi.SOLVER_CHOLESKY))
        got = ctx.download()
        assert summary(s1) == summary(s0)
        for a, b in zip(got, ref):
            assert (a == b).all()
        # after the run: the refined state
        G1 = ctx.covariance(np.arange(n))
        assert (G1 != G0).any()
        state = dict(arr)
        state["cam_q"], state["cam_t"], state["points"] = got
        A1, B1 = Y.route_a(state), Y.route_b(state)
        eps1 = Y.eps_ref(A1, B1)
        rel = Y.rel_blocks(G1, A1)
        print(f"after run: eps_ref {eps1:.3e}, GPU max rel {rel.max():.3e}; before: {Y.rel_blocks(G0, A).max():.3e} (eps_ref {eps:.3e})")
        assert (rel <= Y.tolerance(eps1)).all(), (float(rel.max()), eps1)
        # ... and a second run from the restored state is the first one again
        ctx.reset()
        s2 = ctx.run(capi.default_options(linear_solver=capi.SOLVER_CHOLESKY))
        assert summary(s2) == summary(s0)
        for a, b in zip(ctx.download(), ref):
            assert (a == b).all()
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["level40", "panel40"])
def test_no_gauge_is_singular_or_huge(lib, name):
    arr, A, eps = _yard(name)
    n = arr["cam_q"].shape[0]
    ctx = _ctx(arr)
    try:
        fixed = ctx.covariance(np.arange(n))
    finally:
        ctx.close()
    free = dict(arr)
    free["cam_const"] = np.zeros(n, np.uint8)
    ctx = _ctx(free)
    try:
        cov = np.full((n, 6, 6), 7.0)
        sel = np.arange(n, dtype=np.int32)
        rc = ctx.lib.xrsfm_ba_covariance(ctx._h, 5.99, n, sel.ctypes.data_as(C.POINTER(C.c_int32)), cov.ctypes.data_as(C.POINTER(C.c_double)))
        assert rc in (0, -8), rc
        assert np.isfinite(cov).all()          # never NaN / Inf in cov, whatever the code
        if rc == 0:
            big = max(np.linalg.eigvalsh(c).max() for c in cov)
            ref = max(np.linalg.eigvalsh(c).max() for c in fixed)
            print(f"{name} without a gauge: finite, largest eigenvalue {big:.3e} against {ref:.3e} with the gauge fixed")
            assert big > 1e6 * ref
        else:
            assert (cov == 7.0).all()          # an error code leaves the caller's array untouched
            print(f"{name} without a gauge: XRSFM_BA_ESINGULAR")
    finally:
        ctx.close()


@pytest.mark.gpu
def test_unobserved_camera_is_singular(lib):
    arr, _, _ = _yard("ring12")
    n = arr["cam_q"].shape[0]
    ext = dict(arr)
    ext["cam_q"] = np.concatenate([arr["cam_q"], arr["cam_q"][-1:]])
    ext["cam_t"] = np.concatenate([arr["cam_t"], arr["cam_t"][-1:] + 1.0])
    ext["cam_const"] = np.concatenate([arr["cam_const"], np.zeros(1, np.uint8)])
    ext["cam_intr"] = np.concatenate([arr["cam_intr"], arr["cam_intr"][-1:]])
    ctx = _ctx(ext)
    try:
        with pytest.raises(RuntimeError, match="ESINGULAR"):
            ctx.covariance([3, n])
        G = ctx.covariance([3])          # the others are unaffected by a camera that is not in the program
        assert np.isfinite(G).all()
    finally:
        ctx.close()
    ctx = _ctx(arr)
    try:
        assert (ctx.covariance([3]) == G).all()
    finally:
        ctx.close()


@pytest.mark.gpu
def test_singular_point_block_is_an_error(lib, capfd):
    """A free point with one observation: its undamped 3x3 block has rank 2.  ESINGULAR, cov untouched, the point named on stderr."""
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
        cov = np.full((1, 6, 6), 7.0)
        sel = np.array([4], np.int32)
        rc = ctx.lib.xrsfm_ba_covariance(ctx._h, 5.99, 1, sel.ctypes.data_as(C.POINTER(C.c_int32)), cov.ctypes.data_as(C.POINTER(C.c_double)))
        assert rc == -8 and (cov == 7.0).all()
        err = capfd.readouterr().err
        assert "1 free point" in err and f"caller point {j}" in err, err
        # held constant, the same point is harmless
        ext["point_const"][j] = 1
    finally:
        ctx.close()
    ctx = _ctx(ext)
    try:
        G = ctx.covariance([4])
    finally:
        ctx.close()
    A, B = Y.route_a(ext), Y.route_b(ext)          # (its observation still constrains the camera: the yardstick of THIS problem)
    assert Y.rel_blocks(G, A[4:5]).max() <= Y.tolerance(Y.eps_ref(A, B))


@pytest.mark.gpu
def test_argument_errors(lib):
    arr, _, _ = _yard("ring12")
    n = arr["cam_q"].shape[0]
    ctx = _ctx(arr)
    try:
        for bad in ([n], [-1], [2, 5, 2]):
            with pytest.raises(RuntimeError, match="EINVAL"):
                ctx.covariance(bad)
        cov = np.full((2, 6, 6), 7.0)
        sel = np.array([1, 2], np.int32)
        ip, dp = sel.ctypes.data_as(C.POINTER(C.c_int32)), cov.ctypes.data_as(C.POINTER(C.c_double))
        assert ctx.lib.xrsfm_ba_covariance(ctx._h, 5.99, -1, ip, dp) == -1
        assert ctx.lib.xrsfm_ba_covariance(ctx._h, 5.99, 0, ip, dp) == 0
        assert ctx.lib.xrsfm_ba_covariance(ctx._h, 5.99, 0, None, None) == 0
        assert (cov == 7.0).all()
        # a context with the test transport attached counts as multi-rank
        ctx.comm_hook(1, 0, lambda buf, op: None)
        with pytest.raises(RuntimeError, match="EINVAL"):
            ctx.covariance([1])
    finally:
        ctx.close()
    b9 = _ctx(H.make_bal9(12, 300, 4, seed=5))
    try:
        with pytest.raises(RuntimeError, match="EINVAL"):
            b9.covariance([1])
    finally:
        b9.close()


def _at_size(arr, sel, want_packed):
    """finite, symmetric to 1e-14 relative, positive definite, equal within 1e-8 relative to the fallback on the same context."""
    from xrsfm_amd import capi
    arr = Y.fix_gauge(arr)
    plan = capi.debug_chol_plan(H.to_product(arr))
    assert plan["level_schedule"] == 1 and plan["facts"]["packed"] == want_packed, plan["facts"]
    ctx = _ctx(arr)
    try:
        G = ctx.covariance(sel)
        os.environ["XRSFM_BA_COV_FALLBACK"] = "1"          # (read per call)
        try:
            F = ctx.covariance(sel)
        finally:
            del os.environ["XRSFM_BA_COV_FALLBACK"]
        G2 = ctx.covariance(sel)
    finally:
        ctx.close()
    assert np.isfinite(G).all() and (G2 == G).all()
    for g in G:
        assert np.abs(g - g.T).max() <= 1e-14 * np.abs(g).max()
        assert np.linalg.eigvalsh(g).min() > 0
    rel = Y.rel_blocks(F, G)
    print(f"T {plan['tiles']}, levels {plan['levels']}, packed {plan['facts']['packed']}: kernel vs fallback max rel {rel.max():.3e}")
    assert (F != G).any()
    assert (rel <= 1e-8).all(), float(rel.max())


@pytest.mark.gpu
def test_config_L_ten_cameras(lib):
    from xrsfm_amd import synth
    d = synth.make_problem(**synth.CONFIGS["L"])
    arr = {k: d[k] for k in H.FIELDS}
    _at_size(arr, np.array([999, 5, 250, 251, 252, 500, 617, 733, 734, 2]), False)


@pytest.mark.gpu
def test_packed_storage_20000_cameras(lib):
    """The 20 000-camera sequential shape of tools/big_sequential_check.py (fewer points per camera: the tile pattern, not the
    track count, is what this exercises): the factor's non-zero tiles are stored packed.
    Gauge: with only the reference's two constant frames a 20 000-frame loop is a chain whose drift variance grows with the cube
    of its length (measured: largest covariance entry 5.3e3 at 1000 cameras, 1.4e6 at 5000), the undamped S is no longer
    positive definite in float64 and the call returns XRSFM_BA_ESINGULAR (asserted below: never NaN, never a crash) — the run
    path's own solve of the same system at radius 1e300 is not finite either.  So every 2000th frame is held constant as well,
    like a map with absolute anchors; the storage and the schedule are the same."""
    from xrsfm_amd import capi
    arr = H.make(20000, 400000, 4, seed=13)
    loose = Y.fix_gauge(arr)
    ctx = _ctx(loose)
    try:
        sel = np.array([19999, 3, 10000, 10001], np.int32)
        cov = np.full((4, 6, 6), 7.0)
        rc = ctx.lib.xrsfm_ba_covariance(ctx._h, 5.99, 4, sel.ctypes.data_as(C.POINTER(C.c_int32)), cov.ctypes.data_as(C.POINTER(C.c_double)))
        assert rc in (0, capi.ESINGULAR) and np.isfinite(cov).all()
        if rc != 0:
            assert (cov == 7.0).all()
        print(f"two-frame gauge only: rc {rc}")
    finally:
        ctx.close()
    cc = arr["cam_const"].copy()
    cc[::2000] |= 3
    arr["cam_const"] = cc
    _at_size(arr, np.array([19999, 3, 10001, 10002]), True)          # (free cameras: 10000 is an anchor)
