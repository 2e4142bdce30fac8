"""xrsfm_ba_joint_covariance on the GPU against a dense CPU inverse (tests/cov_joint_yardstick.py: route A; per-entry error on the
scale of the two variances, tolerance 50 x eps_ref + 1e-12 with eps_ref = the disagreement of the two CPU routes over the full
joint matrix of that fixture), the Gram kernel against the fallback, repeatability, special blocks, argument errors, side effects,
and the call at size (config L; the 20 000-camera sequential shape on packed tiles)."""
import ctypes as C
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from tests import cov_joint_yardstick as Jy
from tests import cov_yardstick as Y
from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 1024
_YARD = {}


def _yard(name):
    """(arr, route A, eps_ref) of a fixture, computed once per session."""
    if name not in _YARD:
        arr = Jy.FIXTURES[name][0]()
        A, B = Jy.route_a(arr), Jy.route_b(arr)
        _YARD[name] = (arr, A, Jy.eps_ref(A, B))
    return _YARD[name]


def _ctx(arr):
    from xrsfm_amd import capi
    return capi.Context(H.to_product(arr))


def _big_selection(arr):
    """All cameras and every 5th observed point, the points cut so that the selection stays under the cap."""
    cams = np.arange(arr["cam_q"].shape[0], dtype=np.int32)
    pts = Jy.observed_points(arr)[::5]
    room = (CAP - 6 * cams.shape[0]) // 3
    return cams, pts[:room], pts.shape[0] > room


def _raw(ctx, cams, pts, fill=7.0):
    cams = np.ascontiguousarray(cams, np.int32)
    pts = np.ascontiguousarray(pts, np.int32)
    N = 6 * cams.shape[0] + 3 * pts.shape[0]
    cov = np.full((max(1, N), max(1, N)), fill)
    ip = C.POINTER(C.c_int32)
    rc = ctx.lib.xrsfm_ba_joint_covariance(ctx._h, 5.99, cams.shape[0], cams.ctypes.data_as(ip), pts.shape[0], pts.ctypes.data_as(ip),
                                           cov.ctypes.data_as(C.POINTER(C.c_double)))
    return rc, cov


def _rows(n_cams_sel, cam_pos, pt_pos):
    """Rows of a joint matrix that belong to the cameras cam_pos and the points pt_pos of its selection."""
    r = [6 * i + a for i in cam_pos for a in range(6)]
    r += [6 * n_cams_sel + 3 * i + a for i in pt_pos for a in range(3)]
    return np.array(r, int)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(Jy.FIXTURES))
def test_against_dense_inverse(lib, name):
    arr, A, eps = _yard(name)
    want = Jy.FIXTURES[name][1]
    sched = Jy.schedule_of(arr)          # asserted with xrsfm_ba_debug_chol_plan, not assumed
    if want is not None:
        assert sched == want
    cams, pts, cut = _big_selection(arr)
    N = 6 * cams.shape[0] + 3 * pts.shape[0]
    assert N <= CAP and (not cut or N > CAP - 3), (name, N, cut)          # cut to the cap where the fixture is larger, and only there
    want_S = A.select(cams, pts)
    ctx = _ctx(arr)
    try:
        G = ctx.joint_covariance(cams, pts)
        err = Jy.entry_err(G, want_S)
        print(f"{name}: schedule {sched}, N {N}, joint eps_ref {eps:.3e}, GPU max entry error {err:.3e} = {err / max(eps, 1e-300):.2f} x eps_ref")
        assert np.isfinite(G).all()
        assert err <= Jy.tolerance(eps), (name, err, eps)
        assert (G == G.T).all()
        fixed = np.diag(want_S) == 0
        assert (G[fixed, :] == 0).all() and (G[:, fixed] == 0).all()
        # diagonal blocks against the two marginal calls of the same context
        Gc, Gp = ctx.covariance(cams), ctx.point_covariance(pts)
        o = 6 * cams.shape[0]
        dc = max(Jy.entry_err(G[6 * i:6 * i + 6, 6 * i:6 * i + 6], Gc[i]) for i in range(cams.shape[0]))
        dp = max(Jy.entry_err(G[o + 3 * i:o + 3 * i + 3, o + 3 * i:o + 3 * i + 3], Gp[i]) for i in range(pts.shape[0]))
        print(f"{name}: diagonal blocks against covariance {dc:.3e}, against point_covariance {dp:.3e}")
        assert dc <= 50.0 * eps and dp <= 50.0 * eps
        # a scrambled sub-selection: 3 cameras and 4 points from different chunks of the big call, as far as the fixture has them
        # (ring10 / ring12: 10 / 12 cameras are one / two camera chunks, 60 points three point chunks)
        cch, pch = _camera_chunks(arr, cams), _point_chunks(arr, pts)
        cpos = _one_per_chunk(cch, 3)
        ppos = _one_per_chunk(pch, 4)
        cpos, ppos = [cpos[1], cpos[2], cpos[0]], [ppos[2], ppos[0], ppos[3], ppos[1]]
        assert len(set(cpos)) == 3 and len(set(ppos)) == 4
        assert len({int(cch[i]) for i in cpos}) == min(3, int(cch.max()) + 1) and len({int(pch[i]) for i in ppos}) == min(4, int(pch.max()) + 1)
        if name in ("level40", "const_q"):
            assert len({int(cch[i]) for i in cpos}) == 3 and len({int(pch[i]) for i in ppos}) == 4
        Gs = ctx.joint_covariance(cams[cpos], pts[ppos])
        rows = _rows(cams.shape[0], cpos, ppos)
        sub = G[np.ix_(rows, rows)]
        if sched in ("level", "single"):
            assert (Gs == sub).all()
        else:
            assert Jy.entry_err(Gs, A.select(cams[cpos], pts[ppos])) <= Jy.tolerance(eps)
            assert Jy.entry_err(Gs, sub) <= 50.0 * eps
    finally:
        ctx.close()


def _camera_chunks(arr, cams):
    """Chunk of every camera of `cams` on the kernel path: 10 per chunk in elimination order (xrsfm_ba_debug_chol_plan)."""
    from xrsfm_amd import capi
    off = np.asarray(capi.debug_chol_plan(H.to_product(arr))["cam_offset"])[cams]
    ch = np.empty(len(cams), int)
    ch[np.argsort(off, kind="stable")] = np.arange(len(cams)) // 10
    return ch


def _point_chunks(arr, pts):
    """Chunk of every (free) point of `pts` on the kernel path: ordered by the first tile column of the observing cameras, then by
    packed index, 21 per chunk.  The packed index ascends with a point's first slot of the track-major packing (xrsfm_ba_debug_pack)."""
    from xrsfm_amd import capi
    prod = H.to_product(arr)
    col = np.asarray(capi.debug_chol_plan(prod)["cam_offset"]) // 64
    kmin = np.full(arr["points"].shape[0], 1 << 30)
    np.minimum.at(kmin, arr["obs_pt"], col[arr["obs_cam"]])
    so = capi.debug_pack(prod)["slot_obs"]
    first = np.full(arr["points"].shape[0], 1 << 30)
    ok = so >= 0
    np.minimum.at(first, arr["obs_pt"][so[ok]], np.nonzero(ok)[0])
    ch = np.empty(len(pts), int)
    ch[np.lexsort((first[pts], kmin[pts]))] = np.arange(len(pts)) // 21
    return ch


def _one_per_chunk(chunk, m):
    """m positions spread over the chunks, one per chunk while there are chunks left, each from the middle of its chunk (so that its
    chunk does not hinge on a tie at a chunk boundary)."""
    ids = np.unique(chunk)
    take = ids[np.linspace(0, ids.shape[0] - 1, min(m, ids.shape[0])).astype(int)]
    out = []
    for c in take:
        members = np.nonzero(chunk == c)[0]
        out.append(int(members[members.shape[0] // 2]))
    spare = [i for i in range(chunk.shape[0]) if i not in out]
    return out + spare[:m - len(out)]


_CHILD = textwrap.dedent("""
    import sys, numpy as np
    sys.path.insert(0, %r)
    import torch  # noqa: F401
    from tests import cov_joint_yardstick as Jy
    from tests import helpers as H
    from xrsfm_amd import capi
    out = {}
    for name in sys.argv[2:]:
        arr = Jy.FIXTURES[name][0]()
        ctx = capi.Context(H.to_product(arr))
        out[name] = ctx.joint_covariance(np.arange(arr["cam_q"].shape[0])[::3], Jy.observed_points(arr)[::29])
        ctx.close()
    np.savez(sys.argv[1], **out)
""")


@pytest.mark.gpu
def test_kernel_against_fallback(lib, tmp_path):
    """A/B: XRSFM_BA_COV_FALLBACK=1 in a fresh child process (one full factor-and-solve per selected column; every 3rd camera and
    every 29th point of a fixture) against the Gram kernel in this process, on the fixtures the kernel serves."""
    names = [n for n, (_, want) in Jy.FIXTURES.items() if want in ("level", "single")]
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
        cams, pts = np.arange(arr["cam_q"].shape[0])[::3], Jy.observed_points(arr)[::29]
        ctx = _ctx(arr)
        try:
            G = ctx.joint_covariance(cams, pts)
        finally:
            ctx.close()
        F = fb[name]
        err = Jy.entry_err(F, G)
        print(f"{name}: N {G.shape[0]}, kernel vs fallback max entry error {err:.3e}, joint eps_ref {eps:.3e}")
        if name == "level40":
            assert (F != G).any()          # two different computations: the switch did switch
        assert (F == F.T).all()
        assert err <= 50.0 * eps, (name, err, eps)
        want = A.select(cams, pts)
        assert Jy.entry_err(F, want) <= Jy.tolerance(eps) and Jy.entry_err(G, want) <= Jy.tolerance(eps)


_FB_SEL = {"const_q": [5, 17, 33], "ring12": [2, 7, 11]}          # (const_q: level plan, camera 17 rotation-constant; ring12: panel plan)
_FB_CHILD = textwrap.dedent("""
    import sys, numpy as np
    sys.path.insert(0, %r)
    import torch  # noqa: F401
    from tests import cov_joint_yardstick as Jy
    from tests import helpers as H
    from xrsfm_amd import capi
    out = {}
    for spec in sys.argv[2:]:
        name, cams = spec.split(":")[0], [int(v) for v in spec.split(":")[1].split(",")]
        arr = dict(Jy.FIXTURES[name][0]())
        pts = Jy.observed_points(arr)[[8, 100, 250]]
        pc = np.array(arr["point_const"], np.uint8, copy=True)
        pc[pts[1]] = 1
        arr["point_const"] = pc
        ctx = capi.Context(H.to_product(arr))
        out[name + "_joint"] = ctx.joint_covariance(cams, pts)
        out[name + "_cams"] = ctx.covariance(cams)
        out[name + "_pts"] = ctx.point_covariance(pts)
        ctx.close()
    np.savez(sys.argv[1], **out)
""")


@pytest.mark.gpu
def test_fallback_marginals_are_joint_diagonal_blocks(lib, tmp_path):
    """With XRSFM_BA_COV_FALLBACK=1 (a fresh child process) the three calls share one solver: the 6x6 and 3x3 diagonal blocks of the
    joint matrix are the blocks of the two marginal calls bit for bit (the same right-hand sides reach the same factor-and-solve and
    the sums run in the same order).  3 cameras and 3 observed points, the second point constant."""
    assert Jy.FIXTURES["ring12"][1] == "panel" and Jy.FIXTURES["const_q"][1] == "level" and Jy.CONST_Q_CAM in _FB_SEL["const_q"]
    env = dict(os.environ)
    env["XRSFM_BA_COV_FALLBACK"] = "1"
    out = str(tmp_path / "fallback_blocks.npz")
    specs = [f"{name}:{','.join(str(v) for v in cams)}" for name, cams in _FB_SEL.items()]
    r = subprocess.run([sys.executable, "-c", _FB_CHILD % ROOT, out] + specs, capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    fb = np.load(out)
    for name in _FB_SEL:
        G, Gc, Gp = fb[name + "_joint"], fb[name + "_cams"], fb[name + "_pts"]
        assert G.shape == (27, 27) and Gc.shape == (3, 6, 6) and Gp.shape == (3, 3, 3) and np.isfinite(G).all()
        for i in range(3):
            assert (G[6 * i:6 * i + 6, 6 * i:6 * i + 6] == Gc[i]).all(), (name, "camera", i)
            assert (G[18 + 3 * i:21 + 3 * i, 18 + 3 * i:21 + 3 * i] == Gp[i]).all(), (name, "point", i)
        assert (Gp[1] == 0).all() and (Gp[0] != 0).all() and (Gp[2] != 0).all() and (np.diagonal(Gc, axis1=1, axis2=2)[[0, 2]] > 0).all()
        if name == "const_q":
            assert (Gc[1][:3] == 0).all() and (Gc[1][3:, 3:] != 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["level40", "ring12"])
def test_repeatable(lib, name):
    """Two calls are bit-identical (kernel path and fallback path), and a permutation of cam_sel and pt_sel permutes rows and
    columns exactly."""
    arr, _, _ = _yard(name)
    cams = np.arange(arr["cam_q"].shape[0], dtype=np.int32)[:: (1 if name == "level40" else 4)]
    pts = Jy.observed_points(arr)[:: (9 if name == "level40" else 60)]
    ctx = _ctx(arr)
    try:
        G1 = ctx.joint_covariance(cams, pts)
        G2 = ctx.joint_covariance(cams, pts)
        rng = np.random.default_rng(0)
        pc, pp = rng.permutation(cams.shape[0]), rng.permutation(pts.shape[0])
        G3 = ctx.joint_covariance(cams[pc], pts[pp])
    finally:
        ctx.close()
    assert (G1 == G2).all()
    rows = _rows(cams.shape[0], pc, pp)
    assert (G3 == G1[np.ix_(rows, rows)]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["level40", "ring12"])
def test_constant_point_has_zero_rows_and_columns(lib, name):
    base, _, _ = _yard(name)
    arr = dict(base)
    obs = Jy.observed_points(base)
    j, k = int(obs[5]), int(obs[6])
    pc = np.array(base["point_const"], np.uint8, copy=True)
    pc[j] = 1
    arr["point_const"] = pc
    A, B = Jy.route_a(arr), Jy.route_b(arr)
    eps = Jy.eps_ref(A, B)
    cams, pts = [4, 9], [k, j, int(obs[50])]
    ctx = _ctx(arr)
    try:
        G = ctx.joint_covariance(cams, pts)
        Gj = ctx.joint_covariance([], [j])          # nothing but a constant point selected
    finally:
        ctx.close()
    assert (G[15:18, :] == 0).all() and (G[:, 15:18] == 0).all() and (Gj == 0).all()
    assert Jy.entry_err(G, A.select(cams, pts)) <= Jy.tolerance(eps)
    keep = np.r_[0:15, 18:21]
    assert (G[np.ix_(keep, keep)] != 0).all()


@pytest.mark.gpu
def test_const_q_camera(lib):
    """const_q's camera 17: zero rotation rows and columns, translation cross blocks as the dense inverse has them."""
    arr, A, eps = _yard("const_q")
    c = Jy.CONST_Q_CAM
    cams, pts = [5, c, 33], Jy.observed_points(arr)[[3, 300, 600]]
    want = A.select(cams, pts)
    ctx = _ctx(arr)
    try:
        G = ctx.joint_covariance(cams, pts)
    finally:
        ctx.close()
    assert (G[6:9, :] == 0).all() and (G[:, 6:9] == 0).all()
    assert (G[9:12, :6] != 0).all() and (G[9:12, 12:] != 0).all()
    assert Jy.entry_err(G, want) <= Jy.tolerance(eps)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["level40", "ring12"])
def test_point_seen_by_constant_cameras_only(lib, name):
    """LBA-shaped: every camera that observes the point is constant: exactly zero cross blocks, the diagonal block inv(E^T E)."""
    base, _, _ = _yard(name)
    j = int(Jy.observed_points(base)[40])
    arr = Jy.lba_shaped(base, j)
    A, B = Jy.route_a(arr), Jy.route_b(arr)
    eps = Jy.eps_ref(A, B)
    free = np.nonzero(arr["cam_const"] == 0)[0]
    cams = free[[0, free.shape[0] // 2, -1]]
    others = Jy.observed_points(arr)[:30:7]
    others = others[others != j]
    pts = np.concatenate([others[:2], [j], others[2:]])
    ctx = _ctx(arr)
    try:
        G = ctx.joint_covariance(cams, pts)
        G1 = ctx.joint_covariance([], [j])
    finally:
        ctx.close()
    o = 18 + 3 * 2
    blk = G[o:o + 3, o:o + 3]
    rest = np.r_[0:o, o + 3:G.shape[0]]
    assert (G[o:o + 3][:, rest] == 0).all() and (G[rest][:, o:o + 3] == 0).all()
    err = Jy.entry_err(blk, Jy.point_hinv(arr, j))
    print(f"{name}: point {j} under constant cameras: entry error {err:.3e} against inv(E^T E), joint eps_ref {eps:.3e}")
    assert err <= Jy.tolerance(eps)
    assert (G1 == blk).all() or Jy.schedule_of(arr) == "panel"
    assert Jy.entry_err(G, A.select(cams, pts)) <= Jy.tolerance(eps)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["level40", "ring12"])
def test_cameras_only_and_points_only(lib, name):
    arr, A, eps = _yard(name)
    cams, pts = np.array([7, 2, 11], np.int32), Jy.observed_points(arr)[[100, 8, 250]]
    ctx = _ctx(arr)
    try:
        Gc = ctx.joint_covariance(cams, [])
        Gp = ctx.joint_covariance([], pts)
        G = ctx.joint_covariance(cams, pts)
    finally:
        ctx.close()
    assert Gc.shape == (18, 18) and Gp.shape == (9, 9)
    assert Jy.entry_err(Gc, A.select(cams, [])) <= Jy.tolerance(eps)
    assert Jy.entry_err(Gp, A.select([], pts)) <= Jy.tolerance(eps)
    if Jy.schedule_of(arr) == "level":
        assert (Gc == G[:18, :18]).all() and (Gp == G[18:, 18:]).all()


@pytest.mark.gpu
def test_unobserved_blocks_are_singular(lib):
    arr, _, _ = _yard("ring12")
    ext = dict(arr)
    j = arr["points"].shape[0]
    ext["points"] = np.concatenate([arr["points"], arr["points"][:1] + 0.1])
    ext["point_const"] = np.concatenate([arr["point_const"], np.zeros(1, np.uint8)])
    ctx = _ctx(ext)
    try:
        rc, cov = _raw(ctx, [3], [3, j])
        assert rc == -8 and (cov == 7.0).all()
        rc, cov = _raw(ctx, [], [j])
        assert rc == -8 and (cov == 7.0).all()
        with pytest.raises(RuntimeError, match="ESINGULAR"):
            ctx.joint_covariance([], [j])
    finally:
        ctx.close()
    # a camera without an observation
    n = arr["cam_q"].shape[0]
    ext = dict(arr)
    ext["cam_q"] = np.concatenate([arr["cam_q"], arr["cam_q"][-1:]])
    ext["cam_t"] = np.concatenate([arr["cam_t"], arr["cam_t"][-1:] + 1.0])
    ext["cam_const"] = np.concatenate([arr["cam_const"], np.zeros(1, np.uint8)])
    ext["cam_intr"] = np.concatenate([arr["cam_intr"], arr["cam_intr"][-1:]])
    ctx = _ctx(ext)
    try:
        rc, cov = _raw(ctx, [3, n], [3])
        assert rc == -8 and (cov == 7.0).all()
        rc, cov = _raw(ctx, [3], [3])
        assert rc == 0 and (cov != 7.0).all()
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
        rc, cov = _raw(ctx, [4], [4])
        assert rc == -8 and (cov == 7.0).all()
        err = capfd.readouterr().err
        assert "1 free point" in err and f"caller point {j}" in err, err
    finally:
        ctx.close()


@pytest.mark.gpu
def test_argument_errors(lib):
    arr, _, _ = _yard("ring12")
    n_c, n_p = arr["cam_q"].shape[0], arr["points"].shape[0]
    ctx = _ctx(arr)
    try:
        for cams, pts in (([n_c], [1]), ([-1], [1]), ([2, 5, 2], [1]), ([1], [n_p]), ([1], [-1]), ([1], [2, 5, 2])):
            rc, cov = _raw(ctx, cams, pts)
            assert rc == -1 and (cov == 7.0).all(), (cams, pts, rc)
            with pytest.raises(RuntimeError, match="EINVAL"):
                ctx.joint_covariance(cams, pts)
        ctx.joint_covariance([2], [2, 5])          # a camera and a point may share an index
        cov = np.full((15, 15), 7.0)
        cs, ps = np.array([1], np.int32), np.array([1, 2, 3], np.int32)
        ip = C.POINTER(C.c_int32)
        cp, pp, dp = cs.ctypes.data_as(ip), ps.ctypes.data_as(ip), cov.ctypes.data_as(C.POINTER(C.c_double))
        f = ctx.lib.xrsfm_ba_joint_covariance
        assert f(ctx._h, 5.99, -1, cp, 3, pp, dp) == -1
        assert f(ctx._h, 5.99, 1, cp, -1, pp, dp) == -1
        assert f(ctx._h, 5.99, 1, None, 3, pp, dp) == -1
        assert f(ctx._h, 5.99, 1, cp, 3, None, dp) == -1
        assert f(ctx._h, 5.99, 1, cp, 3, pp, None) == -1
        assert f(ctx._h, 5.99, 0, cp, 0, pp, dp) == 0
        assert f(ctx._h, 5.99, 0, None, 0, None, None) == 0
        assert (cov == 7.0).all()
        assert f(ctx._h, 5.99, 0, None, 3, pp, dp) == 0          # either count may be zero: a 9 x 9 result, the first 81 doubles
        flat = cov.reshape(-1)
        assert (flat[:81] != 7.0).all() and (flat[81:] == 7.0).all()
        assert f(ctx._h, 5.99, 1, cp, 0, None, dp) == 0 and (flat[36:81] != 7.0).all() and (flat[81:] == 7.0).all()
        # a context with the test transport attached counts as multi-rank
        ctx.comm_hook(1, 0, lambda buf, op: None)
        rc, cov = _raw(ctx, [1], [1])
        assert rc == -1 and (cov == 7.0).all()
        with pytest.raises(RuntimeError, match="EINVAL"):
            ctx.joint_covariance([1], [1])
    finally:
        ctx.close()
    b9 = _ctx(H.make_bal9(12, 300, 4, seed=5))
    try:
        rc, cov = _raw(b9, [1], [1])
        assert rc == -1 and (cov == 7.0).all()
        with pytest.raises(RuntimeError, match="EINVAL"):
            b9.joint_covariance([1], [1])
    finally:
        b9.close()
    # a track observed twice by one camera
    dup = dict(arr)
    dup["obs_cam"] = np.concatenate([arr["obs_cam"], arr["obs_cam"][:1]])
    dup["obs_pt"] = np.concatenate([arr["obs_pt"], arr["obs_pt"][:1]])
    dup["obs_uv"] = np.concatenate([arr["obs_uv"], arr["obs_uv"][:1] + 0.5])
    ctx = _ctx(dup)
    try:
        rc, cov = _raw(ctx, [1], [1])
        assert rc == -1 and (cov == 7.0).all()
    finally:
        ctx.close()


@pytest.mark.gpu
def test_cap(lib):
    """N above XRSFM_BA_JOINT_COV_MAX_COLS is EINVAL with cov untouched; the largest selection under it runs on the kernel path."""
    arr, A, eps = _yard("level40")
    cams, allp = np.arange(40), Jy.observed_points(arr)
    assert 6 * 40 + 3 * 262 == CAP + 2 and 6 * 40 + 3 * 261 == CAP - 1
    ctx = _ctx(arr)
    try:
        rc, big = _raw(ctx, cams, allp[:262])
        assert rc == -1 and (big == 7.0).all()
        rc, big = _raw(ctx, cams, allp[:261])
    finally:
        ctx.close()
    assert rc == 0 and np.isfinite(big).all() and (big == big.T).all()
    assert Jy.entry_err(big, A.select(cams, allp[:261])) <= Jy.tolerance(eps)


@pytest.mark.gpu
def test_side_effect_free(lib):
    from xrsfm_amd import capi
    arr, A, eps = _yard("level40")
    cams, pts, _ = _big_selection(arr)
    pts = pts[::4]

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
        Gc, Gp = ctx.covariance([5, 17, 33]), ctx.point_covariance(pts[:30])
        G0 = ctx.joint_covariance(cams, pts)
        # the two marginal calls of the same context are not disturbed by a joint call (one shared front half)
        assert (ctx.covariance([5, 17, 33]) == Gc).all() and (ctx.point_covariance(pts[:30]) == Gp).all()
        s1 = ctx.run(capi.default_options(linear_solver=capi.SOLVER_CHOLESKY))
        got = ctx.download()
        assert summary(s1) == summary(s0)
        for a, b in zip(got, ref):
            assert (a == b).all()
        # after the run: the refined state
        G1 = ctx.joint_covariance(cams, pts)
        assert (G1 != G0).any()
        state = dict(arr)
        state["cam_q"], state["cam_t"], state["points"] = got
        A1, B1 = Jy.route_a(state), Jy.route_b(state)
        eps1 = Jy.eps_ref(A1, B1)
        err = Jy.entry_err(G1, A1.select(cams, pts))
        print(f"after run: joint eps_ref {eps1:.3e}, GPU max entry error {err:.3e}; before: {Jy.entry_err(G0, A.select(cams, pts)):.3e} (eps_ref {eps:.3e})")
        assert err <= Jy.tolerance(eps1), (err, eps1)
        # ... and a second run from the restored state is the first one again
        ctx.reset()
        ctx.joint_covariance(cams[:7], pts[:30])
        s2 = ctx.run(capi.default_options(linear_solver=capi.SOLVER_CHOLESKY))
        assert summary(s2) == summary(s0)
        for a, b in zip(ctx.download(), ref):
            assert (a == b).all()
    finally:
        ctx.close()


def _at_size(arr, cams, pts, want_packed):
    """Level schedule asserted; finite, exactly symmetric, positive definite, within 1e-8 (per-entry error on the scale of the two
    variances: the bound of the two marginal tests at size) of the fallback on the same context, not bit-equal to it, and a second
    call bit-identical."""
    from xrsfm_amd import capi
    arr = Y.fix_gauge(arr)
    plan = capi.debug_chol_plan(H.to_product(arr))
    assert plan["level_schedule"] == 1 and plan["facts"]["packed"] == want_packed, plan["facts"]
    ctx = _ctx(arr)
    try:
        G = ctx.joint_covariance(cams, pts)
        os.environ["XRSFM_BA_COV_FALLBACK"] = "1"          # (read per call)
        try:
            F = ctx.joint_covariance(cams, pts)
        finally:
            del os.environ["XRSFM_BA_COV_FALLBACK"]
        G2 = ctx.joint_covariance(cams, pts)
    finally:
        ctx.close()
    assert np.isfinite(G).all() and (G2 == G).all() and (G == G.T).all() and (F == F.T).all()
    lam = np.linalg.eigvalsh(G)
    err = Jy.entry_err(F, G)
    print(f"T {plan['tiles']}, levels {plan['levels']}, packed {plan['facts']['packed']}: N {G.shape[0]}, kernel vs fallback max entry error {err:.3e}, "
          f"eigenvalues {lam.min():.3e} .. {lam.max():.3e}")
    assert lam.min() > 0
    assert (F != G).any()
    assert err <= 1e-8, err


def _spread(arr, m):
    """m observed points whose first observing cameras are spread evenly over the cameras."""
    first = np.full(arr["points"].shape[0], arr["cam_q"].shape[0], np.int64)
    np.minimum.at(first, arr["obs_pt"], arr["obs_cam"])
    n_cams = arr["cam_q"].shape[0]
    order = np.argsort(first, kind="stable")
    order = order[first[order] < n_cams]
    return order[np.linspace(0, order.shape[0] - 1, m).astype(int)].astype(np.int32)


@pytest.mark.gpu
def test_config_L_12_cameras_30_points(lib):
    from xrsfm_amd import synth
    d = synth.make_problem(**synth.CONFIGS["L"])
    arr = {k: d[k] for k in H.FIELDS}
    n = arr["cam_q"].shape[0]
    cams = np.linspace(2, n - 1, 12).astype(np.int32)          # spread over the ring, past the two frames of the gauge
    pts = _spread(arr, 30)
    assert np.unique(cams).shape[0] == 12 and np.unique(pts).shape[0] == 30
    _at_size(arr, cams, pts, False)


@pytest.mark.gpu
def test_packed_storage_20000_cameras(lib):
    """The 20 000-camera sequential shape of the two marginal tests (every 2000th frame constant: see there), 4 cameras and 8 points
    spread over the loop."""
    arr = H.make(20000, 400000, 4, seed=13)
    cc = arr["cam_const"].copy()
    cc[::2000] |= 3
    arr["cam_const"] = cc
    cams = np.array([1000, 7000, 13000, 19000], np.int32)
    pts = _spread(arr, 8)
    assert np.unique(pts).shape[0] == 8 and (cc[cams] == 0).all()
    _at_size(arr, cams, pts, True)
