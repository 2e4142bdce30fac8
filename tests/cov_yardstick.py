"""Yardstick and fixtures of the camera covariance tests (tests/test_cov_cpu.py, tests/test_gpu_covariance.py).

The yardstick is a dense CPU inverse, never the library: the full robustified Jacobian J from the oracle's linearisation
(oracle/ba_oracle.py, imported), the columns of constant blocks dropped, J^T J in float64 and the camera blocks of its inverse
(route A).  Route B computes the same blocks by the Schur complement onto the cameras.  Their disagreement eps_ref measures the
conditioning of a fixture; the library has to stay within 50 x eps_ref + 1e-12 of route A per camera (relative Frobenius norm)."""
import numpy as np

from oracle import ba_oracle as bo
from tests import helpers as H

HUBER_A = 5.99


def fix_gauge(arr):
    """The gauge as the reference's GBA fixes it: first frame constant, second frame's translation constant."""
    out = dict(arr)
    cc = np.array(arr["cam_const"], np.uint8, copy=True)
    cc[0] |= 3
    cc[1] |= 2
    out["cam_const"] = cc
    return out


def _ring12():
    return fix_gauge(H.make(12, 300, 4, seed=7))


def _ring10():
    return fix_gauge(H.make(10, 300, 4, seed=8))


def _level40():
    """40 cameras the plan puts on a level schedule (4 tile columns, 2 levels), well conditioned: three groups of 10 cameras that
    share tracks only with a fourth group of 10 (the separator, eliminated last), all looking at one scene (helpers.make_tracks).
    (The 40-camera SEQUENTIAL rings that reach a level schedule (k_obs 2 or 3) have eps_ref between 2e-9 and 5e-8 depending on the
    seed and the BLAS: too close to the 1e-8 floor to be a fixture.  Deeper level schedules are checked against the fallback at
    size: 5 levels at 1000 cameras, 8 at 20 000.)"""
    rng = np.random.default_rng(1)
    leaves, per, sep = 3, 10, 10
    tracks = []
    for l in range(leaves):
        base = l * per
        for _ in range(150):
            tracks.append(np.sort(rng.choice(per, 3, replace=False) + base))
        for _ in range(60):
            a = rng.choice(per, 2, replace=False) + base
            b = rng.choice(sep, 2, replace=False) + leaves * per
            tracks.append(np.sort(np.concatenate([a, b])))
    return fix_gauge(H.make_tracks(leaves * per + sep, tracks, seed=3))


def _panel40():
    return fix_gauge(H.make(40, 800, 5, seed=22, mode="unordered"))


def _ragged_models():
    return fix_gauge(H.with_models(H.make(30, 700, 8, seed=23, min_tri_angle_deg=0.5, dropout=0.35), seed=3))


def _const_q():
    arr = _level40()
    cc = arr["cam_const"].copy()
    cc[17] |= 1          # rotation of camera 17 constant, its translation free
    arr["cam_const"] = cc
    return arr


CONST_Q_CAM = 17
# name -> (factory, schedule the plan must put it on: "level" = xrsfm_ba_debug_chol_plan stats[6] bit 0 set, "panel" = clear with
# more than one tile column, "single" = one tile column, None = not asserted)
FIXTURES = {
    "ring12": (_ring12, "panel"),           # (10 cameras fill a tile column: 12 cameras are two columns, two levels: a panel schedule)
    "ring10": (_ring10, "single"),
    "level40": (_level40, "level"),
    "panel40": (_panel40, "panel"),
    "ragged_models": (_ragged_models, None),
    "const_q": (_const_q, "level"),
}


def schedule_of(arr):
    from xrsfm_amd import capi
    plan = capi.debug_chol_plan(H.to_product(arr))
    if plan["tiles"] == 1:
        return "single"
    return "level" if plan["level_schedule"] else "panel"


def _jacobian(arr, huber_a=HUBER_A):
    """Robustified Jacobian blocks of the oracle at the state of `arr`: Fc [n_obs][2][6], Ep [n_obs][2][3] (columns of constant
    blocks are zero), observation indices."""
    pr = H.to_oracle(arr)
    _, _, Fc, Ep = bo.evaluate(pr, pr.cam_q, pr.cam_t, pr.points, a=huber_a)
    return pr, Fc, Ep


def _free_masks(pr, Ep):
    n_cams, n_pts = pr.cam_q.shape[0], pr.points.shape[0]
    cam_free = np.ones((n_cams, 6), bool)
    cam_free[(pr.cam_const & 1) != 0, 0:3] = False
    cam_free[(pr.cam_const & 2) != 0, 3:6] = False
    pt_free = np.zeros(n_pts, bool)
    pt_free[np.unique(pr.obs_pt)] = True
    pt_free &= pr.point_const == 0
    return cam_free, pt_free


def _expand(blocks_free, cam_free):
    """[free dofs of all cameras]^2 inverse -> [n_cams][6][6] with zero rows / columns on constant dofs."""
    n_cams = cam_free.shape[0]
    idx = -np.ones((n_cams, 6), int)
    idx[cam_free] = np.arange(int(cam_free.sum()))
    out = np.zeros((n_cams, 6, 6))
    for c in range(n_cams):
        f = np.nonzero(cam_free[c])[0]
        if f.size:
            ii = idx[c, f]
            out[c][np.ix_(f, f)] = blocks_free[np.ix_(ii, ii)]
    return out


def route_a(arr, huber_a=HUBER_A):
    """Camera blocks of (J^T J)^-1 over ALL free parameters (cameras and points), dense."""
    import scipy.sparse as sp          # (J itself stays sparse: 10 000 x 5 000 dense would be 0.4 GB; only J^T J is formed dense)
    pr, Fc, Ep = _jacobian(arr, huber_a)
    cam_free, pt_free = _free_masks(pr, Ep)
    n_obs, n_cams, n_pts = Fc.shape[0], cam_free.shape[0], pt_free.shape[0]
    ccol = -np.ones((n_cams, 6), int)
    ccol[cam_free] = np.arange(int(cam_free.sum()))
    n_c = int(cam_free.sum())
    pcol = -np.ones(n_pts, int)
    pcol[pt_free] = n_c + 3 * np.arange(int(pt_free.sum()))
    rows, cols, vals = [], [], []
    for r in range(2):
        for a in range(6):
            col = ccol[pr.obs_cam, a]
            ok = col >= 0
            rows.append(2 * np.nonzero(ok)[0] + r); cols.append(col[ok]); vals.append(Fc[ok, r, a])
        for a in range(3):
            col = pcol[pr.obs_pt]
            ok = col >= 0
            rows.append(2 * np.nonzero(ok)[0] + r); cols.append(col[ok] + a); vals.append(Ep[ok, r, a])
    n = n_c + 3 * int(pt_free.sum())
    J = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(2 * n_obs, n))
    JTJ = (J.T @ J).toarray()
    inv = np.linalg.inv(JTJ)
    return _expand(inv[:n_c, :n_c], cam_free)


def route_b(arr, huber_a=HUBER_A):
    """The same blocks by the Schur complement onto the cameras: inv(Hcc - W Hpp^-1 W^T) on the free camera dofs."""
    pr, Fc, Ep = _jacobian(arr, huber_a)
    cam_free, pt_free = _free_masks(pr, Ep)
    n_cams, n_pts = cam_free.shape[0], pt_free.shape[0]
    ci, pi = pr.obs_cam, pr.obs_pt
    keep = pt_free[pi]
    Hpp = np.zeros((n_pts, 3, 3))
    np.add.at(Hpp, pi[keep], np.einsum("nri,nrj->nij", Ep[keep], Ep[keep]))
    Hinv = np.zeros_like(Hpp)
    Hinv[pt_free] = np.linalg.inv(Hpp[pt_free])
    S = np.zeros((6 * n_cams, 6 * n_cams))
    FtF = np.einsum("nri,nrj->nij", Fc, Fc)
    for o in range(Fc.shape[0]):
        c = ci[o]
        S[6 * c:6 * c + 6, 6 * c:6 * c + 6] += FtF[o]
    W = np.einsum("nri,nrj->nij", Fc, Ep)            # [n_obs][6][3]
    order = np.argsort(pi, kind="stable")
    ptr = np.searchsorted(pi[order], np.arange(n_pts + 1))
    for j in np.nonzero(pt_free)[0]:
        ids = order[ptr[j]:ptr[j + 1]]
        Wj = W[ids]
        WH = np.einsum("aij,jk->aik", Wj, Hinv[j])
        blk = np.einsum("aik,bjk->aibj", WH, Wj)
        for x, ca in enumerate(ci[ids]):
            for y, cb in enumerate(ci[ids]):
                S[6 * ca:6 * ca + 6, 6 * cb:6 * cb + 6] -= blk[x, :, y, :]
    f = cam_free.reshape(-1)
    inv = np.linalg.inv(S[np.ix_(f, f)])
    return _expand(inv, cam_free)


def rel_blocks(G, A):
    """Per camera ||G_c - A_c||_F / ||A_c||_F (0 where A_c is all zero and G_c too)."""
    num = np.sqrt(((G - A) ** 2).sum(axis=(1, 2)))
    den = np.sqrt((A ** 2).sum(axis=(1, 2)))
    out = np.zeros_like(num)
    nz = den > 0
    out[nz] = num[nz] / den[nz]
    out[~nz & (num > 0)] = np.inf
    return out


def eps_ref(A, B):
    return float(rel_blocks(B, A).max())


def tolerance(eps):
    return 50.0 * eps + 1e-12
