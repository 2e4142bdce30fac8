"""Yardstick of the point covariance tests (tests/test_cov_point_cpu.py, tests/test_gpu_point_covariance.py), on the fixtures of
the camera tests (tests/cov_yardstick.py).

Like there the yardstick is a dense CPU inverse, never the library.  Route A: the 3x3 point blocks of the dense inverse of the full
J^T J (robustified oracle Jacobian, columns of constant blocks dropped).  Route B: Hinv_p + Hinv_p W_p^T S^-1 W_p Hinv_p from the
dense Schur complement S onto the cameras.  eps_ref is their largest per-point relative Frobenius disagreement; the library has to
stay within 50 x eps_ref + 1e-12 of route A per point (cov_yardstick.tolerance).  Constant points and points without an
observation have an all-zero block in both routes."""
import numpy as np

from tests.cov_yardstick import FIXTURES, HUBER_A, _free_masks, _jacobian, eps_ref, rel_blocks, schedule_of, tolerance  # noqa: F401


def observed_points(arr):
    """The points the library can be asked about: those with an observation (the others are not part of the program)."""
    return np.unique(arr["obs_pt"]).astype(np.int32)


def route_a(arr, huber_a=HUBER_A):
    """Point blocks [n_points][3][3] of (J^T J)^-1 over ALL free parameters (cameras and points), dense."""
    import scipy.sparse as sp
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
    inv = np.linalg.inv((J.T @ J).toarray())
    out = np.zeros((n_pts, 3, 3))
    for j in np.nonzero(pt_free)[0]:
        c = pcol[j]
        out[j] = inv[c:c + 3, c:c + 3]
    return out


def route_b(arr, huber_a=HUBER_A):
    """The same blocks through the Schur complement onto the cameras: Hinv + Hinv W^T S^-1 W Hinv, S = Hcc - W Hinv W^T dense."""
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
    free_pts = np.nonzero(pt_free)[0]
    for j in free_pts:
        ids = order[ptr[j]:ptr[j + 1]]
        Wj = W[ids]
        WH = np.einsum("aij,jk->aik", Wj, Hinv[j])
        blk = np.einsum("aik,bjk->aibj", WH, Wj)
        for x, ca in enumerate(ci[ids]):
            for y, cb in enumerate(ci[ids]):
                S[6 * ca:6 * ca + 6, 6 * cb:6 * cb + 6] -= blk[x, :, y, :]
    f = cam_free.reshape(-1)
    Sinv = np.zeros_like(S)
    if f.any():
        Sinv[np.ix_(f, f)] = np.linalg.inv(S[np.ix_(f, f)])
    out = np.zeros((n_pts, 3, 3))
    for j in free_pts:
        ids = order[ptr[j]:ptr[j + 1]]
        Wp = np.zeros((6 * n_cams, 3))
        for o in ids:
            Wp[6 * ci[o]:6 * ci[o] + 6] += W[o]
        WH = Wp @ Hinv[j]
        out[j] = Hinv[j] + WH.T @ Sinv @ WH
    return out


def point_hinv(arr, j, huber_a=HUBER_A):
    """inv(sum E^T E) of point j from the oracle Jacobian: its covariance when every camera that observes it is constant."""
    pr, Fc, Ep = _jacobian(arr, huber_a)
    ids = np.nonzero(pr.obs_pt == j)[0]
    return np.linalg.inv(np.einsum("nri,nrj->ij", Ep[ids], Ep[ids]))


def lba_shaped(arr, j):
    """`arr` with every camera that observes point j held constant (a local BA around other frames): W_j = 0."""
    out = dict(arr)
    cc = np.array(arr["cam_const"], np.uint8, copy=True)
    cc[np.unique(arr["obs_cam"][arr["obs_pt"] == j])] |= 3
    out["cam_const"] = cc
    return out
