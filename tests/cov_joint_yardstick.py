"""Yardstick of the joint covariance tests (tests/test_cov_joint_cpu.py, tests/test_gpu_joint_covariance.py), on the fixtures of
the camera tests (tests/cov_yardstick.py).

Like there the yardstick is a dense CPU inverse, never the library.  Route A: inv(J^T J) over ALL free parameters (robustified
oracle Jacobian as cov_yardstick._jacobian builds it, columns of constant blocks dropped).  Route B: the same matrix assembled
from the Schur complement onto the cameras: S^-1, -S^-1 E C^-1 and C^-1 + C^-1 E^T S^-1 E C^-1 (C: the 3x3 point blocks, E: the
camera-point blocks of J^T J).  Both are expanded to the selected blocks (cameras first, 6 rows each, then points, 3 rows each)
with zeros on constant degrees of freedom.

Metric: the per-entry error |G_ij - A_ij| / sqrt(A_ii A_jj) over the free rows and columns: an error against a nearly uncorrelated
pair is measured on the scale of the two variances, not against a value near zero.  eps_ref is the largest such disagreement of
route B with route A over the FULL joint matrix of a fixture; the library has to stay within 50 x eps_ref + 1e-12
(cov_yardstick.tolerance)."""
import numpy as np

from tests.cov_yardstick import CONST_Q_CAM, FIXTURES, HUBER_A, _free_masks, _jacobian, fix_gauge, schedule_of, tolerance  # noqa: F401
from tests.cov_point_yardstick import lba_shaped, observed_points, point_hinv  # noqa: F401


class Full:
    """inv(J^T J) on the free parameters and where a caller's block sits in it: ccol [n_cams][6], pcol [n_points] (first of 3), -1 =
    constant or not in the program."""

    def __init__(self, M, ccol, pcol):
        self.M, self.ccol, self.pcol = M, ccol, pcol

    def index(self, cams, pts):
        """Position in M of every row of the selection (cameras first), -1 on constant degrees of freedom."""
        cams = np.asarray(cams, int).reshape(-1)
        pts = np.asarray(pts, int).reshape(-1)
        pc = self.pcol[pts]
        pi = np.where(pc[:, None] >= 0, pc[:, None] + np.arange(3)[None, :], -1)
        return np.concatenate([self.ccol[cams].reshape(-1), pi.reshape(-1)])

    def select(self, cams, pts):
        """The N x N sub-matrix on the selected blocks, zeros on constant degrees of freedom."""
        idx = self.index(cams, pts)
        f = idx >= 0
        out = np.zeros((idx.shape[0], idx.shape[0]))
        out[np.ix_(f, f)] = self.M[np.ix_(idx[f], idx[f])]
        return out


def _normal_matrix(arr, huber_a):
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
    return (J.T @ J).toarray(), n_c, ccol, pcol


def route_a(arr, huber_a=HUBER_A) -> Full:
    """inv(J^T J) over all free parameters, dense."""
    H, _, ccol, pcol = _normal_matrix(arr, huber_a)
    return Full(np.linalg.inv(H), ccol, pcol)


def route_b(arr, huber_a=HUBER_A) -> Full:
    """The same matrix from the Schur complement S = B - E C^-1 E^T onto the cameras (B, E, C: the blocks of J^T J)."""
    H, n_c, ccol, pcol = _normal_matrix(arr, huber_a)
    n_p = (H.shape[0] - n_c) // 3
    B, E = H[:n_c, :n_c], H[:n_c, n_c:]
    C = np.stack([H[n_c + 3 * j:n_c + 3 * j + 3, n_c + 3 * j:n_c + 3 * j + 3] for j in range(n_p)]) if n_p else np.zeros((0, 3, 3))
    Cinv = np.linalg.inv(C) if n_p else C
    ECi = np.einsum("cja,jab->cjb", E.reshape(n_c, n_p, 3), Cinv).reshape(n_c, 3 * n_p)      # E C^-1
    Sinv = np.linalg.inv(B - ECi @ E.T)
    M = np.empty_like(H)
    M[:n_c, :n_c] = Sinv
    X = Sinv @ ECi
    M[:n_c, n_c:] = -X
    M[n_c:, :n_c] = -X.T
    M[n_c:, n_c:] = ECi.T @ X
    for j in range(n_p):
        M[n_c + 3 * j:n_c + 3 * j + 3, n_c + 3 * j:n_c + 3 * j + 3] += Cinv[j]
    return Full(M, ccol, pcol)


def entry_err(G, A):
    """max |G_ij - A_ij| / sqrt(A_ii A_jj) over the free rows and columns of A (those with a positive variance)."""
    d = np.sqrt(np.clip(np.diag(A), 0.0, None))
    f = d > 0
    if not f.any():
        return 0.0
    return float((np.abs(G - A)[np.ix_(f, f)] / np.outer(d[f], d[f])).max())


def eps_ref(A: Full, B: Full):
    return entry_err(B.M, A.M)

