"""Yardstick, catalogue and bars of the absolute-pose tests (tests/test_pose_cpu.py, tests/test_gpu_absolute_pose.py).

The yardstick is a pure numpy restatement of the rule xrsfm_ba_absolute_pose restates (include/xrsfm_ba.h; the reference's
SolvePnP_colmap -> colmap::LORANSAC<P3PEstimator, EPNPEstimator>), parameterised by dtype and run in np.longdouble (x87 extended,
asserted) and in np.float64.  MT19937, the Jacobi routines and the root finder are written by hand.  It is never the library and
shares no code with it.

Rule.  Every frame gets a fresh MT19937 (init_genrand(seed)); the sampler keeps an index array across the trials of the frame and
does three Fisher-Yates steps per trial (bounded draw for m = last - i + 1: s = 0xFFFFFFFF // m, draw words until x < m s,
j = i + x // s).  max_trials = min(max_num_trials, ComputeNumTrials(min_inlier_ratio 1e5, 1e5, confidence)).  Per trial: the P3P
quartic of the three sampled correspondences; its roots as complex numbers (Aberth iteration on the monic polynomial, capped); a
root is taken when |Im| <= 1e-10 and Re >= 0; one model per root in ascending Re (Umeyama without scale, sign from det U det V);
non-finite models are dropped.  Residual: squared reprojection error, DBL_MAX at depth <= DBL_EPSILON.  Support = (count, sum of
inlier residuals in index order); a beats b iff count larger, or equal and sum strictly smaller; initial best (0, DBL_MAX).  A model
that beats the best becomes the best; with count > 3 EPnP on its inliers gives a local model, which replaces it if its support
beats it; dyn = ceil(log(1 - c) / log(1 - (k / n)^3)) (1 if the argument is <= 0, unbounded if 1 - c <= 0 or k = 0) is a matter
of integers and is evaluated in float64 whatever the dtype; after every model, t >= dyn and t >= min_num_trials set abort: the rest
of the trial's models are skipped, the next trial, if the bound admits one, is counted and the scan stops.  Success iff the best
count >= 3; the mask is the inlier test of the returned model.  EPnP follows EPNPEstimator::ComputePose step by step (control
points, barycentric coordinates with the rank test at Eigen's default threshold, M^T M summed over the inliers in index order,
the four smallest eigenvectors, three beta approximations as least-squares solves, five Gauss-Newton steps each, ComputeRT, the
best of three by the sum of the square roots of the residuals); its sign step negates iff the first inlier's depth is negative.

Fragile frames.  A frame is FRAGILE when the two precisions disagree on a discrete output (status, mask, num_inliers, num_trials,
best_trial), or when any of three seeded float64 reruns with every input coordinate perturbed by a relative 2^-43 changes one.
(Equal coordinate values receive equal perturbations, so the exact degeneracies built into the catalogue stay exact.)  At most
FRAGILE_CAP of the catalogue's frames may be fragile: a condition on the catalogue, asserted in both test files.

Bars on non-fragile status-1 frames.  Gross: rotation matrix and t within rtol 1e-6 / atol 1e-9 of the extended run.  Tight:
deviation(pose, extended) <= TIGHT_BAR = TIGHT_FACTOR x RESTATEMENT_DEVIATION, the float64 restatement's own largest deviation
over the catalogue (asserted to be that in tests/test_pose_cpu.py); the factor 16 covers a different but equally valid operation
order.  deviation = max |R - R_ext| and |t - t_ext| / max(1, |t_ext|), entrywise maxima.
"""
import functools
import math

import numpy as np

EXT = np.longdouble
assert np.finfo(EXT).eps < 2e-19, "np.longdouble is not extended precision here"

DBL_EPS = 2.0 ** -52
DBL_MAX = float(np.finfo(np.float64).max)
MAX_CORR = 8192
MAX_TRIALS = 16384
LOCAL_BIT = 1 << 30
UNBOUNDED = 2 ** 31 - 1
CHUNK = 64
FRAGILE_CAP = 0.05
PERTURBATION = 2.0 ** -43
ROOT_MAX_IMAG = 1e-10
ROOT_ITERS = 100
TIGHT_FACTOR = 16
RESTATEMENT_DEVIATION = 4.0e-10  # measured: the float64 restatement against the extended run, largest over the catalogue (3.96e-10, the
                                 # planar frame, whose final model is a sample model; tests/test_pose_cpu.py asserts the measurement)
BRANCHES = ("root_rejected_imag", "root_rejected_sign", "trial_without_model", "local_wins", "local_loses", "abort_dyn", "cap_reached")


class Options:
    def __init__(self, **kw):
        self.max_error = 8.0 / 800.0
        self.confidence = 0.9999
        self.min_inlier_ratio = 0.25
        self.min_num_trials = 100
        self.max_num_trials = MAX_TRIALS
        self.seed = 0
        for k, v in kw.items():
            assert hasattr(self, k), k
            setattr(self, k, v)


def num_trials_bound(k, n, confidence):
    nom = 1.0 - confidence
    if nom <= 0.0 or k <= 0:
        return UNBOUNDED
    denom = 1.0 - (k / float(n)) ** 3
    if denom <= 0.0:
        return 1
    return min(UNBOUNDED, int(math.ceil(math.log(nom) / math.log(denom))))


def trial_cap(opt):
    return min(opt.max_num_trials, num_trials_bound(int(opt.min_inlier_ratio * 100000.0), 100000, opt.confidence))


# ---------------------------------------------------------------------------------------------------- sampler
class MT19937:
    def __init__(self, seed):
        mt = [seed & 0xFFFFFFFF]
        for i in range(1, 624):
            mt.append((1812433253 * (mt[-1] ^ (mt[-1] >> 30)) + i) & 0xFFFFFFFF)
        self.mt, self.idx = mt, 624

    def next(self):
        mt = self.mt
        if self.idx >= 624:
            for i in range(624):
                y = (mt[i] & 0x80000000) | (mt[(i + 1) % 624] & 0x7FFFFFFF)
                mt[i] = mt[(i + 397) % 624] ^ (y >> 1) ^ (0x9908B0DF if y & 1 else 0)
            self.idx = 0
        y = mt[self.idx]
        self.idx += 1
        y ^= y >> 11
        y ^= (y << 7) & 0x9D2C5680
        y ^= (y << 15) & 0xEFC60000
        y ^= y >> 18
        return y & 0xFFFFFFFF


@functools.lru_cache(maxsize=None)
def sample_triples(seed, n, n_trials):
    g, idx, last, out = MT19937(seed), list(range(n)), n - 1, np.zeros((n_trials, 3), np.int32)
    for t in range(n_trials):
        for i in range(3):
            m = last - i + 1
            s = 0xFFFFFFFF // m
            while True:
                x = g.next()
                if x < m * s:
                    break
            j = i + x // s
            idx[i], idx[j] = idx[j], idx[i]
        out[t] = idx[:3]
    return out


# ---------------------------------------------------------------------------------------------------- small linear algebra
def _tols(dt):
    ext = np.dtype(dt) == np.dtype(EXT)
    return dict(rot=dt(1e-18 if ext else 1e-15), floor=dt(1e-21 if ext else 1e-18), root=dt(2.0 ** (-61 if ext else -50)))


def rotation_from_cov(A):
    """batched: the proper rotation U V^T of every 3x3 A = U S V^T [B, 3, 3] by one-sided Jacobi; the column with the shortest image is
    replaced by the cross products of the two others"""
    dt = A.dtype.type
    tol = _tols(dt)["rot"]
    A = A.copy()
    V = np.broadcast_to(np.eye(3, dtype=A.dtype), A.shape).copy()
    with np.errstate(all="ignore"):
        for _ in range(20):
            rotated = False
            for p, q in ((0, 1), (0, 2), (1, 2)):
                al, be, ga = (A[:, :, p] ** 2).sum(1), (A[:, :, q] ** 2).sum(1), (A[:, :, p] * A[:, :, q]).sum(1)
                m = np.abs(ga) > tol * np.sqrt(al * be)
                if not m.any():
                    continue
                rotated = True
                zeta = np.where(m, (be - al) / np.where(m, 2 * ga, 1), 1)
                t = np.copysign(dt(1), zeta) / (np.abs(zeta) + np.sqrt(1 + zeta * zeta))
                c = np.where(m, 1 / np.sqrt(1 + t * t), 1)
                s = np.where(m, c * t, 0)
                for Z in (A, V):
                    zp, zq = Z[:, :, p].copy(), Z[:, :, q].copy()
                    Z[:, :, p] = c[:, None] * zp - s[:, None] * zq
                    Z[:, :, q] = s[:, None] * zp + c[:, None] * zq
            if not rotated:
                break
        nn = (A ** 2).sum(1)
        drop = np.where((nn[:, 0] <= nn[:, 1]) & (nn[:, 0] <= nn[:, 2]), 0, np.where(nn[:, 1] <= nn[:, 2], 1, 2))
        i1, i2 = np.where(drop == 0, 1, 0), np.where(drop == 2, 1, 2)
        b = np.arange(len(A))
        u1, u2 = A[b, :, i1] / np.sqrt(nn[b, i1])[:, None], A[b, :, i2] / np.sqrt(nn[b, i2])[:, None]
        v1, v2 = V[b, :, i1], V[b, :, i2]
        u3, v3 = np.cross(u1, u2), np.cross(v1, v2)
        return u1[:, :, None] * v1[:, None, :] + u2[:, :, None] * v2[:, None, :] + u3[:, :, None] * v3[:, None, :]


def jacobi_eig(M):
    """eigenvalues and eigenvectors (columns) of a symmetric matrix by cyclic two-sided Jacobi"""
    dt = M.dtype.type
    tl = _tols(dt)
    M = M.copy()
    N = len(M)
    V = np.eye(N, dtype=M.dtype)
    floor_abs = tl["floor"] * np.abs(np.diag(M)).sum()
    for _ in range(30):
        rotated = False
        for p in range(N - 1):
            for q in range(p + 1, N):
                mpq, mpp, mqq = M[p, q], M[p, p], M[q, q]
                if not (abs(mpq) > tl["rot"] * np.sqrt(abs(mpp * mqq)) + floor_abs):
                    continue
                rotated = True
                theta = (mqq - mpp) / (2 * mpq)
                t = np.copysign(dt(1), theta) / (abs(theta) + np.sqrt(1 + theta * theta))
                c = 1 / np.sqrt(1 + t * t)
                s = c * t
                mp, mq = M[:, p].copy(), M[:, q].copy()
                M[:, p], M[:, q] = c * mp - s * mq, s * mp + c * mq
                vp, vq = V[:, p].copy(), V[:, q].copy()
                V[:, p], V[:, q] = c * vp - s * vq, s * vp + c * vq
                mp, mq = M[p, :].copy(), M[q, :].copy()
                M[p, :], M[q, :] = c * mp - s * mq, s * mp + c * mq
                M[p, q] = M[q, p] = 0
        if not rotated:
            break
    return np.diag(M).copy(), V


def ls_solve(A, b, thr):
    """minimum-norm least squares by one-sided Jacobi SVD; singular values at or below thr times the largest are dropped"""
    dt = A.dtype.type
    tol = _tols(dt)["rot"]
    A = A.copy()
    c = A.shape[1]
    V = np.eye(c, dtype=A.dtype)
    for _ in range(30):
        rotated = False
        for p in range(c - 1):
            for q in range(p + 1, c):
                al, be, ga = (A[:, p] ** 2).sum(), (A[:, q] ** 2).sum(), (A[:, p] * A[:, q]).sum()
                if not (abs(ga) > tol * np.sqrt(al * be)):
                    continue
                rotated = True
                zeta = (be - al) / (2 * ga)
                t = np.copysign(dt(1), zeta) / (abs(zeta) + np.sqrt(1 + zeta * zeta))
                cs = 1 / np.sqrt(1 + t * t)
                sn = cs * t
                for Z in (A, V):
                    zp, zq = Z[:, p].copy(), Z[:, q].copy()
                    Z[:, p], Z[:, q] = cs * zp - sn * zq, sn * zp + cs * zq
        if not rotated:
            break
    s2 = (A ** 2).sum(0)
    x = np.zeros(c, A.dtype)
    for j in range(c):
        if s2[j] > 0 and np.sqrt(s2[j]) > thr * np.sqrt(s2.max()):
            x = x + V[:, j] * ((A[:, j] * b).sum() / s2[j])
    return x


def seq_sum(a):
    """sum over axis 0 in index order"""
    return np.cumsum(a, axis=0)[-1]


# ---------------------------------------------------------------------------------------------------- geometry
def residuals(P, xy, X):
    """P [..., 3, 4]; -> [..., n]"""
    dt = X.dtype.type
    with np.errstate(all="ignore"):
        px = P[..., None, :, :3] @ X[:, :, None]
        px = px[..., 0] + P[..., None, :, 3]
        pz = px[..., 2]
        front = pz > dt(DBL_EPS)
        inv = 1 / np.where(front, pz, 1)
        dx, dy = xy[:, 0] - px[..., 0] * inv, xy[:, 1] - px[..., 1] * inv
        return np.where(front, dx * dx + dy * dy, dt(DBL_MAX))


def supports(res, max_res):
    inl = res <= max_res
    return inl.sum(-1), np.cumsum(np.where(inl, res, 0), axis=-1)[..., -1], inl


def p3p_chunk(xy, X, flags):
    """xy [T, 3, 2], X [T, 3, 3] -> per trial the list of models (3x4) in ascending root order"""
    dt = X.dtype.type
    T = len(X)
    cdt = np.clongdouble if np.dtype(dt) == np.dtype(EXT) else np.complex128
    with np.errstate(all="ignore"):
        lift = np.concatenate([xy, np.ones((T, 3, 1), X.dtype)], 2) / np.sqrt((xy ** 2).sum(2) + 1)[:, :, None]
        u, v, w = lift[:, 0], lift[:, 1], lift[:, 2]
        cos_uv, cos_uw, cos_vw = (u * v).sum(1), (u * w).sum(1), (v * w).sum(1)
        dAB2, dAC2, dBC2 = ((X[:, 0] - X[:, 1]) ** 2).sum(1), ((X[:, 0] - X[:, 2]) ** 2).sum(1), ((X[:, 1] - X[:, 2]) ** 2).sum(1)
        dAB, a, b = np.sqrt(dAB2), dBC2 / dAB2, dAC2 / dAB2
        a2, b2, p, q, r = a * a, b * b, 2 * cos_vw, 2 * cos_uw, 2 * cos_uv
        p2, q2, r2 = p * p, q * q, r * r
        p3, r3 = p2 * p, r2 * r
        r4 = r3 * r
        r5 = r4 * r
        c0 = -2 * b + b2 + a2 + 1 + a * b * (2 - r2) - 2 * a
        c1 = -2 * q * a2 - r * p * b2 + 4 * q * a + (2 * q + p * r) * b + (r2 * q - 2 * q + r * p) * a * b - 2 * q
        c2 = (2 + q2) * a2 + (p2 + r2 - 2) * b2 - (4 + 2 * q2) * a - (p * q * r + p2) * b - (p * q * r + r2) * a * b + q2 + 2
        c3 = -2 * q * a2 - r * p * b2 + 4 * q * a + (p * r + q * p2 - 2 * q) * b + (r * p + 2 * q) * a * b - 2 * q
        c4 = a2 + b2 - 2 * a + (2 - p2) * b - 2 * a * b + 1
        m = np.stack([c1 / c0, c2 / c0, c3 / c0, c4 / c0], 1)                     # z^4 + m0 z^3 + m1 z^2 + m2 z + m3
        valid = (c0 != 0) & np.isfinite(m).all(1)
        mm = np.where(valid[:, None], m, 0)
        rad = 1 + np.abs(mm).max(1)
        kc, ks = dt(0.9210609940028851), dt(0.3894183423086505)
        start = np.array([kc + 1j * ks, -ks + 1j * kc, -kc - 1j * ks, ks - 1j * kc], cdt)
        z = rad[:, None].astype(cdt) * start[None, :]
        active = valid.copy()
        tol2 = _tols(dt)["root"] ** 2
        for _ in range(ROOT_ITERS):
            if not active.any():
                break
            moved = np.zeros(T, bool)
            for i in range(4):
                zi = z[:, i]
                pv = zi + mm[:, 0]
                dv = np.ones(T, cdt)
                for k in range(3):
                    dv = dv * zi + pv
                    pv = pv * zi + mm[:, k + 1]
                nwt = pv / dv
                S = sum(1 / (zi - z[:, j]) for j in range(4) if j != i)
                wv = nwt / (1 - nwt * S)
                upd = active & (dv != 0) & (pv != 0)
                big = ~((wv.real ** 2 + wv.imag ** 2) <= tol2 * (zi.real ** 2 + zi.imag ** 2))
                moved |= upd & big
                z[:, i] = np.where(upd, zi - wv, zi)
            active &= moved
            bad = active & ~np.isfinite(z.real).all(1)
            valid &= ~bad
            active &= ~bad
        order = np.argsort(z.real, axis=1, kind="stable")
        z = np.take_along_axis(z, order, 1)
        x, xim = z.real.astype(X.dtype), z.imag.astype(X.dtype)
        rej_imag = ~(np.abs(xim) <= dt(ROOT_MAX_IMAG))
        rej_sign = ~rej_imag & ~(x >= 0)
        take = valid[:, None] & ~rej_imag & ~rej_sign
        if (valid[:, None] & rej_imag).any():
            flags.add("root_rejected_imag")
        if (valid[:, None] & rej_sign).any():
            flags.add("root_rejected_sign")
        ti, si = np.nonzero(take)
        models = [[] for _ in range(T)]
        if len(ti) == 0:
            return models
        g = lambda arr: arr[ti]
        a, b, a2, b2, p, q, r, p2, q2, r2, p3, r3, r4, r5, cos_uv, dAB = map(g, (a, b, a2, b2, p, q, r, p2, q2, r2, p3, r3, r4, r5, cos_uv, dAB))
        x = x[ti, si]
        x2 = x * x
        x3 = x2 * x
        bb1 = (p2 - p * q * r + r2) * a + (p2 - r2) * b - p2 + p * q * r - r2
        b1 = b * bb1 * bb1
        b0 = (((1 - a - b) * x2 + (a - 1) * q * x - a + b + 1) *
              (r3 * (a2 + b2 - 2 * a - 2 * b + (2 - r2) * a * b + 1) * x3 +
               r2 * (p + p * a2 - 2 * r * q * a * b + 2 * r * q * b - 2 * r * q - 2 * p * a - 2 * p * b + p * r2 * b + 4 * r * q * a +
                     q * r3 * a * b - 2 * r * q * a2 + 2 * p * a * b + p * b2 - r2 * p * b2) * x2 +
               (r5 * (b2 - a * b) - r4 * p * q * b + r3 * (q2 - 4 * a - 2 * q2 * a + q2 * a2 + 2 * a2 - 2 * b2 + 2) +
                r2 * (4 * p * q * a - 2 * p * q * a * b + 2 * p * q * b - 2 * p * q - 2 * p * q * a2) +
                r * (p2 * b2 - 2 * p2 * b + 2 * p2 * a * b - 2 * p2 * a + p2 + p2 * a2)) * x +
               (2 * p * r2 - 2 * r3 * q + p3 - 2 * p2 * q * r + p * q2 * r2) * a2 + (p3 - 2 * p * r2) * b2 +
               (4 * q * r3 - 4 * p * r2 - 2 * p3 + 4 * p2 * q * r - 2 * p * q2 * r2) * a + (-2 * q * r3 + p * r4 + 2 * p2 * q * r - 2 * p3) * b +
               (2 * p3 + 2 * q * r3 - 2 * p2 * q * r) * a * b + p * q2 * r2 - 2 * p2 * q * r + 2 * p * r2 + p3 - 2 * r3 * q))
        y = b0 / b1
        nu = x2 + y * y - 2 * x * y * cos_uv
        dPC = dAB / np.sqrt(nu)
        cam = np.stack([u[ti] * (x * dPC)[:, None], v[ti] * (y * dPC)[:, None], w[ti] * dPC[:, None]], 1)       # [B, point, 3]
        Xs = X[ti]
        ms, md = Xs.sum(1) / 3, cam.sum(1) / 3
        sig = ((cam - md[:, None, :])[:, :, :, None] * (Xs - ms[:, None, :])[:, :, None, :]).sum(1) / 3
        R = rotation_from_cov(sig)
        tt = md - (R @ ms[:, :, None])[:, :, 0]
        P = np.concatenate([R, tt[:, :, None]], 2)
        ok = np.isfinite(P).all((1, 2))
        for k in range(len(ti)):
            if ok[k]:
                models[ti[k]].append(P[k])
        return models


def epnp(xy, X, flags):
    """EPNPEstimator::ComputePose on the given correspondences (the inliers, in index order) -> 3x4 model or None"""
    dt = X.dtype.type
    n = len(X)
    with np.errstate(all="ignore"):
        c0 = seq_sum(X) / n
        PW0 = X - c0
        D, U = jacobi_eig(seq_sum(PW0[:, :, None] * PW0[:, None, :]))
        order = np.argsort(-np.abs(D), kind="stable")
        cws = [c0] + [c0 + np.sqrt(np.abs(D[order[i]]) / n) * U[:, order[i]] for i in range(3)]
        CC = np.stack([cws[j] - cws[0] for j in (1, 2, 3)], 1)
        # rank by column-pivoted orthogonalisation at Eigen's default threshold (3 eps of the largest pivot)
        C, used, piv = CC.copy(), [False] * 3, []
        for _ in range(3):
            nn = [(C[:, j] ** 2).sum() if not used[j] else -1 for j in range(3)]
            best = int(np.argmax(nn))
            used[best] = True
            piv.append(np.sqrt(nn[best]))
            if not nn[best] > 0:
                break
            for j in range(3):
                if not used[j]:
                    C[:, j] = C[:, j] - ((C[:, best] * C[:, j]).sum() / nn[best]) * C[:, best]
        piv += [dt(0)] * (3 - len(piv))
        thr = piv[0] * dt(3 * DBL_EPS)
        if not (piv[0] > 0 and piv[1] > thr and piv[2] > thr):
            flags.add("local_no_model")
            return None
        det = (CC[0, 0] * (CC[1, 1] * CC[2, 2] - CC[1, 2] * CC[2, 1]) - CC[0, 1] * (CC[1, 0] * CC[2, 2] - CC[1, 2] * CC[2, 0]) +
               CC[0, 2] * (CC[1, 0] * CC[2, 1] - CC[1, 1] * CC[2, 0]))
        cof = np.array([[CC[1, 1] * CC[2, 2] - CC[1, 2] * CC[2, 1], CC[0, 2] * CC[2, 1] - CC[0, 1] * CC[2, 2], CC[0, 1] * CC[1, 2] - CC[0, 2] * CC[1, 1]],
                        [CC[1, 2] * CC[2, 0] - CC[1, 0] * CC[2, 2], CC[0, 0] * CC[2, 2] - CC[0, 2] * CC[2, 0], CC[0, 2] * CC[1, 0] - CC[0, 0] * CC[1, 2]],
                        [CC[1, 0] * CC[2, 1] - CC[1, 1] * CC[2, 0], CC[0, 1] * CC[2, 0] - CC[0, 0] * CC[2, 1], CC[0, 0] * CC[1, 1] - CC[0, 1] * CC[1, 0]]],
                       X.dtype)
        CCi = cof / det
        if not np.isfinite(CCi).all():
            flags.add("local_no_model")
            return None
        al = np.zeros((n, 4), X.dtype)
        al[:, 1:] = PW0 @ CCi.T
        al[:, 0] = 1 - al[:, 1] - al[:, 2] - al[:, 3]
        M = np.zeros((2 * n, 12), X.dtype)
        for j in range(4):
            M[0::2, 3 * j] = al[:, j]
            M[0::2, 3 * j + 2] = -al[:, j] * xy[:, 0]
            M[1::2, 3 * j + 1] = al[:, j]
            M[1::2, 3 * j + 2] = -al[:, j] * xy[:, 1]
        MtM = np.zeros((12, 12), X.dtype)
        for lo in range(0, 2 * n, 256):                    # in row order, 256 rows at a time
            MtM = seq_sum(np.concatenate([MtM[None], M[lo:lo + 256, :, None] * M[lo:lo + 256, None, :]], 0))
        ev, V = jacobi_eig(MtM)
        small = np.argsort(ev, kind="stable")[:4]
        Ut = [V[:, k] for k in small]                    # Ut rows 11, 10, 9, 8
        pairs = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
        L = np.zeros((6, 10), X.dtype)
        rho = np.zeros(6, X.dtype)
        for j, (a, b) in enumerate(pairs):
            dv = [Ut[i][3 * a:3 * a + 3] - Ut[i][3 * b:3 * b + 3] for i in range(4)]
            d = lambda i, k: (dv[i] * dv[k]).sum()
            L[j] = [d(0, 0), 2 * d(0, 1), d(1, 1), 2 * d(0, 2), 2 * d(1, 2), d(2, 2), 2 * d(0, 3), 2 * d(1, 3), 2 * d(2, 3), d(3, 3)]
            rho[j] = ((cws[a] - cws[b]) ** 2).sum()
        cands = []
        for cand in range(3):
            be = np.zeros(4, X.dtype)
            cols = [(0, 1, 3, 6), (0, 1, 2), (0, 1, 2, 3, 4)][cand]
            x = ls_solve(L[:, cols], rho, dt(len(cols) * DBL_EPS))
            if cand == 0:
                be[0] = np.sqrt(-x[0]) if x[0] < 0 else np.sqrt(x[0])
                be[1:] = (-x[1:] if x[0] < 0 else x[1:]) / be[0]
            else:
                if x[0] < 0:
                    be[0], be[1] = np.sqrt(-x[0]), (np.sqrt(-x[2]) if x[2] < 0 else 0)
                else:
                    be[0], be[1] = np.sqrt(x[0]), (np.sqrt(x[2]) if x[2] > 0 else 0)
                if x[1] < 0:
                    be[0] = -be[0]
                be[2] = x[3] / be[0] if cand == 2 else 0
            for _ in range(5):
                A = np.stack([2 * L[:, 0] * be[0] + L[:, 1] * be[1] + L[:, 3] * be[2] + L[:, 6] * be[3],
                              L[:, 1] * be[0] + 2 * L[:, 2] * be[1] + L[:, 4] * be[2] + L[:, 7] * be[3],
                              L[:, 3] * be[0] + L[:, 4] * be[1] + 2 * L[:, 5] * be[2] + L[:, 8] * be[3],
                              L[:, 6] * be[0] + L[:, 7] * be[1] + L[:, 8] * be[2] + 2 * L[:, 9] * be[3]], 1)
                rhs = rho - (L[:, 0] * be[0] * be[0] + L[:, 1] * be[0] * be[1] + L[:, 2] * be[1] * be[1] + L[:, 3] * be[0] * be[2] +
                             L[:, 4] * be[1] * be[2] + L[:, 5] * be[2] * be[2] + L[:, 6] * be[0] * be[3] + L[:, 7] * be[1] * be[3] +
                             L[:, 8] * be[2] * be[3] + L[:, 9] * be[3] * be[3])
                be = be + ls_solve(A, rhs, dt(0))
            cc = sum(be[i] * Ut[i] for i in range(4)).reshape(4, 3)
            pcs = al @ cc
            if pcs[0, 2] < 0:
                cc, pcs = -cc, -pcs
            pc0, pw0 = seq_sum(pcs) / n, seq_sum(X) / n
            abt = seq_sum((pcs - pc0)[:, :, None] * (X - pw0)[:, None, :])
            R = rotation_from_cov(abt[None])[0]
            P = np.concatenate([R, (pc0 - R @ pw0)[:, None]], 1)
            cands.append((seq_sum(np.sqrt(residuals(P, xy, X))), P))
        best = 0
        if cands[1][0] < cands[0][0]:
            best = 1
        if cands[2][0] < cands[best][0]:
            best = 2
        P = cands[best][1]
        if not np.isfinite(P).all():
            flags.add("local_no_model")
            return None
        return P


def quat_of(P):
    m = P
    tr = m[0, 0] + m[1, 1] + m[2, 2]
    if tr > 0:
        s = np.sqrt(tr + 1) * 2
        w, x, y, z = s / 4, (m[2, 1] - m[1, 2]) / s, (m[0, 2] - m[2, 0]) / s, (m[1, 0] - m[0, 1]) / s
    elif m[0, 0] > m[1, 1] and m[0, 0] > m[2, 2]:
        s = np.sqrt(1 + m[0, 0] - m[1, 1] - m[2, 2]) * 2
        w, x, y, z = (m[2, 1] - m[1, 2]) / s, s / 4, (m[0, 1] + m[1, 0]) / s, (m[0, 2] + m[2, 0]) / s
    elif m[1, 1] > m[2, 2]:
        s = np.sqrt(1 + m[1, 1] - m[0, 0] - m[2, 2]) * 2
        w, x, y, z = (m[0, 2] - m[2, 0]) / s, (m[0, 1] + m[1, 0]) / s, s / 4, (m[1, 2] + m[2, 1]) / s
    else:
        s = np.sqrt(1 + m[2, 2] - m[0, 0] - m[1, 1]) * 2
        w, x, y, z = (m[1, 0] - m[0, 1]) / s, (m[0, 2] + m[2, 0]) / s, (m[1, 2] + m[2, 1]) / s, s / 4
    q = np.array([x, y, z, w], P.dtype)
    return q * ((-1 if w < 0 else 1) / np.sqrt((q * q).sum()))


def quat_to_mat(q, dtype=EXT):
    x, y, z, w = (dtype(v) for v in q)
    n = x * x + y * y + z * z + w * w
    s = 2 / n
    return np.array([[1 - s * (y * y + z * z), s * (x * y - z * w), s * (x * z + y * w)],
                     [s * (x * y + z * w), 1 - s * (x * x + z * z), s * (y * z - x * w)],
                     [s * (x * z - y * w), s * (y * z + x * w), 1 - s * (x * x + y * y)]], dtype)


# ---------------------------------------------------------------------------------------------------- the rule
def run_frame(xy, X, opt=None, dtype=EXT, max_error=None, seed=None, want_records=False):
    """-> dict(status, mask, num_inliers, num_trials, best_trial, P (3x4, dtype) / q / t on status 1, flags, records)"""
    opt = opt or Options()
    dt = np.dtype(dtype).type
    n = len(xy)
    out = dict(status=0, mask=np.zeros(n, np.uint8), num_inliers=0, num_trials=0, best_trial=-1, flags=set(), records=[])
    if n < 3 or n > MAX_CORR:
        out["status"] = 2 if n < 3 else 3
        return out
    xy, X = np.asarray(xy, np.float64).astype(dtype), np.asarray(X, np.float64).astype(dtype)
    me = dt(opt.max_error if max_error is None else max_error)
    max_res = me * me
    cap = trial_cap(opt)
    tri = sample_triples(int(opt.seed if seed is None else seed), n, cap)
    flags = out["flags"]
    best_count, best_sum, best_trial, best_local, best_P = 0, dt(DBL_MAX), -1, False, None
    dyn, abort, num_trials = cap, False, cap
    beats = lambda ca, sa, cb, sb: ca > cb or (ca == cb and sa < sb)
    for t0 in range(0, cap, CHUNK):
        sel = tri[t0:t0 + CHUNK]
        models = p3p_chunk(xy[sel], X[sel], flags)
        flat = [P for ms in models for P in ms]
        if flat:
            cnts, sums, _ = supports(residuals(np.stack(flat), xy, X), max_res)
        k = 0
        for l, ms in enumerate(models):
            t = t0 + l
            if not ms:
                flags.add("trial_without_model")
            for P in ms:
                cnt, sm = int(cnts[k]), sums[k]
                k += 1
                rec = [t, cnt, float(sm), -2, 0.0]
                if beats(cnt, sm, best_count, best_sum):
                    best_count, best_sum, best_trial, best_local, best_P = cnt, sm, t, False, P
                    if cnt > 3:
                        inl = residuals(P, xy, X) <= max_res
                        Pl = epnp(xy[inl], X[inl], flags)
                        rec[3] = -1
                        if Pl is not None:
                            lc, ls, _ = supports(residuals(Pl, xy, X), max_res)
                            rec[3], rec[4] = int(lc), float(ls)
                            if beats(int(lc), ls, best_count, best_sum):
                                best_count, best_sum, best_local, best_P = int(lc), ls, True, Pl
                                flags.add("local_wins")
                            else:
                                flags.add("local_loses")
                    dyn = num_trials_bound(best_count, n, opt.confidence)
                out["records"].append(rec)
                if t >= dyn and t >= opt.min_num_trials:
                    abort = True
                    num_trials = t + 2 if t + 1 < cap else t + 1
                    flags.add("abort_dyn")
                    break
            if abort:
                break
        if abort:
            break
    if not abort:
        flags.add("cap_reached")
    out["scan"] = dict(n=n, best_trial=best_trial, local=int(best_local), num_trials=num_trials, success=int(best_count >= 3))
    if not want_records:
        out["records"] = []
    if best_count < 3 or best_P is None or not np.isfinite(best_P).all():
        return out
    inl = residuals(best_P, xy, X) <= max_res
    out.update(status=1, mask=inl.astype(np.uint8), num_inliers=int(inl.sum()), num_trials=num_trials,
               best_trial=best_trial | (LOCAL_BIT if best_local else 0), P=best_P, q=quat_of(best_P), t=best_P[:, 3].copy())
    return out


def mask_check(q, t, xy, X, max_error, mask, rel=1e-9):
    """the residuals of (q, t) in extended precision reproduce mask wherever the residual is farther than rel from max_error^2"""
    P = np.concatenate([quat_to_mat(q), np.asarray(t, np.float64).astype(EXT)[:, None]], 1)
    res = residuals(P, np.asarray(xy).astype(EXT), np.asarray(X).astype(EXT))
    mr = EXT(max_error) ** 2
    clear = np.abs(res - mr) > rel * mr
    return bool(np.array_equal((res <= mr)[clear], np.asarray(mask, bool)[clear]))


def deviation(R, t, e):
    """of a pose (rotation matrix, t) from the extended result e"""
    Re, te = np.asarray(e["P"][:, :3], np.float64), np.asarray(e["t"], np.float64)
    return max(float(np.abs(np.asarray(R, np.float64) - Re).max()), float(np.abs(np.asarray(t, np.float64) - te).max() / max(1.0, np.abs(te).max())))


# ---------------------------------------------------------------------------------------------------- catalogue
LENGTHS = (3, 4, 5, 20, 63, 64, 65, 255, 256, 257, 1000)
MAX_ERROR = 8.0 / 800.0


def _rand_rot(rng):
    q = rng.normal(size=4)
    return np.asarray(quat_to_mat(q / np.linalg.norm(q), np.float64), np.float64)


def _frame(rng, n, outlier=0.0, tag="", planar=False, behind=0, noise=0.1):
    R = _rand_rot(rng)
    Xc = np.stack([rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(3, 9, n)], 1)       # in the camera frame
    t = rng.uniform(-1, 1, 3)
    if planar:
        R, t = _rand_rot(rng), None
        Xw = np.stack([rng.uniform(-2, 2, n), rng.uniform(-2, 2, n), np.full(n, 4.0)], 1)
        R = np.asarray(quat_to_mat([0.2, -0.1, 0.05, 0.97], np.float64), np.float64)
        t = np.array([0.1, -0.2, 2.0])
        Xc = Xw @ R.T + t
    else:
        Xw = (Xc - t) @ R                     # Xc = R Xw + t
    xy = Xc[:, :2] / Xc[:, 2:3] + np.clip(rng.normal(size=(n, 2)), -2.5, 2.5) * (noise * MAX_ERROR)
    k = int(round(outlier * n))
    out = rng.permutation(n)[:k]
    xy[out] = rng.uniform(-0.6, 0.6, (k, 2))
    if behind:
        bi = rng.permutation(n)[:behind]
        Xb = Xc[bi] * [1, 1, -1]
        Xw[bi] = (Xb - t) @ R
    return dict(xy=np.ascontiguousarray(xy), X=np.ascontiguousarray(Xw), tag=tag, R=R, t=t)


@functools.lru_cache(maxsize=None)
def pool():
    rng = np.random.default_rng(20261019)
    F = [_frame(rng, n, 0.3 if n >= 20 else 0.0, "len%d" % n) for n in LENGTHS]
    F += [_frame(rng, 100, s, "share%g" % s) for s in (0.0, 0.3, 0.6, 0.8)]
    F.append(_frame(rng, 50, 1.0, "outliers_only"))
    F.append(_frame(rng, 40, 0.2, "behind_camera", behind=10))
    F.append(_frame(rng, 30, 0.1, "planar", planar=True))
    f = _frame(rng, 12, 0.0, "repeated_point")
    f["X"][1:4] = f["X"][0]
    f["xy"][1:4] = f["xy"][0]
    F.append(f)
    f = _frame(rng, 6, 0.0, "one_point_only")
    f["X"][:] = f["X"][0]
    F.append(f)
    F.append(_frame(rng, MAX_CORR + 1, 0.0, "too_long"))
    F.append(_frame(rng, 2, 0.0, "two"))
    F.append(dict(xy=np.zeros((0, 2)), X=np.zeros((0, 3)), tag="empty", R=np.eye(3), t=np.zeros(3)))
    F += [_frame(rng, int(n), float(s), "random") for n, s in zip(rng.integers(8, 120, 24), rng.uniform(0, 0.5, 24))]
    return F


OPTION_SETS = {
    "defaults": (),
    "early": (("min_num_trials", 0), ("confidence", 0.99)),
    "cap7": (("max_num_trials", 7), ("min_num_trials", 7)),
    "cap64": (("max_num_trials", 64), ("min_num_trials", 64)),
    "cap65": (("max_num_trials", 65), ("min_num_trials", 64)),
}
OPTION_FRAMES = ("len5", "len20", "len65", "share0.6", "repeated_point")      # the frames the other option sets run on


def frames_of(opt_name):
    P = pool()
    return list(range(len(P))) if opt_name == "defaults" else [k for k, f in enumerate(P) if f["tag"] in OPTION_FRAMES]


def _perturbed(a, rng):
    """every coordinate times 1 +- 2^-43; equal values get equal factors"""
    vals, inv = np.unique(a, return_inverse=True)
    return (vals * (1.0 + PERTURBATION * rng.choice([-1.0, 1.0], len(vals))))[inv].reshape(a.shape)


@functools.lru_cache(maxsize=None)
def reference(dtype_name="longdouble", opt_name="defaults"):
    """pool index -> the yardstick's result, for the frames of the option set"""
    opt = Options(**dict(OPTION_SETS[opt_name]))
    P = pool()
    return {k: run_frame(P[k]["xy"], P[k]["X"], opt=opt, dtype=np.dtype(dtype_name), want_records=(dtype_name == "longdouble"))
            for k in frames_of(opt_name)}


DISCRETE = ("status", "num_inliers", "num_trials", "best_trial")


def same_discrete(a, b):
    return all(int(a[k]) == int(b[k]) for k in DISCRETE) and np.array_equal(a["mask"], b["mask"])


@functools.lru_cache(maxsize=None)
def fragile(opt_name="defaults"):
    """pool index -> bool"""
    ext, f64, P = reference("longdouble", opt_name), reference("float64", opt_name), pool()
    opt = Options(**dict(OPTION_SETS[opt_name]))
    out = {}
    for k in frames_of(opt_name):
        bad = not same_discrete(ext[k], f64[k])
        n = len(P[k]["xy"])
        if not bad and 3 <= n <= MAX_CORR:
            for rerun in range(3):
                rng = np.random.default_rng(1000 * rerun + k)
                r = run_frame(_perturbed(P[k]["xy"], rng), _perturbed(P[k]["X"], rng), opt=opt, dtype=np.float64)
                if not same_discrete(ext[k], r):
                    bad = True
                    break
        out[k] = bad
    return out


def fragile_share():
    """over the whole catalogue: every (option set, frame)"""
    fr = [v for name in OPTION_SETS for v in fragile(name).values()]
    return sum(fr) / len(fr)


@functools.lru_cache(maxsize=None)
def restatement_deviation():
    """the float64 restatement's largest deviation from the extended run over the non-fragile status-1 frames of the catalogue"""
    worst = 0.0
    for name in OPTION_SETS:
        ext, f64, fr = reference("longdouble", name), reference("float64", name), fragile(name)
        for k, e in ext.items():
            if e["status"] == 1 and not fr[k]:
                worst = max(worst, deviation(np.asarray(f64[k]["P"][:, :3], np.float64), np.asarray(f64[k]["t"], np.float64), e))
    return worst


def all_flags():
    return set().union(*[e["flags"] for name in OPTION_SETS for e in reference("longdouble", name).values()])


@functools.lru_cache(maxsize=None)
def cases():
    """name -> pool indices in batch order (default options): one frame, every frame, and 257 frames (more workgroups than compute
    units) drawn from the frames of at most 257 correspondences"""
    P = pool()
    ext = reference("longdouble")
    small = [k for k, f in enumerate(P) if len(f["xy"]) <= 257]
    rng = np.random.default_rng(3)
    one = next(k for k in small if ext[k]["status"] == 1 and len(P[k]["xy"]) >= 20)
    return {"one": [one], "all": list(range(len(P))), "b257": [int(k) for k in rng.permutation((small * (257 // len(small) + 1))[:257])]}


def arrays(idx):
    """-> corr_ptr, xy, points3d of the frames idx"""
    P = pool()
    ptr = np.zeros(len(idx) + 1, np.int32)
    ptr[1:] = np.cumsum([len(P[k]["xy"]) for k in idx])
    return ptr, np.ascontiguousarray(np.concatenate([P[k]["xy"] for k in idx])), np.ascontiguousarray(np.concatenate([P[k]["X"] for k in idx]))


TIGHT_BAR = TIGHT_FACTOR * RESTATEMENT_DEVIATION
