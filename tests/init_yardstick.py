"""Yardstick of the two-view initialisation (xrsfm_ba_two_view_init): the rule of ba_init_scan.h and the geometry of
ba_init_geom.h restated in numpy, run in np.longdouble (the reference) and np.float64 (the restatement whose own deviation from the
extended run sets the tight bars), with its own MT19937, Jacobi and eigenvalue routines, and the catalogue of pairs.

Nothing here reads the library.  The convergence thresholds of the iterations scale with the precision (the float64 run uses the
library's constants), the decision thresholds (|Im| < 1e-10, the inlier test, the depth and angle tests) do not."""
import functools
import math

import numpy as np

MAX_MATCHES, MAX_TRIALS, SLOT_STRIDE, UNBOUNDED = 8192, 64, 16, 2 ** 31 - 1
DEG = 0.0174532925199432954743716805978692718781530857086181640625
FX = 800.0
TH = 10.0 / FX
FRAGILE_CAP = 0.05
TIGHT_FACTOR = 16
# The float64 restatement's largest deviation from the longdouble run over the non-fragile pairs of the catalogue, measured by
# restatement_deviation() and asserted (not below it, not inflated beyond 4x) in tests/test_init_cpu.py:
#   E (unit norm, up to sign), R, t: absolute; points: relative to 1 + |p|; det E and the trace constraint: absolute
# Measured: restatement E 8.41e-9, R 3.25e-10, t 1.21e-8, points 2.26e-7, det 5.72e-12, trace 1.08e-9 (all from one pair, n = 11 with
# a narrow baseline; the others stay below 2e-10); sequential host build of the headers 1.14e-8 / 4.41e-10 / 1.64e-8 / 3.06e-7 /
# 7.76e-12 / 1.47e-9; library on the GPU 2.15e-9 / 8.32e-11 / 3.10e-9 / 5.78e-8 / 1.45e-12 / 2.76e-10.
RESTATEMENT_DEVIATION = dict(E=8.5e-9, R=3.3e-10, t=1.3e-8, points=2.3e-7, det=5.8e-12, trace=1.1e-9)
TIGHT_BAR = {k: TIGHT_FACTOR * v for k, v in RESTATEMENT_DEVIATION.items()}


class Options:
    def __init__(self, **kw):
        self.confidence, self.max_iterations, self.seed, self.min_matches, self.max_depth = 0.9, 50, 0, 10, 100.0
        self.min_angle_rad = (16.0 * DEG, 8.0 * DEG)
        self.min_front_ratio, self.min_angle_ratio, self.min_num_valid = 0.5, 0.5, 200
        for k, v in kw.items():
            if not hasattr(self, k):
                raise AttributeError(k)
            setattr(self, k, v)


# ---------------------------------------------------------------------------------------------------- sampler
class MT19937:
    def __init__(self, seed):
        mt = [seed & 0xFFFFFFFF]
        for i in range(1, 624):
            mt.append((1812433253 * (mt[-1] ^ (mt[-1] >> 30)) + i) & 0xFFFFFFFF)
        self.mt, self.idx = mt, 624

    def next(self):
        if self.idx >= 624:
            mt = self.mt
            for i in range(624):
                y = (mt[i] & 0x80000000) | (mt[(i + 1) % 624] & 0x7FFFFFFF)
                mt[i] = mt[(i + 397) % 624] ^ (y >> 1) ^ (0x9908B0DF if y & 1 else 0)
            self.idx = 0
        y = self.mt[self.idx]
        self.idx += 1
        y ^= y >> 11
        y ^= (y << 7) & 0x9D2C5680
        y ^= (y << 15) & 0xEFC60000
        y ^= y >> 18
        return y


def sample_quintuples(seed, n, n_trials):
    g, idx, out = MT19937(seed), list(range(n)), np.zeros((n_trials, 5), np.int32)
    for t in range(n_trials):
        for i in range(5):
            m = n - i
            s = 0xFFFFFFFF // m
            while True:
                x = g.next()
                if x < m * s:
                    break
            j = i + x // s
            idx[i], idx[j] = idx[j], idx[i]
        out[t] = idx[:5]
    return out


def bound_row(n, confidence):
    """ceil(log(1 - confidence) / log(1 - (k / n)^5)) for k = 0 .. n; NaN, -inf and anything past int32 are 'unbounded'"""
    log = lambda v: np.float64(math.log(v)) if v > 0.0 else np.float64(-np.inf)            # (C's log(0) = -inf)
    row, K = [], log(1.0 - confidence)
    with np.errstate(all="ignore"):
        for k in range(n + 1):
            N = K / log(1.0 - math.pow(k / n, 5))                                            # IEEE division: inf and NaN as in C
            row.append(UNBOUNDED if (N != N or N < 0.0 or np.ceil(N) >= UNBOUNDED) else int(np.ceil(N)))
    return row


# ---------------------------------------------------------------------------------------------------- geometry
QL_T = np.array([0, 1, 4, 10, 1, 2, 5, 11, 2, 3, 6, 12, 4, 5, 7, 13, 5, 6, 8, 14, 7, 8, 9, 15, 10, 11, 13, 16, 11, 12, 14, 17, 13, 14, 15, 18,
                 16, 17, 18, 19])          # cubic index of (quadratic monomial, linear monomial), row-major


def _scale(T):
    return float(np.finfo(T).eps) / 2.0 ** -52


def lin_lin(a, b):
    return np.array([a[0] * b[0], a[0] * b[1] + a[1] * b[0], a[1] * b[1], a[0] * b[2] + a[2] * b[0], a[1] * b[2] + a[2] * b[1], a[2] * b[2],
                     a[0] * b[3] + a[3] * b[0], a[1] * b[3] + a[3] * b[1], a[2] * b[3] + a[3] * b[2], a[3] * b[3]], a.dtype)


def quad_lin(q, l):
    out = np.zeros(20, q.dtype)
    np.add.at(out, QL_T, np.outer(q, l).ravel())
    return out


def _jacobi_columns(A, V, tol, floor_abs, sweeps):
    """one-sided Jacobi on the columns of A (rotations accumulated in V), cyclic, in place"""
    n = A.shape[1]
    for _ in range(sweeps):
        rotated = False
        for p in range(n - 1):
            for q in range(p + 1, n):
                ap, aq = A[:, p], A[:, q]
                al, be, ga = ap @ ap, aq @ aq, ap @ aq
                if abs(ga) > tol * np.sqrt(al * be) and abs(ga) > floor_abs:
                    rotated = True
                    zeta = (be - al) / (2 * ga)
                    t = np.copysign(1, zeta) / (abs(zeta) + np.sqrt(1 + zeta * zeta))
                    c = 1 / np.sqrt(1 + t * t)
                    s = c * t
                    A[:, p], A[:, q] = c * ap - s * aq, s * ap + c * aq
                    vp, vq = V[:, p].copy(), V[:, q].copy()
                    V[:, p], V[:, q] = c * vp - s * vq, s * vp + c * vq
        if not rotated:
            break


def null_basis(pts, T):
    """pts [5][4] -> B [9][4]: the coefficients (x, y, z, 1) of E's entries, row-major"""
    A = np.zeros((5, 9), T)
    for i in range(5):
        p1 = np.array([pts[i, 0], pts[i, 1], 1], T)
        p2 = np.array([pts[i, 2], pts[i, 3], 1], T)
        A[i] = np.outer(p1, p2).ravel()
    V = np.eye(9, dtype=T)
    sc = _scale(T)
    _jacobi_columns(A, V, T(1e-15) * T(sc), T(2.0 ** -60) * T(sc) * (A * A).sum(), 30)
    norms = [A[:, c] @ A[:, c] for c in range(9)]
    used, picks = set(), []
    for b in range(4):
        pick = -1
        for c in range(9):
            if c not in used and (pick < 0 or norms[c] < norms[pick]):
                pick = c
        used.add(pick)
        picks.append(pick)
    N = V[:, picks]
    W = [N @ N[k] for k in range(4)]                     # the canonical basis: e0..e3 projected onto the null space, orthonormalised
    for k in range(4):
        for j in range(k):
            W[k] = W[k] - (W[j] @ W[k]) * W[j]
        W[k] = W[k] * (1 / np.sqrt(W[k] @ W[k]))
    B = np.zeros((9, 4), T)
    for b in range(4):
        for i in range(3):
            for j in range(3):
                B[3 * i + j, b] = W[b][3 * j + i]
    return B


def polynomials(B):
    T = B.dtype.type
    e = lambda i, j: B[3 * i + j]
    P = np.zeros((10, 20), T)
    minors = [lin_lin(e(1, 1), e(2, 2)) - lin_lin(e(1, 2), e(2, 1)), lin_lin(e(1, 2), e(2, 0)) - lin_lin(e(1, 0), e(2, 2)),
              lin_lin(e(1, 0), e(2, 1)) - lin_lin(e(1, 1), e(2, 0))]
    for j in range(3):
        P[9] += quad_lin(minors[j], e(0, j))
    Q = [[sum((lin_lin(e(i, j), e(k, j)) for j in range(3)), np.zeros(10, T)) for k in range(3)] for i in range(3)]
    h = T(0.5) * (Q[0][0] + Q[1][1] + Q[2][2])
    for i in range(3):
        Q[i][i] = Q[i][i] - h
    for i in range(3):
        for j in range(3):
            for k in range(3):
                P[3 * i + j] += quad_lin(Q[i][k], e(k, j))
    return P


def action_matrix(P):
    T = P.dtype.type
    perm = list(range(10))
    for i in range(10):
        for j in range(i + 1, 10):
            if abs(P[perm[i], i]) < abs(P[perm[j], i]):
                perm[i], perm[j] = perm[j], perm[i]
        if P[perm[i], i] == 0:
            continue
        P[perm[i]] = P[perm[i]] / P[perm[i], i]
        for j in range(i + 1, 10):
            P[perm[j]] = P[perm[j]] - P[perm[i]] * P[perm[j], i]
    for i in range(9, 0, -1):
        for j in range(i):
            P[perm[j]] = P[perm[j]] - P[perm[i]] * P[perm[j], i]
    A = np.zeros((10, 10), T)
    for r, src in enumerate((0, 1, 2, 4, 5, 7)):
        A[r] = -P[perm[src], 10:]
    A[6, 0] = A[7, 1] = A[8, 3] = A[9, 6] = 1
    return A


def _csqrt(z):
    T = type(z.real)
    m = np.sqrt(z.real * z.real + z.imag * z.imag)
    re = np.sqrt(T(0.5) * (m + abs(z.real)))
    if re == 0:
        return z * 0
    im = z.imag / (2 * re)
    return (re + 1j * im) if z.real >= 0 else (abs(im) + 1j * np.copysign(re, z.imag))


def real_eigenvalues(A):
    """Householder-Hessenberg, complex single-shift QR with deflation; None when the cap of 30 iterations per value is hit"""
    T = A.dtype.type
    CT = np.clongdouble if T is np.longdouble else np.complex128
    eps = T(np.finfo(T).eps)
    n = 10
    H = A.copy()
    for k in range(n - 2):
        x = H[k + 1:, k].copy()
        nn = x @ x
        alpha = -np.sqrt(nn) if x[0] > 0 else np.sqrt(nn)
        v = x
        v[0] = v[0] - alpha
        vv = v @ v
        if vv == 0:
            continue
        beta = 2 / vv
        H[k + 1:, :] -= np.outer(v, beta * (v @ H[k + 1:, :]))
        H[:, k + 1:] -= np.outer(beta * (H[:, k + 1:] @ v), v)
        H[k + 2:, k] = 0
    hnorm = np.abs(H).sum()
    H = H.astype(CT)
    a1 = lambda z: abs(z.real) + abs(z.imag)
    a2 = lambda z: z.real * z.real + z.imag * z.imag
    hi, its = n - 1, 0
    while hi >= 0:
        lo = hi
        while lo > 0:
            s = a1(H[lo - 1, lo - 1]) + a1(H[lo, lo])
            if s == 0:
                s = hnorm
            if a1(H[lo, lo - 1]) <= eps * s:
                H[lo, lo - 1] = 0
                break
            lo -= 1
        if lo == hi:
            hi -= 1
            its = 0
            continue
        if its >= 30:
            return None
        its += 1
        a, b, c, d = H[hi - 1, hi - 1], H[hi - 1, hi], H[hi, hi - 1], H[hi, hi]
        if its in (10, 20):
            mu = d + a1(c)
        else:
            h, bc = (a - d) * T(0.5), b * c
            sq = _csqrt(h * h + bc)
            dp, dm = h + sq, h - sq
            den = dp if a2(dp) >= a2(dm) else dm
            mu = d if a2(den) == 0 else d - bc / den
        idx = np.arange(lo, hi + 1)
        H[idx, idx] -= mu
        rots = []
        for k in range(lo, hi):
            x, y = H[k, k], H[k + 1, k]
            c1, s1 = T(1), CT(0)
            if a2(y) != 0:
                ax, nrm = np.sqrt(a2(x)), np.sqrt(a2(x) + a2(y))
                if ax == 0:
                    c1, s1 = T(0), np.conj(y) / np.sqrt(a2(y))
                else:
                    c1, s1 = ax / nrm, (x / ax) * np.conj(y) / nrm
            u, v = H[k, k:hi + 1].copy(), H[k + 1, k:hi + 1].copy()
            H[k, k:hi + 1], H[k + 1, k:hi + 1] = c1 * u + s1 * v, c1 * v - np.conj(s1) * u
            H[k + 1, k] = 0
            rots.append((c1, s1))
        for k in range(lo, hi):                      # (left and right rotations commute: the same products as the interleaved form)
            c1, s1 = rots[k - lo]
            u, v = H[lo:k + 2, k].copy(), H[lo:k + 2, k + 1].copy()
            H[lo:k + 2, k], H[lo:k + 2, k + 1] = c1 * u + v * np.conj(s1), c1 * v - u * s1
        H[idx, idx] += mu
    lam = [H[k, k] for k in range(n)]
    return sorted(T(z.real) for z in lam if abs(z.imag) < 1e-10 and np.isfinite(z.real))


def model_of(A, B, lam):
    T = A.dtype.type
    M = A - lam * np.eye(10, dtype=T)
    with np.errstate(all="ignore"):
        for k in range(9):
            p = k + int(np.argmax(np.abs(M[k:, k])))
            if p != k:
                M[[k, p]] = M[[p, k]]
            f = M[k + 1:, k] / M[k, k]
            M[k + 1:, k:] -= np.outer(f, M[k, k:])
        h = np.zeros(10, T)
        h[9] = 1
        for r in range(8, -1, -1):
            h[r] = -(M[r, r + 1:] @ h[r + 1:]) / M[r, r]
        x = np.array([h[6] / h[9], h[7] / h[9], h[8] / h[9], 1], T)
        E = B @ x
    return E if np.isfinite(E).all() else None


def five_point_models(pts, T):
    B = null_basis(np.asarray(pts, T), T)
    A = action_matrix(polynomials(B))
    lams = real_eigenvalues(A)
    if lams is None:
        return []
    return [E for E in (model_of(A, B, lam) for lam in lams) if E is not None]


def sampson(E, xa, xb):
    """E [9] row-major, xa, xb [n][2] -> se [n]"""
    with np.errstate(all="ignore"):
        x1, y1, x2, y2 = xa[:, 0], xa[:, 1], xb[:, 0], xb[:, 1]
        a0, a1, a2 = E[0] * x1 + E[1] * y1 + E[2], E[3] * x1 + E[4] * y1 + E[5], E[6] * x1 + E[7] * y1 + E[8]
        b0, b1 = E[0] * x2 + E[3] * y2 + E[6], E[1] * x2 + E[4] * y2 + E[7]
        r = x2 * a0 + y2 * a1 + a2
        return r * r * (1 / (a0 * a0 + a1 * a1) + 1 / (b0 * b0 + b1 * b1))


def support(E, xa, xb, th2):
    se = sampson(E, xa, xb)
    with np.errstate(all="ignore"):
        score = np.cumsum(np.log(1 + se * se / th2))[-1]           # (sequential, in index order)
    return int((se < th2).sum()), score


SIGN_E = (0.31, -0.17, 0.23, 0.41, 0.13, -0.29, 0.19, 0.37, 0.11)
ORIENT = (0.6, 0.48, 0.64)


def decompose_essential(E):
    T = E.dtype.type
    sg = -1 if (E @ np.asarray(SIGN_E, T)) < 0 else 1
    a, v = sg * E.reshape(3, 3), np.eye(3, dtype=T)
    sc = _scale(T)
    for _ in range(20):
        rotated = False
        for p, q in ((0, 1), (0, 2), (1, 2)):
            ap, aq = a[:, p].copy(), a[:, q].copy()
            al, be, ga = ap @ ap, aq @ aq, ap @ aq
            if abs(ga) > T(1e-15) * T(sc) * np.sqrt(al * be):
                rotated = True
                zeta = (be - al) / (2 * ga)
                t = np.copysign(1, zeta) / (abs(zeta) + np.sqrt(1 + zeta * zeta))
                c = 1 / np.sqrt(1 + t * t)
                s = c * t
                a[:, p], a[:, q] = c * ap - s * aq, s * ap + c * aq
                vp, vq = v[:, p].copy(), v[:, q].copy()
                v[:, p], v[:, q] = c * vp - s * vq, s * vp + c * vq
        if not rotated:
            break
    nn = [a[:, c] @ a[:, c] for c in range(3)]
    drop = 0 if (nn[0] <= nn[1] and nn[0] <= nn[2]) else (1 if nn[1] <= nn[2] else 2)
    keep = [c for c in range(3) if c != drop]
    u1, u2 = a[:, keep[0]] / np.sqrt(nn[keep[0]]), a[:, keep[1]] / np.sqrt(nn[keep[1]])
    v1, v2 = v[:, keep[0]], v[:, keep[1]]
    u3, v3 = np.cross(u1, u2), np.cross(v1, v2)
    o = -1 if (v3 @ np.asarray(ORIENT, T)) < 0 else 1
    u3, v3, u1, v1 = o * u3, o * v3, o * u1, o * v1
    tw, ax = np.outer(u1, v2) - np.outer(u2, v1), np.outer(u3, v3)
    return tw + ax, ax - tw, u3


def null4_batch(a):
    """null vectors of a [m][4][4] by one-sided Jacobi, every matrix on its own (a matrix that is done gets identity rotations)"""
    T = a.dtype.type
    a = a.copy()
    m = len(a)
    v = np.broadcast_to(np.eye(4, dtype=T), (m, 4, 4)).copy()
    tol = T(1e-15) * T(_scale(T))
    with np.errstate(all="ignore"):
        for _ in range(12):
            any_rot = False
            for p in range(3):
                for q in range(p + 1, 4):
                    ap, aq = a[:, :, p].copy(), a[:, :, q].copy()
                    al, be, ga = (ap * ap).sum(1), (aq * aq).sum(1), (ap * aq).sum(1)
                    rot = np.abs(ga) > tol * np.sqrt(al * be)
                    if not rot.any():
                        continue
                    any_rot = True
                    zeta = (be - al) / (2 * np.where(rot, ga, 1))
                    t = np.copysign(1, zeta) / (np.abs(zeta) + np.sqrt(1 + zeta * zeta))
                    c = np.where(rot, 1 / np.sqrt(1 + t * t), 1)
                    s = np.where(rot, c * t, 0)
                    c, s = c[:, None], s[:, None]
                    a[:, :, p], a[:, :, q] = c * ap - s * aq, s * ap + c * aq
                    vp, vq = v[:, :, p].copy(), v[:, :, q].copy()
                    v[:, :, p], v[:, :, q] = c * vp - s * vq, s * vp + c * vq
            if not any_rot:
                break
    nn = (a * a).sum(1)                       # [m][4] column norms
    pick = np.argmin(nn, axis=1)              # (the first of equal ones, as the library's `<`)
    return v[np.arange(m), :, pick]


def check_points(R, t, xa, xb, max_depth):
    """-> (ok [n], p [n][3])"""
    T = R.dtype.type
    n = len(xa)
    a = np.zeros((n, 4, 4), T)
    a[:, 0, 0] = -1; a[:, 0, 2] = xa[:, 0]; a[:, 1, 1] = -1; a[:, 1, 2] = xa[:, 1]
    a[:, 2, :3] = xb[:, :1] * R[2] - R[0]; a[:, 2, 3] = xb[:, 0] * t[2] - t[0]
    a[:, 3, :3] = xb[:, 1:] * R[2] - R[1]; a[:, 3, 3] = xb[:, 1] * t[2] - t[1]
    q = null4_batch(a)
    with np.errstate(all="ignore"):
        q1z, q2z = q[:, 2], q[:, :3] @ R[2] + t[2] * q[:, 3]
        ok = (q1z * q[:, 3] > 0) & (q2z * q[:, 3] > 0) & (q1z / q[:, 3] < max_depth) & (q2z / q[:, 3] < max_depth)
        p = q[:, :3] / q[:, 3:]
    ok &= np.isfinite(p).all(1)
    return ok, p


def tri_angle(c2, p):
    """angle at p between the centres 0 and c2"""
    with np.errstate(all="ignore"):
        b2, r1 = c2 @ c2, (p * p).sum(1)
        d = p - c2
        r2 = (d * d).sum(1)
        den = 2 * np.sqrt(r1 * r2)
        ang = np.abs(np.arccos((r1 + r2 - b2) / np.where(den == 0, 1, den)))
        ang = np.minimum(ang, p.dtype.type(3.14159265358979323846) - ang)
    return np.where(den == 0, 0, ang)


def quat_of(R):
    T = R.dtype.type
    m = R
    tr = m[0, 0] + m[1, 1] + m[2, 2]
    if tr > 0:
        s = np.sqrt(tr + 1) * 2; w = s / 4; x = (m[2, 1] - m[1, 2]) / s; y = (m[0, 2] - m[2, 0]) / s; z = (m[1, 0] - m[0, 1]) / s
    elif m[0, 0] > m[1, 1] and m[0, 0] > m[2, 2]:
        s = np.sqrt(1 + m[0, 0] - m[1, 1] - m[2, 2]) * 2; w = (m[2, 1] - m[1, 2]) / s; x = s / 4; y = (m[0, 1] + m[1, 0]) / s; z = (m[0, 2] + m[2, 0]) / s
    elif m[1, 1] > m[2, 2]:
        s = np.sqrt(1 + m[1, 1] - m[0, 0] - m[2, 2]) * 2; w = (m[0, 2] - m[2, 0]) / s; x = (m[0, 1] + m[1, 0]) / s; y = s / 4; z = (m[1, 2] + m[2, 1]) / s
    else:
        s = np.sqrt(1 + m[2, 2] - m[0, 0] - m[1, 1]) * 2; w = (m[1, 0] - m[0, 1]) / s; x = (m[0, 2] + m[2, 0]) / s; y = (m[1, 2] + m[2, 1]) / s; z = s / 4
    q = np.array([x, y, z, w], T)
    return q * ((-1 if w < 0 else 1) / np.sqrt(q @ q))


def quat_to_mat(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], q.dtype)


# ---------------------------------------------------------------------------------------------------- one pair
def solve_pair(xa, xb, th, opt, precision="longdouble"):
    """-> dict(status, E [9] unit norm, R, q, t, points, essential_mask, front_mask, counts [8], accepted, num_trials, best_trial,
    records [(trial, slot, count, score)] (slot -1: a trial without a model), nmodels [per executed trial], lowered)"""
    with np.errstate(all="ignore"):
        return _solve_pair(xa, xb, th, opt, precision)


def _solve_pair(xa, xb, th, opt, precision):
    T = np.longdouble if precision == "longdouble" else np.float64
    n = len(xa)
    out = dict(status=0, E=None, R=None, q=None, t=None, points=np.zeros((n, 3), T), essential_mask=np.zeros(n, np.uint8),
               front_mask=np.zeros(n, np.uint8), counts=np.zeros(8, np.int32), accepted=0, num_trials=0, best_trial=-1, records=[], nmodels=[],
               lowered=False, n=n)
    if n < opt.min_matches or n > MAX_MATCHES:
        out["status"] = 2 if n < opt.min_matches else 3
        return out
    xa, xb = np.asarray(xa, T), np.asarray(xb, T)
    th2 = 2 * T(th) * T(th)
    row, quint = bound_row(n, opt.confidence), sample_quintuples(opt.seed, n, opt.max_iterations)
    bound, best_count, best_score, best_code, best_E = opt.max_iterations, 0, None, -1, None
    t = 0
    while t < bound:
        i5 = quint[t]
        models = five_point_models(np.concatenate([xa[i5], xb[i5]], axis=1), T)
        out["nmodels"].append(len(models))
        if not models:
            out["records"].append((t, -1, 0, 0.0))
        for slot, E in enumerate(models):
            cnt, score = support(E, xa, xb, th2)
            out["records"].append((t, slot, cnt, float(score)))
            if cnt > best_count or (cnt == best_count and best_count > 0 and score < best_score):
                best_count, best_score, best_code, best_E = cnt, score, t * SLOT_STRIDE + slot, E
                if row[cnt] < bound:
                    bound = row[cnt]
                    out["lowered"] = True
        t += 1
    out["num_trials"], out["best_trial"] = t, best_code
    if best_E is None:
        return out
    En = best_E / np.sqrt(best_E @ best_E)
    R1, R2, Tv = decompose_essential(En)
    if not (np.isfinite(En).all() and np.isfinite(R1).all() and np.isfinite(R2).all()):
        out["num_trials"], out["best_trial"] = t, best_code
        return out
    out["E"] = En
    out["essential_mask"] = (sampson(best_E, xa, xb) < th2).astype(np.uint8)
    out["counts"][0] = best_count
    cands = [(R1, Tv), (R1, -Tv), (R2, Tv), (R2, -Tv)]
    res = [check_points(R, tt, xa, xb, T(opt.max_depth)) for R, tt in cands]
    best_k, best_num = 0, 0
    for k in range(4):
        c = int(res[k][0].sum())
        if c > best_num:
            best_num, best_k = c, k
    out["front_counts"] = [int(r[0].sum()) for r in res]
    if best_num == 0:
        return out
    R, tt = cands[best_k]
    ok, p = res[best_k]
    out.update(status=1, R=R, t=tt, q=quat_of(R), front_mask=ok.astype(np.uint8))
    out["points"][ok] = p[ok]
    ang = tri_angle(-(R.T @ tt), p[ok])
    out["angles"] = ang
    out["counts"][1], out["counts"][2] = best_num, best_k
    for a, amin in enumerate(opt.min_angle_rad):
        nv = int((ang > T(amin)).sum())
        out["counts"][4 + a] = nv
        if best_num >= opt.min_front_ratio * n and nv >= opt.min_angle_ratio * best_num and nv > opt.min_num_valid:
            out["accepted"] |= 1 << a
    return out


DISCRETE = ("status", "num_trials", "best_trial", "accepted")


def same_discrete(a, b):
    return (all(int(a[k]) == int(b[k]) for k in DISCRETE) and np.array_equal(np.asarray(a["counts"]), np.asarray(b["counts"])) and
            np.array_equal(a["essential_mask"], b["essential_mask"]) and np.array_equal(a["front_mask"], b["front_mask"]))


# ---------------------------------------------------------------------------------------------------- the catalogue
def _rot(axis, ang):
    axis = np.asarray(axis, float) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + math.sin(ang) * K + (1 - math.cos(ang)) * K @ K


def make_pair(n, outliers, noise_px, baseline, seed, depth=(5.0, 7.0), forward=False, planar=False, rotation_only=False):
    """two views of n points: frame 1 at the identity, frame 2 = (R, t) with |t| = 1 and the scene scaled so that the baseline is
    `baseline` scene units at depths `depth`; -> xa, xb, R, t"""
    rng = np.random.default_rng(seed)
    s = 1.0 / baseline                                         # scene scale: the baseline becomes 1
    X = np.stack([rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(depth[0], depth[1], n)], 1) * s
    if planar:
        X[:, 2] = (6.0 + 0.2 * X[:, 0] / s) * s
    R = _rot([0.1, 1.0, 0.05], -0.08 if not forward else 0.02)
    c2 = np.array([0.0, 0.02, 1.0]) if forward else np.array([1.0, 0.03, 0.05])
    c2 = c2 / np.linalg.norm(c2)
    if rotation_only:
        c2 = c2 * 0.0
    t = -R @ c2
    Y = X @ R.T + t
    xa, xb = X[:, :2] / X[:, 2:], Y[:, :2] / Y[:, 2:]
    if noise_px:
        xa = xa + rng.normal(0, noise_px / FX, xa.shape)
        xb = xb + rng.normal(0, noise_px / FX, xb.shape)
    n_out = int(round(outliers * n))
    if n_out:
        idx = rng.permutation(n)[:n_out]
        xb[idx] = np.stack([rng.uniform(-0.5, 0.5, n_out), rng.uniform(-0.4, 0.4, n_out)], 1)
    return np.ascontiguousarray(xa), np.ascontiguousarray(xb), R, t


LENGTHS = (10, 11, 63, 64, 65, 255, 256, 257, 300, 1000)
BASELINES = dict(wide=2.2, mid=1.25, narrow=0.3)               # passes 16 deg, passes only 8 deg, passes neither (depths 5..7)


@functools.lru_cache(maxsize=None)
def catalogue():
    """-> (main, degenerate): lists of dict(tag, xa, xb, th, opt (dict of overrides), R, t)"""
    main, seed = [], 100
    kinds = ("wide", "mid", "narrow")
    for li, n in enumerate(LENGTHS):
        for si, share in enumerate((0.0, 0.2, 0.6)):
            for variant in range(2):
                seed += 1
                kind = kinds[(li + si + variant) % 3]
                # a noise-free pair with outliers is fragile by construction (exact models tie on the inlier count and their scores
                # differ by rounding only): those sit in the degenerate list
                noise = 0.0 if (share == 0.0 and variant == 0) else 0.5
                opt = {} if (variant == 0 and n >= 300) else dict(min_num_valid=20)
                if share == 0.6 and n < 255:
                    opt["max_iterations"] = 24 if variant else 40
                xa, xb, R, t = make_pair(n, share, noise, BASELINES[kind], seed)
                main.append(dict(tag="n%d_s%g_%s_v%d" % (n, share, kind, variant), xa=xa, xb=xb, th=TH, opt=opt, R=R, t=t))
    def add(tag, opt=None, th=TH, **kw):
        nonlocal seed
        seed += 1
        xa, xb, R, t = make_pair(seed=seed, **kw)
        main.append(dict(tag=tag, xa=xa, xb=xb, th=th, opt=opt or {}, R=R, t=t))
    add("forward", n=300, outliers=0.2, noise_px=0.5, baseline=2.0, forward=True)
    add("maxit1", dict(max_iterations=1), n=300, outliers=0.2, noise_px=0.5, baseline=2.2)
    add("maxit64", dict(max_iterations=64), n=65, outliers=0.6, noise_px=0.5, baseline=2.2)
    add("bound_drops", n=300, outliers=0.2, noise_px=0.5, baseline=2.2)
    add("accept16", n=600, outliers=0.2, noise_px=0.5, baseline=2.2)
    add("accept8", n=600, outliers=0.2, noise_px=0.5, baseline=1.25)
    add("reject", n=600, outliers=0.2, noise_px=0.5, baseline=0.3)
    add("too_few", n=7, outliers=0.0, noise_px=0.0, baseline=2.2)
    add("seed7", dict(seed=7), n=257, outliers=0.2, noise_px=0.5, baseline=2.2)
    add("wide_threshold", th=20.0 / FX, n=256, outliers=0.2, noise_px=0.5, baseline=1.25)
    too_many = np.zeros((MAX_MATCHES + 1, 2))
    main.append(dict(tag="too_many", xa=too_many, xb=too_many.copy(), th=TH, opt={}, R=None, t=None))
    deg = []
    def addd(tag, opt=None, xform=None, **kw):
        nonlocal seed
        seed += 1
        xa, xb, R, t = make_pair(seed=seed, **kw)
        if xform:
            xa, xb = xform(xa, xb)
        deg.append(dict(tag=tag, xa=xa, xb=xb, th=TH, opt=opt or {}, R=R, t=t))
    addd("n5", dict(min_matches=5, min_num_valid=2), n=5, outliers=0.0, noise_px=0.5, baseline=2.2)
    addd("n6", dict(min_matches=5, min_num_valid=2), n=6, outliers=0.0, noise_px=0.5, baseline=2.2)
    addd("pure_rotation", dict(min_num_valid=20), n=64, outliers=0.0, noise_px=0.5, baseline=1.0, rotation_only=True)
    addd("planar", dict(min_num_valid=20), n=100, outliers=0.0, noise_px=0.5, baseline=2.2, planar=True)
    rng = np.random.default_rng(5)
    deg.append(dict(tag="outliers_only", xa=rng.uniform(-0.5, 0.5, (64, 2)), xb=rng.uniform(-0.5, 0.5, (64, 2)), th=TH, opt=dict(min_num_valid=20), R=None, t=None))
    addd("duplicated", dict(min_num_valid=20), xform=lambda a, b: (np.ascontiguousarray(np.repeat(a[:8], 8, 0)), np.ascontiguousarray(np.repeat(b[:8], 8, 0))),
         n=64, outliers=0.0, noise_px=0.5, baseline=2.2)
    addd("nothing_in_front", dict(max_depth=1e-9), n=64, outliers=0.0, noise_px=0.5, baseline=2.2)       # status 0 with an E
    # coordinates whose products overflow float64: every trial ends without a model and best_E stays NaN (status 0 without an E).
    # The extended run does not overflow and finds models, so this pair differs between the precisions by construction.
    addd("overflow", dict(max_iterations=3), xform=lambda a, b: (a * 1e160, b * 1e160), n=12, outliers=0.0, noise_px=0.5, baseline=2.2)
    addd("exact_with_outliers", dict(min_num_valid=20), n=64, outliers=0.2, noise_px=0.0, baseline=2.2)
    addd("exact_with_outliers_300", n=300, outliers=0.6, noise_px=0.0, baseline=2.2, opt=dict(max_iterations=16))
    return main, deg


def entries():
    main, deg = catalogue()
    return main + deg


def n_main():
    return len(catalogue()[0])


def arrays(idx):
    """the flat arrays of a call over the catalogue entries idx (all must share their options): match_ptr, xy_a, xy_b, thresholds"""
    E = entries()
    ptr = np.zeros(len(idx) + 1, np.int32)
    for i, k in enumerate(idx):
        ptr[i + 1] = ptr[i] + len(E[k]["xa"])
    xa = np.concatenate([E[k]["xa"] for k in idx]) if idx else np.zeros((0, 2))
    xb = np.concatenate([E[k]["xb"] for k in idx]) if idx else np.zeros((0, 2))
    return ptr, np.ascontiguousarray(xa), np.ascontiguousarray(xb), np.array([E[k]["th"] for k in idx])


def option_groups():
    """catalogue indices grouped by their option overrides (one library call per group)"""
    groups = {}
    for k, e in enumerate(entries()):
        groups.setdefault(tuple(sorted(e["opt"].items())), []).append(k)
    return groups


@functools.lru_cache(maxsize=None)
def reference(precision="longdouble"):
    return [solve_pair(e["xa"], e["xb"], e["th"], Options(**e["opt"]), precision) for e in entries()]


@functools.lru_cache(maxsize=None)
def fragile():
    """per entry: the two precisions disagree on a discrete output, or one of three float64 reruns with every coordinate perturbed
    by a relative 2^-43 does"""
    ext, f64, out = reference("longdouble"), reference("float64"), []
    for k, e in enumerate(entries()):
        bad = not same_discrete(ext[k], f64[k])
        if not bad and ext[k]["status"] < 2:
            for rerun in range(3):
                rng = np.random.default_rng(9000 + 10 * k + rerun)
                pa = e["xa"] * (1 + rng.choice([-1.0, 1.0], e["xa"].shape) * 2.0 ** -43)
                pb = e["xb"] * (1 + rng.choice([-1.0, 1.0], e["xb"].shape) * 2.0 ** -43)
                if not same_discrete(solve_pair(pa, pb, e["th"], Options(**e["opt"]), "float64"), f64[k]):
                    bad = True
                    break
        out.append(bad)
    return out


def fragile_share():
    return sum(fragile()[:n_main()]) / n_main()


# ---------------------------------------------------------------------------------------------------- the checks
def det_and_trace(E):
    """|det E| and ||2 E E' E - tr(E E') E|| of a unit-norm E, in extended precision"""
    M = np.asarray(E, np.longdouble).reshape(3, 3)
    EEt = M @ M.T
    det = (M[0, 0] * (M[1, 1] * M[2, 2] - M[1, 2] * M[2, 1]) - M[0, 1] * (M[1, 0] * M[2, 2] - M[1, 2] * M[2, 0]) +
           M[0, 2] * (M[1, 0] * M[2, 1] - M[1, 1] * M[2, 0]))
    return float(abs(det)), float(np.sqrt(((2 * EEt @ M - np.trace(EEt) * M) ** 2).sum()))


def deviations(got, ext):
    """got: dict(E [9], R [3][3] or q, t, points, front_mask) of a status-1 result; -> dict of deviations from the extended run"""
    L = np.longdouble
    E, Ee = np.asarray(got["E"], L).ravel(), ext["E"]
    E = E / np.sqrt(E @ E)
    R = np.asarray(got["R"], L) if got.get("R") is not None else quat_to_mat(np.asarray(got["q"], L))
    m = ext["front_mask"].astype(bool)
    p, pe = np.asarray(got["points"], L)[m], ext["points"][m]
    d, tr = det_and_trace(E)
    de, tre = det_and_trace(Ee)
    return dict(E=float(min(np.abs(E - Ee).max(), np.abs(E + Ee).max())), R=float(np.abs(R - ext["R"]).max()),
                t=float(np.abs(np.asarray(got["t"], L) - ext["t"]).max()),
                points=float((np.abs(p - pe) / (1 + np.abs(pe))).max()) if m.any() else 0.0, det=abs(d - de), trace=abs(tr - tre))


def loose_ok(got, ext):
    """rtol 1e-6 / atol 1e-9 on E (up to sign), R, t and the points where front_mask"""
    f = lambda a: np.asarray(a, np.float64)
    E, Ee = f(got["E"]).ravel(), f(ext["E"])
    E = E / np.linalg.norm(E)
    R = f(got["R"]) if got.get("R") is not None else f(quat_to_mat(np.asarray(got["q"], np.longdouble)))
    m = ext["front_mask"].astype(bool)
    close = lambda a, b: np.allclose(a, b, rtol=1e-6, atol=1e-9)
    return (close(E, Ee) or close(-E, Ee)) and close(R, f(ext["R"])) and close(f(got["t"]), f(ext["t"])) and close(f(got["points"])[m], f(ext["points"])[m])


def always_true(got, xa, xb, th):
    """the properties every result has, degenerate pairs included; got: status, E, q, t, points, essential_mask, front_mask, counts.
    Returns the list of violated properties."""
    bad, L = [], np.longdouble
    st = int(got["status"])
    if st == 1 or (st == 0 and int(got["best_trial"]) >= 0 and got["E"] is not None and np.any(np.asarray(got["E"], np.float64) != 0)):
        E = np.asarray(got["E"], L).ravel()
        if not np.isfinite(np.asarray(E, np.float64)).all():
            bad.append("E not finite")
        if abs(float(E @ E) - 1.0) > 32 * 2.0 ** -53:
            bad.append("|E| != 1")
        se = sampson(E, np.asarray(xa, L), np.asarray(xb, L))
        th2 = 2 * L(th) * L(th)
        with np.errstate(all="ignore"):
            near = np.abs(se - th2) <= 1e-8 * th2
        want = (se < th2)
        if not np.array_equal(want[~near], np.asarray(got["essential_mask"]).astype(bool)[~near]):
            bad.append("essential_mask is not the Sampson test of the returned E")
        if int(np.asarray(got["essential_mask"]).sum()) != int(got["counts"][0]):
            bad.append("counts[0] is not the mask's sum")
    if st == 1:
        q = np.asarray(got["q"], L)
        if abs(float(q @ q) - 1.0) > 8 * 2.0 ** -53 or q[3] < 0:
            bad.append("|q|^2 != 1 or w < 0")
        m = np.asarray(got["front_mask"]).astype(bool)
        if not (np.isfinite(np.asarray(got["t"], np.float64)).all() and np.isfinite(np.asarray(got["points"], np.float64)[m]).all()):
            bad.append("t or points not finite")
        if int(m.sum()) != int(got["counts"][1]) or int(got["counts"][1]) == 0:
            bad.append("counts[1] is not the front mask's sum")
    else:
        if np.asarray(got["front_mask"]).any() or int(got["accepted"]) != 0:
            bad.append("front mask or accepted set without geometry")
    return bad


@functools.lru_cache(maxsize=None)
def restatement_deviation():
    ext, f64, fr, worst = reference("longdouble"), reference("float64"), fragile(), {k: 0.0 for k in RESTATEMENT_DEVIATION}
    for k in range(n_main()):
        if fr[k] or ext[k]["status"] != 1:
            continue
        for name, v in deviations(f64[k], ext[k]).items():
            worst[name] = max(worst[name], v)
    return worst
