"""Yardstick, catalogue and bars of the pair-verification tests (tests/test_fund_cpu.py, tests/test_gpu_fund.py).

The yardstick is a pure numpy restatement of the rule xrsfm_ba_verify_pairs restates (include/xrsfm_ba.h; the reference's
SolveFundamnetalCOLMAP -> colmap::LORANSAC<FundamentalMatrixSevenPointEstimator, FundamentalMatrixEightPointEstimator>),
parameterised by dtype and run in np.longdouble (x87 extended, asserted) and in np.float64.  MT19937, the Householder QR, the cubic
solver and the Jacobi routines are written by hand.  It is never the library and shares no code with it.

Rule.  Every pair gets a fresh MT19937 (init_genrand(seed)); the sampler keeps an index array across the trials of the pair and
does seven Fisher-Yates steps per trial (bounded draw for m = last - i + 1: s = 0xFFFFFFFF // m, draw words until x < m s,
at most 16 redraws, then x = m s - 1; j = i + x // s).  max_trials = min(max_num_trials, ComputeNumTrials(min_inlier_ratio 1e5, 1e5, confidence)) with exponent 7.  Per
trial: the 7 x 9 system on raw pixel coordinates; Householder QR of its transpose (reflector sign opposite to the pivot's),
g1 = Q e7, g2 = Q e8, f1 = g1 - g2, f2 = g2; the cubic det(lambda f1 + f2); leading zeros lower the degree; a cubic is made monic,
one real root found by 128 bisection steps on [-R, R], R = 1 + max |coefficient|, the deflated quadratic in closed form, two Newton
steps per real root on the original polynomial; a complex pair counts (real part, twice) when |Im| <= 1e-10; ascending roots;
a root is dropped when |F(2,2)| < 1e-10; F / F(2,2); non-finite models are dropped.  Residual: squared Sampson error.  Support =
(count, sum of inlier residuals in index order); a beats b iff count larger, or equal and sum strictly smaller; initial best
(0, DBL_MAX).  A model that beats the best becomes the best; with count >= 8 the 8-point model of its inliers (centred and scaled
to rms distance sqrt 2 per image, null vector of the 9 x 9 Gram matrix by cyclic Jacobi, rank 2 by dropping the smallest term of a
one-sided Jacobi SVD, T2' F T1) replaces it if its support beats it; dyn = ceil(log(1 - c) / log(1 - (k / n)^7)) (1 if the argument
is <= 0, unbounded if 1 - c <= 0 or k = 0), in float64 whatever the dtype; after every model, t >= dyn and t >= min_num_trials set
abort: the rest of the trial's models are skipped, the next trial, if the bound admits one, is counted and the scan stops.  Success
iff the best count >= 7; the mask is the inlier test of the returned model; accepted iff num_inliers >= max(min_num_inliers,
int(min_accept_ratio n)).  F is returned with unit Frobenius norm and its entry of largest magnitude positive.

Fragile pairs.  A pair is FRAGILE when the two precisions disagree on a discrete output (status, mask, num_inliers, num_trials,
best_trial, accepted), or when any of three seeded float64 reruns with every input coordinate perturbed by a relative 2^-43 changes
one.  At most FRAGILE_CAP of the main catalogue may be fragile: a condition on the catalogue, asserted in both test files.
Constructions that are fragile by design sit in the degenerate list, where only the always-true properties are checked.

Bars on non-fragile status-1 pairs of the main catalogue.  Loose: F within rtol 1e-6 / atol 1e-9 of the extended run.  Tight:
max |F - F_ext| <= TIGHT_BAR = 16 x RESTATEMENT_DEVIATION, the float64 restatement's own largest deviation over the catalogue
(asserted to be that in tests/test_fund_cpu.py); the factor 16 covers a different but equally valid operation order.
"""
import functools
import math

import numpy as np

EXT = np.longdouble
assert np.finfo(EXT).eps < 2e-19, "np.longdouble is not extended precision here"

DBL_MAX = float(np.finfo(np.float64).max)
MAX_MATCHES = 8192
MAX_TRIALS = 16384
LOCAL_BIT = 1 << 30
UNBOUNDED = 2 ** 31 - 1
CHUNK = 64
FRAGILE_CAP = 0.05
PERTURBATION = 2.0 ** -43
ROOT_MAX_IMAG = 1e-10
F22_EPS = 1e-10
BISECT = 128
MAX_REDRAWS = 16
POLISH = 2
TIGHT_FACTOR = 16
RESTATEMENT_DEVIATION = 4.4e-13  # measured: the float64 restatement against the extended run, largest over the catalogue (4.39e-13,
                                 # n15_s0, an 8-point model of 15 matches; tests/test_fund_cpu.py asserts the measurement)
TIGHT_BAR = TIGHT_FACTOR * RESTATEMENT_DEVIATION
BRANCHES = ("trial_without_model", "three_models", "local_wins", "local_loses", "abort_dyn", "cap_reached", "root_rejected_imag")


class Options:
    def __init__(self, **kw):
        self.max_error = 4.0
        self.confidence = 0.999
        self.min_inlier_ratio = 0.25
        self.min_num_trials = 100
        self.max_num_trials = 10000
        self.seed = 0
        self.min_matches = 15
        self.min_num_inliers = 15
        self.min_accept_ratio = 0.25
        for k, v in kw.items():
            assert hasattr(self, k), k
            setattr(self, k, v)


def num_trials_bound(k, n, confidence):
    nom = 1.0 - confidence
    if nom <= 0.0 or k <= 0:
        return UNBOUNDED
    denom = 1.0 - (k / float(n)) ** 7
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


class _Tuples:
    """the septuples of one (seed, n), drawn on demand"""
    def __init__(self, seed, n):
        self.g, self.idx, self.n, self.rows = MT19937(seed), list(range(n)), n, []

    def upto(self, n_trials):
        g, idx, last = self.g, self.idx, self.n - 1
        while len(self.rows) < n_trials:
            for i in range(7):
                m = last - i + 1
                s = 0xFFFFFFFF // m
                x = g.next()
                for _ in range(MAX_REDRAWS):
                    if x < m * s:
                        break
                    x = g.next()
                x = min(x, m * s - 1)
                j = i + x // s
                idx[i], idx[j] = idx[j], idx[i]
            self.rows.append(idx[:7])
        return self.rows


@functools.lru_cache(maxsize=None)
def _tuples(seed, n):
    return _Tuples(seed, n)


def sample_tuples(seed, n, n_trials):
    return np.array(_tuples(int(seed), int(n)).upto(n_trials)[:n_trials], np.int32).reshape(n_trials, 7)


# ---------------------------------------------------------------------------------------------------- small linear algebra
def _tols(dt):
    ext = np.dtype(dt) == np.dtype(EXT)
    return dict(rot=dt(1e-18 if ext else 1e-15), floor=dt(1e-21 if ext else 1e-18))


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


def rank2(A):
    """the 3x3 A with the smallest term of its singular value decomposition dropped (one-sided Jacobi: A V = U S)"""
    dt = A.dtype.type
    tol = _tols(dt)["rot"]
    A = A.copy()
    V = np.eye(3, dtype=A.dtype)
    for _ in range(20):
        rotated = False
        for p, q in ((0, 1), (0, 2), (1, 2)):
            al, be, ga = (A[:, p] ** 2).sum(), (A[:, q] ** 2).sum(), (A[:, p] * A[:, q]).sum()
            if not (abs(ga) > tol * np.sqrt(al * be)):
                continue
            rotated = True
            zeta = (be - al) / (2 * ga)
            t = np.copysign(dt(1), zeta) / (abs(zeta) + np.sqrt(1 + zeta * zeta))
            c = 1 / np.sqrt(1 + t * t)
            s = c * t
            for Z in (A, V):
                zp, zq = Z[:, p].copy(), Z[:, q].copy()
                Z[:, p], Z[:, q] = c * zp - s * zq, s * zp + c * zq
        if not rotated:
            break
    nn = (A ** 2).sum(0)
    drop = 0 if (nn[0] <= nn[1] and nn[0] <= nn[2]) else (1 if nn[1] <= nn[2] else 2)
    return sum(np.outer(A[:, i], V[:, i]) for i in range(3) if i != drop)


def seq_sum(a):
    """sum over axis 0 in index order"""
    return np.cumsum(a, axis=0)[-1]


# ---------------------------------------------------------------------------------------------------- geometry
def residuals(F, xa, xb):
    """squared Sampson error; F [..., 9] row-major with x_b' F x_a = 0; -> [..., n]"""
    with np.errstate(all="ignore"):
        f = [F[..., k, None] for k in range(9)]
        x0, y0, x1, y1 = xa[:, 0], xa[:, 1], xb[:, 0], xb[:, 1]
        Fx0 = f[0] * x0 + f[1] * y0 + f[2]
        Fx1 = f[3] * x0 + f[4] * y0 + f[5]
        Fx2 = f[6] * x0 + f[7] * y0 + f[8]
        Ft0 = f[0] * x1 + f[3] * y1 + f[6]
        Ft1 = f[1] * x1 + f[4] * y1 + f[7]
        e = x1 * Fx0 + y1 * Fx1 + Fx2
        return e * e / (Fx0 * Fx0 + Fx1 * Fx1 + Ft0 * Ft0 + Ft1 * Ft1)


def supports(res, max_res):
    with np.errstate(all="ignore"):
        inl = res <= max_res
    return inl.sum(-1), np.cumsum(np.where(inl, res, 0), axis=-1)[..., -1], inl


def _polish(c, r):
    with np.errstate(all="ignore"):
        for _ in range(POLISH):
            p = ((c[0] * r + c[1]) * r + c[2]) * r + c[3]
            d = (3 * c[0] * r + 2 * c[1]) * r + c[2]
            step = p / d
            r = np.where((d != 0) & np.isfinite(step), r - step, r)
    return r


def cubic_roots(c, flags):
    """c [4][T] -> per trial the ascending list of the roots taken"""
    dt = c.dtype.type
    T = c.shape[1]
    one = np.ones(T, c.dtype)
    with np.errstate(all="ignore"):
        cub = c[0] != 0
        c0s = np.where(cub, c[0], one)
        a, b, cc = c[1] / c0s, c[2] / c0s, c[3] / c0s
        R = 1 + np.maximum(np.abs(a), np.maximum(np.abs(b), np.abs(cc)))
        okc = cub & np.isfinite(R) & (np.abs(R) <= dt(DBL_MAX))
        lo, hi = -R, R.copy()
        for _ in range(BISECT):
            mid = 0.5 * (lo + hi)
            neg = ((mid + a) * mid + b) * mid + cc < 0
            lo, hi = np.where(neg, mid, lo), np.where(neg, hi, mid)
        r = _polish(c, 0.5 * (lo + hi))
        quad2 = ~cub & (c[1] != 0)
        c1s = np.where(quad2, c[1], one)
        B = np.where(cub, a + r, c[2] / c1s)
        Cq = np.where(cub, b + r * B, c[3] / c1s)
        quad = okc | quad2
        lin = ~cub & (c[1] == 0) & (c[2] != 0)
        disc = B * B - 4 * Cq
        real2 = quad & (disc >= 0)
        qq = -0.5 * (B + np.copysign(np.sqrt(np.where(disc >= 0, disc, 0)), B))
        q1 = _polish(c, qq)
        q2 = _polish(c, np.where(qq != 0, Cq / np.where(qq != 0, qq, one), 0))
        im = 0.5 * np.sqrt(np.where(disc < 0, -disc, 0))
        cpx = quad & (disc < 0) & (im <= dt(ROOT_MAX_IMAG))
        if (quad & (disc < 0) & ~cpx).any():
            flags.add("root_rejected_imag")
        linr = -c[3] / np.where(lin, c[2], one)
    out = []
    for t in range(T):
        rt = [r[t]] if okc[t] else []
        if real2[t]:
            rt += [q1[t], q2[t]]
        elif cpx[t]:
            rt += [-0.5 * B[t]] * 2
        if lin[t]:
            rt = [linr[t]]
        out.append(sorted(rt))
    return out


def seven_point_chunk(pts, flags):
    """pts [T, 7, 4] (x_a y_a x_b y_b) -> per trial the list of models (9 entries, row-major) in ascending root order"""
    T = len(pts)
    dtp = pts.dtype
    x0, y0, x1, y1 = (pts[:, :, k] for k in range(4))
    one = np.ones_like(x0)
    with np.errstate(all="ignore"):
        M = np.stack([x1 * x0, x1 * y0, x1, y1 * x0, y1 * y0, y1, x0, y0, one], 1)          # [T, 9 (row i), 7 (column j)]
        vn = np.zeros((T, 7), dtp)
        for j in range(7):
            nn = sum(M[:, i, j] * M[:, i, j] for i in range(j, 9))
            x = M[:, j, j]
            alpha = np.where(x > 0, -np.sqrt(nn), np.sqrt(nn))
            M[:, j, j] = x - alpha
            v = sum(M[:, i, j] * M[:, i, j] for i in range(j, 9))
            vn[:, j] = v
            ok = v > 0
            vs = np.where(ok, v, 1)
            for c in range(j + 1, 7):
                d = sum(M[:, i, j] * M[:, i, c] for i in range(j, 9))
                d = np.where(ok, 2 * d / vs, 0)
                for i in range(j, 9):
                    M[:, i, c] = M[:, i, c] - d * M[:, i, j]
        g = []
        for k in range(2):
            f = np.zeros((T, 9), dtp)
            f[:, 7 + k] = 1
            for j in range(6, -1, -1):
                ok = vn[:, j] > 0
                vs = np.where(ok, vn[:, j], 1)
                d = sum(M[:, i, j] * f[:, i] for i in range(j, 9))
                d = np.where(ok, 2 * d / vs, 0)
                for i in range(j, 9):
                    f[:, i] = f[:, i] - d * M[:, i, j]
            g.append(f)
        b = [g[1][:, k] for k in range(9)]
        a = [g[0][:, k] - g[1][:, k] for k in range(9)]
        t0, t1, t2 = a[4] * a[8] - a[5] * a[7], a[3] * a[8] - a[5] * a[6], a[3] * a[7] - a[4] * a[6]
        t3, t4, t5 = b[4] * b[8] - b[5] * b[7], b[3] * b[8] - b[5] * b[6], b[3] * b[7] - b[4] * b[6]
        c0 = a[0] * t0 - a[1] * t1 + a[2] * t2
        c1 = (b[0] * t0 - b[1] * t1 + b[2] * t2 - b[3] * (a[1] * a[8] - a[2] * a[7]) + b[4] * (a[0] * a[8] - a[2] * a[6]) -
              b[5] * (a[0] * a[7] - a[1] * a[6]) + b[6] * (a[1] * a[5] - a[2] * a[4]) - b[7] * (a[0] * a[5] - a[2] * a[3]) +
              b[8] * (a[0] * a[4] - a[1] * a[3]))
        c2 = (a[0] * t3 - a[1] * t4 + a[2] * t5 - a[3] * (b[1] * b[8] - b[2] * b[7]) + a[4] * (b[0] * b[8] - b[2] * b[6]) -
              a[5] * (b[0] * b[7] - b[1] * b[6]) + a[6] * (b[1] * b[5] - b[2] * b[4]) - a[7] * (b[0] * b[5] - b[2] * b[3]) +
              a[8] * (b[0] * b[4] - b[1] * b[3]))
        c3 = b[0] * t3 - b[1] * t4 + b[2] * t5
        cs = np.stack([c0, c1, c2, c3])
        valid = np.isfinite(cs.astype(np.float64)).all(0)
        roots = cubic_roots(np.where(valid, cs, 0), flags)
        A, Bv = np.stack(a, 1), np.stack(b, 1)
        models = []
        for t in range(T):
            ms = []
            if valid[t]:
                for lam in roots[t]:
                    F = lam * A[t] + Bv[t]
                    f8 = F[8]
                    if not (abs(f8) >= F22_EPS):
                        continue
                    m = F / f8
                    if np.isfinite(m.astype(np.float64)).all():
                        ms.append(m)
            models.append(ms)
        return models


def eight_point(xa, xb):
    """FundamentalMatrixEightPointEstimator::Estimate on the given matches (the inliers, in index order) -> model (9) or None"""
    dt = xa.dtype.type
    n = len(xa)
    with np.errstate(all="ignore"):
        ca, cb = seq_sum(xa) / n, seq_sum(xb) / n
        da, db = xa - ca, xb - cb
        sa = np.sqrt(dt(2)) / np.sqrt(seq_sum(da[:, 0] * da[:, 0] + da[:, 1] * da[:, 1]) / n)
        sb = np.sqrt(dt(2)) / np.sqrt(seq_sum(db[:, 0] * db[:, 0] + db[:, 1] * db[:, 1]) / n)
        pa, pb = sa * xa + (-sa * ca), sb * xb + (-sb * cb)
        one = np.ones(n, xa.dtype)
        r = np.stack([pb[:, 0] * pa[:, 0], pb[:, 0] * pa[:, 1], pb[:, 0], pb[:, 1] * pa[:, 0], pb[:, 1] * pa[:, 1], pb[:, 1], pa[:, 0], pa[:, 1], one], 1)
        G = seq_sum(r[:, :, None] * r[:, None, :])
        if not np.isfinite(G.astype(np.float64)).all():
            return None
        ev, V = jacobi_eig(G)
        Fp = rank2(V[:, int(np.argmin(ev))].reshape(3, 3))
        T1 = np.array([[sa, 0, -sa * ca[0]], [0, sa, -sa * ca[1]], [0, 0, 1]], xa.dtype)
        T2 = np.array([[sb, 0, -sb * cb[0]], [0, sb, -sb * cb[1]], [0, 0, 1]], xa.dtype)
        F = (T2.T @ (Fp @ T1)).ravel()
        return F if np.isfinite(F.astype(np.float64)).all() else None


def normalised(F):
    """unit Frobenius norm, the entry of largest magnitude (the first of them) positive"""
    F = np.asarray(F).ravel()
    big = int(np.argmax(np.abs(F)))
    return F * ((-1 if F[big] < 0 else 1) / np.sqrt((F * F).sum()))


# ---------------------------------------------------------------------------------------------------- the rule
def run_pair(xa, xb, opt=None, dtype=EXT, max_error=None, seed=None, want_records=False):
    """-> dict(status, mask, num_inliers, num_trials, best_trial, accepted, F (9, dtype, normalised) on status 1, flags, records)"""
    opt = opt or Options()
    dt = np.dtype(dtype).type
    n = len(xa)
    out = dict(status=0, mask=np.zeros(n, np.uint8), num_inliers=0, num_trials=0, best_trial=-1, accepted=0, F=None, flags=set(), records=[], nmodels=[])
    if n < opt.min_matches or n > MAX_MATCHES:
        out["status"] = 2 if n < opt.min_matches else 3
        return out
    xa, xb = np.asarray(xa, np.float64).astype(dtype), np.asarray(xb, np.float64).astype(dtype)
    m4 = np.concatenate([xa, xb], 1)
    me = dt(opt.max_error if max_error is None else max_error)
    max_res = me * me
    cap = trial_cap(opt)
    sd = int(opt.seed if seed is None else seed)
    flags = out["flags"]
    best_count, best_sum, best_trial, best_local, best_F = 0, dt(DBL_MAX), -1, False, None
    dyn, abort, num_trials = cap, False, cap
    beats = lambda ca, sa, cb, sb: ca > cb or (ca == cb and sa < sb)
    for t0 in range(0, cap, CHUNK):
        t1 = min(cap, t0 + CHUNK)
        sel = sample_tuples(sd, n, t1)[t0:t1]
        models = seven_point_chunk(m4[sel], flags)
        flat = [F for ms in models for F in ms]
        if flat:
            cnts, sums, _ = supports(residuals(np.stack(flat), xa, xb), max_res)
        k = 0
        for l, ms in enumerate(models):
            t = t0 + l
            out["nmodels"].append(len(ms))
            if not ms:
                flags.add("trial_without_model")
            if len(ms) == 3:
                flags.add("three_models")
            for F in ms:
                cnt, sm = int(cnts[k]), sums[k]
                k += 1
                rec = [t, cnt, float(sm), -2, 0.0]
                if beats(cnt, sm, best_count, best_sum):
                    best_count, best_sum, best_trial, best_local, best_F = cnt, sm, t, False, F
                    if cnt > 7 and cnt >= 8:
                        with np.errstate(all="ignore"):
                            inl = residuals(F, xa, xb) <= max_res
                        Fl = eight_point(xa[inl], xb[inl])
                        rec[3] = -1
                        if Fl is not None:
                            lc, ls, _ = supports(residuals(Fl, xa, xb), max_res)
                            rec[3], rec[4] = int(lc), float(ls)
                            if beats(int(lc), ls, best_count, best_sum):
                                best_count, best_sum, best_local, best_F = int(lc), ls, True, Fl
                                flags.add("local_wins")
                            else:
                                flags.add("local_loses")
                    dyn = num_trials_bound(best_count, n, opt.confidence)
                out["records"].append(rec)
                if t >= dyn and t >= opt.min_num_trials:
                    abort = True
                    num_trials = t + 2 if t + 1 < cap else t + 1
                    flags.add("abort_dyn")
                    out["abort_trial"] = t
                    break
            if abort:
                break
        if abort:
            break
    if not abort:
        flags.add("cap_reached")
    out["scan"] = dict(n=n, best_trial=best_trial, local=int(best_local), num_trials=num_trials, success=int(best_count >= 7))
    if not want_records:
        out["records"] = []
    if best_count < 7 or best_F is None:
        return out
    Fn = normalised(best_F)
    if not np.isfinite(Fn.astype(np.float64)).all():
        return out
    with np.errstate(all="ignore"):
        inl = residuals(best_F, xa, xb) <= max_res
    ninl = int(inl.sum())
    out.update(status=1, mask=inl.astype(np.uint8), num_inliers=ninl, num_trials=num_trials, best_trial=best_trial | (LOCAL_BIT if best_local else 0),
               accepted=int(ninl >= max(opt.min_num_inliers, int(opt.min_accept_ratio * n))), F=Fn)
    return out


# ---------------------------------------------------------------------------------------------------- the checks
DISCRETE = ("status", "num_inliers", "num_trials", "best_trial", "accepted")


def same_discrete(a, b):
    return all(int(a[k]) == int(b[k]) for k in DISCRETE) and np.array_equal(np.asarray(a["mask"]), np.asarray(b["mask"]))


def deviation(F, e):
    """of a returned F from the extended result e (both carry the sign convention)"""
    return float(np.abs(np.asarray(F, EXT).ravel() - e["F"]).max())


def loose_ok(F, e):
    return bool(np.allclose(np.asarray(F, np.float64).ravel(), np.asarray(e["F"], np.float64), rtol=1e-6, atol=1e-9))


def always_true(got, xa, xb, max_error, rel=1e-9):
    """the properties every result has, degenerate pairs included; got: status, F, mask, num_inliers, num_trials, best_trial,
    accepted.  Returns the list of violated properties."""
    bad = []
    st, mask = int(got["status"]), np.asarray(got["mask"])
    if st == 1:
        F = np.asarray(got["F"], EXT).ravel()
        if not np.isfinite(np.asarray(got["F"], np.float64)).all():
            return ["F not finite"]
        if abs(float(F @ F) - 1.0) > 32 * 2.0 ** -53:
            bad.append("|F| != 1")
        if not F[int(np.argmax(np.abs(F)))] > 0:
            bad.append("the largest entry of F is not positive")
        res = residuals(F, np.asarray(xa).astype(EXT), np.asarray(xb).astype(EXT))
        mr = EXT(max_error) ** 2
        with np.errstate(all="ignore"):
            clear = np.abs(res - mr) > rel * mr
            want = res <= mr
        if not np.array_equal(want[clear], mask.astype(bool)[clear]):
            bad.append("the mask is not the Sampson test of the returned F")
        if int(mask.sum()) != int(got["num_inliers"]) or int(got["num_inliers"]) < 7:
            bad.append("num_inliers is not the mask's sum, or below 7")
        if int(got["num_trials"]) < 1 or (int(got["best_trial"]) & ~LOCAL_BIT) >= int(got["num_trials"]):
            bad.append("best_trial outside the trials run")
    else:
        if mask.any() or int(got["num_inliers"]) or int(got["num_trials"]) or int(got["best_trial"]) != -1 or int(got["accepted"]):
            bad.append("outputs set without a model")
    return bad


# ---------------------------------------------------------------------------------------------------- catalogue
WIDTH, HEIGHT, FOCAL = 1280.0, 720.0, 1000.0
K = np.array([[FOCAL, 0, WIDTH / 2], [0, FOCAL, HEIGHT / 2], [0, 0, 1]])


def _rot(axis, ang):
    axis = np.asarray(axis, float) / np.linalg.norm(axis)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + math.sin(ang) * Kx + (1 - math.cos(ang)) * Kx @ Kx


def make_pair(n, outliers, noise_px, seed, planar=False, rotation_only=False, baseline=1.0):
    """two views of n points in pixels: image a at the identity, image b = (R, t), |t| about `baseline` at depths 5 .. 9;
    -> xa, xb, R, t"""
    rng = np.random.default_rng(seed)
    X = np.stack([rng.uniform(-3, 3, n), rng.uniform(-1.7, 1.7, n), rng.uniform(5, 9, n)], 1)
    if planar:
        X[:, 2] = 6.0 + 0.2 * X[:, 0] - 0.1 * X[:, 1]
    R = _rot([0.1, 1.0, 0.05], -0.07)
    t = np.array([-1.0, 0.05, 0.1]) * (0.0 if rotation_only else baseline)
    Y = X @ R.T + t
    xa = (X / X[:, 2:]) @ K.T
    xb = (Y / Y[:, 2:]) @ K.T
    xa, xb = xa[:, :2].copy(), xb[:, :2].copy()
    if noise_px:
        xa += np.clip(rng.normal(0, noise_px, xa.shape), -2.5 * noise_px, 2.5 * noise_px)
        xb += np.clip(rng.normal(0, noise_px, xb.shape), -2.5 * noise_px, 2.5 * noise_px)
    n_out = int(round(outliers * n))
    if n_out:
        idx = rng.permutation(n)[:n_out]
        xb[idx] = np.stack([rng.uniform(0, WIDTH, n_out), rng.uniform(0, HEIGHT, n_out)], 1)
    return np.ascontiguousarray(xa), np.ascontiguousarray(xb), R, t


LENGTHS = (15, 16, 63, 64, 65, 255, 256, 257, 1000)
TINY = dict(min_matches=7, min_num_inliers=7, max_num_trials=2, min_num_trials=0)
ONE_TRIAL = dict(min_matches=7, min_num_inliers=7, max_num_trials=1, min_num_trials=0)


@functools.lru_cache(maxsize=None)
def catalogue():
    """-> (main, degenerate): lists of dict(tag, xa, xb, opt (dict of overrides), R, t)"""
    main, seed = [], 500

    def add(tag, opt=None, lst=None, xform=None, **kw):
        nonlocal seed
        seed += 1
        xa, xb, R, t = make_pair(seed=kw.pop("seed", seed), **kw)
        if xform:
            xa, xb = xform(xa, xb)
        (main if lst is None else lst).append(dict(tag=tag, xa=xa, xb=xb, opt=opt or {}, R=R, t=t))
    for n in LENGTHS:
        for share in (0.0, 0.3):
            add("n%d_s%g" % (n, share), n=n, outliers=share, noise_px=0.5)
    add("n100_s0.5", n=100, outliers=0.5, noise_px=0.5)
    add("n257_s0.5", n=257, outliers=0.5, noise_px=0.5)
    add("n100_s0.7", n=100, outliers=0.7, noise_px=0.5)
    add("n8192", n=MAX_MATCHES, outliers=0.3, noise_px=0.5)
    add("too_few", n=14, outliers=0.0, noise_px=0.5)
    too_many = np.zeros((MAX_MATCHES + 1, 2))
    main.append(dict(tag="too_many", xa=too_many, xb=too_many.copy(), opt={}, R=None, t=None))
    # seven matches: every trial solves the same seven equations, so the trials (and the roots of one trial, each an exact fit)
    # differ by rounding only.  One trial, and a seed whose cubic has a single real root, leave nothing to a tie.  Eight matches:
    # a seed whose 8-point model wins.
    add("n7", ONE_TRIAL, n=7, outliers=0.0, noise_px=0.5, seed=901)
    add("n8", TINY, n=8, outliers=0.0, noise_px=0.5, seed=907)
    add("n20_tiny", TINY, n=20, outliers=0.0, noise_px=0.5)
    rng = np.random.default_rng(77)
    main.append(dict(tag="pure_noise", xa=rng.uniform(0, 700, (64, 2)), xb=rng.uniform(0, 700, (64, 2)), opt=dict(max_num_trials=300), R=None, t=None))
    for mt in (63, 64, 65):
        add("abort%d" % mt, dict(min_num_trials=mt), n=100, outliers=0.1, noise_px=0.5)
    add("cap70", dict(max_num_trials=70, min_num_trials=70), n=100, outliers=0.3, noise_px=0.5)
    add("cap70_s0", dict(max_num_trials=70, min_num_trials=70), n=65, outliers=0.0, noise_px=0.5)
    add("confidence1", dict(confidence=1.0, max_num_trials=130, min_num_trials=0), n=64, outliers=0.2, noise_px=0.5)
    add("early", dict(min_num_trials=0, confidence=0.99), n=100, outliers=0.2, noise_px=0.5)
    add("early_s0", dict(min_num_trials=0, confidence=0.99), n=257, outliers=0.0, noise_px=0.5)
    add("seed7", dict(seed=7), n=256, outliers=0.3, noise_px=0.5)
    add("wide_error", dict(max_error=8.0), n=255, outliers=0.3, noise_px=1.0)
    # the match (0, 0) <-> (0, 0) forces F(2,2) = 0 on every model of a sample that holds it: trials without a model
    def origin(a, b):
        a[0] = 0.0; b[0] = 0.0
        return a, b
    add("origin_match", xform=origin, n=30, outliers=0.2, noise_px=0.5)
    add("noisy", n=200, outliers=0.2, noise_px=1.5)
    add("noisy40", n=40, outliers=0.2, noise_px=1.5)
    rng = np.random.default_rng(78)
    for n, s in zip(rng.integers(20, 300, 12), rng.uniform(0, 0.45, 12)):
        add("random", n=int(n), outliers=float(s), noise_px=float(rng.uniform(0.3, 1.2)))
    # every match (0, 0) <-> (0, 0): no trial has a model, the scan runs to its cap and there is no result (status 0)
    main.append(dict(tag="all_origin", xa=np.zeros((20, 2)), xb=np.zeros((20, 2)), opt=dict(max_num_trials=130), R=None, t=None))
    deg = []
    add("planar_exact", lst=deg, n=100, outliers=0.0, noise_px=0.0, planar=True)
    add("planar", lst=deg, n=100, outliers=0.1, noise_px=0.5, planar=True)
    add("pure_rotation", lst=deg, n=64, outliers=0.0, noise_px=0.5, rotation_only=True)
    add("exact", lst=deg, n=64, outliers=0.0, noise_px=0.0)
    add("exact_with_outliers", lst=deg, n=100, outliers=0.3, noise_px=0.0)
    add("duplicated", lst=deg, n=64, outliers=0.0, noise_px=0.5,
        xform=lambda a, b: (np.ascontiguousarray(np.repeat(a[:8], 8, 0)), np.ascontiguousarray(np.repeat(b[:8], 8, 0))))
    add("one_match_only", lst=deg, n=32, outliers=0.0, noise_px=0.5,
        xform=lambda a, b: (np.ascontiguousarray(np.repeat(a[:1], 32, 0)), np.ascontiguousarray(np.repeat(b[:1], 32, 0))))

    def collinear(a, b):
        s = np.linspace(0.0, 1.0, len(a))[:, None]
        return (np.ascontiguousarray(np.array([100.0, 80.0]) + s * np.array([900.0, 450.0])),
                np.ascontiguousarray(np.array([140.0, 60.0]) + s * s * np.array([800.0, 500.0])))
    add("collinear", lst=deg, n=40, outliers=0.0, noise_px=0.0, xform=collinear)
    return main, deg


def entries():
    main, deg = catalogue()
    return main + deg


def n_main():
    return len(catalogue()[0])


def arrays(idx):
    """the flat arrays of a call over the catalogue entries idx: match_ptr, xy_a, xy_b"""
    E = entries()
    ptr = np.zeros(len(idx) + 1, np.int32)
    for i, k in enumerate(idx):
        ptr[i + 1] = ptr[i] + len(E[k]["xa"])
    xa = np.concatenate([E[k]["xa"] for k in idx]) if idx else np.zeros((0, 2))
    xb = np.concatenate([E[k]["xb"] for k in idx]) if idx else np.zeros((0, 2))
    return ptr, np.ascontiguousarray(xa), np.ascontiguousarray(xb)


def option_groups():
    """catalogue indices grouped by their option overrides (one library call per group)"""
    groups = {}
    for k, e in enumerate(entries()):
        groups.setdefault(tuple(sorted(e["opt"].items())), []).append(k)
    return groups


@functools.lru_cache(maxsize=None)
def reference(precision="longdouble"):
    return [run_pair(e["xa"], e["xb"], Options(**e["opt"]), np.dtype(precision), want_records=(precision == "longdouble")) for e in entries()]


def _perturbed(a, rng):
    """every coordinate times 1 +- 2^-43; equal values get equal factors"""
    vals, inv = np.unique(a, return_inverse=True)
    return (vals * (1.0 + PERTURBATION * rng.choice([-1.0, 1.0], len(vals))))[inv.ravel()].reshape(a.shape)


@functools.lru_cache(maxsize=None)
def fragile():
    """per entry: the two precisions disagree on a discrete output, or one of three float64 reruns with every coordinate perturbed by
    a relative 2^-43 does"""
    ext, f64, out = reference("longdouble"), reference("float64"), []
    for k, e in enumerate(entries()):
        bad = not same_discrete(ext[k], f64[k])
        if not bad and ext[k]["status"] < 2:
            for rerun in range(3):
                rng = np.random.default_rng(9000 + 10 * k + rerun)
                r = run_pair(_perturbed(e["xa"], rng), _perturbed(e["xb"], rng), Options(**e["opt"]), np.float64)
                if not same_discrete(r, ext[k]):
                    bad = True
                    break
        out.append(bad)
    return out


def fragile_share():
    return sum(fragile()[:n_main()]) / n_main()


@functools.lru_cache(maxsize=None)
def restatement_deviation():
    """the float64 restatement's largest deviation from the extended run over the non-fragile status-1 pairs of the main catalogue"""
    ext, f64, fr, worst = reference("longdouble"), reference("float64"), fragile(), 0.0
    for k in range(n_main()):
        if not fr[k] and ext[k]["status"] == 1:
            worst = max(worst, deviation(f64[k]["F"], ext[k]))
    return worst


def all_flags(only_solid=True):
    ext, fr = reference("longdouble"), fragile()
    return set().union(*[e["flags"] for k, e in enumerate(ext) if k < n_main() and not (only_solid and fr[k])])


@functools.lru_cache(maxsize=None)
def cases():
    """name -> catalogue indices in batch order (default options): one pair, every default-option pair, and 257 pairs (more
    workgroups than compute units) drawn from the pairs of at most 257 matches"""
    E, ext = entries(), reference("longdouble")
    dflt = [k for k, e in enumerate(E) if not e["opt"]]
    small = [k for k in dflt if len(E[k]["xa"]) <= 257]
    rng = np.random.default_rng(3)
    one = next(k for k in small if ext[k]["status"] == 1 and len(E[k]["xa"]) >= 63)
    return {"one": [one], "all": dflt, "b257": [int(k) for k in rng.permutation((small * (257 // len(small) + 1))[:257])]}
