"""Yardstick, catalogue and bar of the triangulation tests (tests/test_tri_cpu.py, tests/test_gpu_triangulate.py).

The yardstick is a pure numpy restatement of the rule xrsfm_ba_triangulate_tracks restates (include/xrsfm_ba.h; the reference's
CreatePoint3d1 -> colmap::EstimateTriangulation), parameterised by dtype and run in np.longdouble (x87 extended: eps = 2^-64 <
2e-19, asserted) and in np.float64.  The Jacobi routines are written by hand, because numpy's linear algebra has no extended
precision.  It is never the library and shares no code with it: the scan below is its own restatement, not ba_tri_scan.h.

Rule.  Trials are the pairs (i, j), i < j, of a track's observations in lexicographic order.  max_trials = min(max_num_trials,
ComputeNumTrials(min_inlier_ratio 1e5, 1e5, confidence), C(n, 2)); min_trials = C(n, 2) for n <= exhaustive_threshold, else 0.
Sample model: right singular vector of the smallest singular value of the 4x4 two-view DLT (rows x P2 - P0, y P2 - P1),
de-homogenised; it exists iff both depths are >= DBL_EPSILON and the triangulation angle (law of cosines, min(a, pi - a)) is >=
the minimum.  Residual: acos(r1^ . r2^)^2, r1 = (x, y, 1), r2 = P (X, 1), no depth test, no clamp.  Inlier: residual <=
max_error^2; support = (count, sum of inlier residuals, summed in observation order); a beats b iff count larger, or equal and sum
strictly smaller; initial best (0, DBL_MAX).  Per trial t: a sample whose support beats the best becomes the best; with count > 2
its inliers are refit by the multi-view estimator (A = sum (P - p^ p^T P)^T (P - p^ p^T P), eigenvector of the smallest
eigenvalue; needs every inlier depth >= DBL_EPSILON and any pair of inlier centres with angle >= minimum) and the refit replaces
it if its support over all observations beats it; after each new best dyn = ceil(log(1 - c) / log(1 - (k / n)^2)) (1 if the
denominator's argument is <= 0, unbounded if 1 - c <= 0 or k = 0: the library's defined meaning); only in a trial with a sample
model, t >= dyn and t >= min_trials set abort; the next trial, if the bound admits one, is counted and the scan stops.  Success
iff the best count >= 2; the mask is the inlier test of the returned model.

Margin.  Besides the outputs, every track gets the smallest relative distance of any decision the scan took from its threshold:
residual against max_error^2, depth against DBL_EPSILON, triangulation angle against the minimum, the relative gap of the sums of
two supports of equal (non-zero) count, and 1 - |cos| against 4 * 2^-53 for the acos argument (a cosine closer to 1 than that
counts as distance 0: float64 may round it above 1).  A track is FRAGILE when the extended run's margin is below 1e-8 or the
float64 and the extended run disagree in a discrete output.  1e-8: a decision quantity of an accepted model carries a relative
rounding error of about c 2^-53 / sin^2(1.5 deg) ~ 2e-11 for c ~ 100 operations; 1e-8 is 500 times that.

Model bar (a backward error, independent of parallax).  h = (X, 1) / |(X, 1)| of a returned X; M = the extended-precision A^T A
of the winning pair's DLT (m = 2), or the multi-view A over the m observations that entered the refit when bit 30 of best_trial
is set (the inliers of that trial's sample model, which are the returned inliers whenever the refit keeps them).  Required:
    h^T M h - lambda_min(M) <= (256 + 16 m) 2^-53 trace(M).
Counts: an entry of M is a sum of m (pair: 4) products of entries that are each formed in float64 from a float64 rotation
(quat_to_mat: 4 roundings), the coordinates (x P2 - P0: 2 roundings; p^ p^T P: 8) and then squared and summed (2 per term): at
most 16 roundings of relative size 2^-53 per observation and entry, each bounded by trace(M), and h minimises the quotient of the
float64 M, so its excess for the extended M is at most twice that perturbation divided between the two matrices: 16 m.  The
decomposition adds a backward error of one rounding per rotation entry: a capped 12 sweeps of 6 rotations touch an entry at most
72 x 2 times, and the de-homogenisation and renormalisation add 8: 256 covers them.  A wrong or sloppy null vector misses the bar by
the spectral gap (>= sin^2 of the parallax, times trace).
"""
import functools
import math

import numpy as np

EXT = np.longdouble
assert np.finfo(EXT).eps < 2e-19, "np.longdouble is not extended precision here"

DBL_EPS = 2.0 ** -52
DBL_MAX = float(np.finfo(np.float64).max)
ACOS_GUARD = 4.0 * 2.0 ** -53
MAX_OBS = 128
LOCAL_BIT = 1 << 30
UNBOUNDED = 2 ** 31 - 1
FRAGILE_MARGIN = 1e-8
CHUNK = 64


class Options:
    def __init__(self, **kw):
        self.min_tri_angle_rad = math.radians(1.5)
        self.max_error_rad = math.radians(2.0)
        self.confidence = 0.9999
        self.min_inlier_ratio = 0.02
        self.max_num_trials = 10000
        self.exhaustive_threshold = 15
        for k, v in kw.items():
            assert hasattr(self, k), k
            setattr(self, k, v)


def num_trials_bound(k, n, confidence):
    nom = 1.0 - confidence
    if nom <= 0.0 or k <= 0:
        return UNBOUNDED
    ratio = k / float(n)
    denom = 1.0 - ratio * ratio
    if denom <= 0.0:
        return 1
    return min(UNBOUNDED, int(math.ceil(math.log(nom) / math.log(denom))))


def quat_to_mat(q, dtype):
    x, y, z, w = (np.asarray(q[..., i], dtype) for i in range(4))
    M = np.empty(q.shape[:-1] + (3, 3), dtype)
    M[..., 0, 0] = 1 - 2 * (y * y + z * z); M[..., 0, 1] = 2 * (x * y - w * z); M[..., 0, 2] = 2 * (x * z + w * y)
    M[..., 1, 0] = 2 * (x * y + w * z); M[..., 1, 1] = 1 - 2 * (x * x + z * z); M[..., 1, 2] = 2 * (y * z - w * x)
    M[..., 2, 0] = 2 * (x * z - w * y); M[..., 2, 1] = 2 * (y * z + w * x); M[..., 2, 2] = 1 - 2 * (x * x + y * y)
    return M


def _rot(a, b, sel):
    """Jacobi rotation that zeroes the coupling b between diagonal-like quantities: zeta = a / (2 b); returns (c, s), identity where
    sel is false."""
    zeta = a / (2 * np.where(sel, b, 1))
    t = np.where(zeta >= 0, 1, -1) / (np.abs(zeta) + np.sqrt(1 + zeta * zeta))
    c = 1 / np.sqrt(1 + t * t)
    s = c * t
    one = np.ones_like(c)
    return np.where(sel, c, one), np.where(sel, s, 0 * one)


def null_svd(A):
    """A [T, 4, 4] -> right singular vectors of the smallest singular values [T, 4], one-sided (Hestenes) Jacobi."""
    dt = A.dtype
    A = A.copy()
    T = A.shape[0]
    V = np.tile(np.eye(4, dtype=dt), (T, 1, 1))
    tol = 8 * np.finfo(dt).eps
    with np.errstate(all="ignore"):
        for _ in range(40):
            any_rot = False
            for p in range(3):
                for q in range(p + 1, 4):
                    ap, aq = A[:, :, p].copy(), A[:, :, q].copy()
                    al, be, ga = (ap * ap).sum(1), (aq * aq).sum(1), (ap * aq).sum(1)
                    sel = np.abs(ga) > tol * np.sqrt(al * be)
                    if not sel.any():
                        continue
                    any_rot = True
                    c, s = _rot(be - al, ga, sel)
                    c, s = c[:, None], s[:, None]
                    A[:, :, p], A[:, :, q] = c * ap - s * aq, s * ap + c * aq
                    vp, vq = V[:, :, p].copy(), V[:, :, q].copy()
                    V[:, :, p], V[:, :, q] = c * vp - s * vq, s * vp + c * vq
            if not any_rot:
                break
        idx = np.argmin((A * A).sum(1), axis=1)
    return V[np.arange(T), :, idx]


def min_eig(M):
    """Symmetric M [4, 4] -> (smallest eigenvalue, its eigenvector), cyclic two-sided Jacobi."""
    dt = M.dtype
    M = M.copy()
    V = np.eye(4, dtype=dt)
    floor = np.finfo(dt).eps * 1e-3 * np.trace(M)
    tol = 8 * np.finfo(dt).eps
    for _ in range(40):
        any_rot = False
        for p in range(3):
            for q in range(p + 1, 4):
                if not abs(M[p, q]) > tol * np.sqrt(abs(M[p, p] * M[q, q])) + floor:
                    continue
                any_rot = True
                theta = (M[q, q] - M[p, p]) / (2 * M[p, q])
                t = (1 if theta >= 0 else -1) / (abs(theta) + np.sqrt(1 + theta * theta))
                c = 1 / np.sqrt(1 + t * t)
                s = c * t
                mp, mq = M[:, p].copy(), M[:, q].copy()
                M[:, p], M[:, q] = c * mp - s * mq, s * mp + c * mq
                mp, mq = M[p, :].copy(), M[q, :].copy()
                M[p, :], M[q, :] = c * mp - s * mq, s * mp + c * mq
                M[p, q] = M[q, p] = 0
                vp, vq = V[:, p].copy(), V[:, q].copy()
                V[:, p], V[:, q] = c * vp - s * vq, s * vp + c * vq
        if not any_rot:
            break
    i = int(np.argmin(np.diag(M)))
    return M[i, i], V[:, i]


def tri_angle(c1, c2, X):
    """law of cosines, min(a, pi - a); broadcasts"""
    dt = X.dtype
    b2 = ((c1 - c2) ** 2).sum(-1); r1 = ((X - c1) ** 2).sum(-1); r2 = ((X - c2) ** 2).sum(-1)
    den = 2 * np.sqrt(r1 * r2)
    with np.errstate(all="ignore"):
        ang = np.abs(np.arccos((r1 + r2 - b2) / np.where(den == 0, 1, den)))
        ang = np.minimum(ang, _pi(dt) - ang)
    return np.where(den == 0, 0 * ang, ang)


def _pi(dt):
    return np.float64(math.pi) if np.dtype(dt) == np.float64 else np.arctan(EXT(1)) * 4


def residuals(P, xy, X):
    """P [n, 3, 4], xy [n, 2], X [T, 3] -> (squared angles [T, n], 1 - |cos| [T, n])"""
    dt = P.dtype
    r2 = np.einsum("nrc,tc->tnr", P[:, :, :3], X) + P[None, :, :, 3]
    r1 = np.concatenate([xy, np.ones((len(xy), 1), dt)], axis=1)
    with np.errstate(all="ignore"):
        u1 = r1 / np.sqrt((r1 * r1).sum(-1))[:, None]
        u2 = r2 / np.sqrt((r2 * r2).sum(-1))[:, :, None]
        cos = (u1[None] * u2).sum(-1)
        ang = np.arccos(cos)
    return ang * ang, 1 - np.abs(cos)


def support(res, max_res):
    """count and sum of the inlier residuals, summed in observation order; res [T, n]"""
    with np.errstate(invalid="ignore"):
        inl = res <= max_res
    s = np.zeros(res.shape[0], res.dtype)
    for k in range(res.shape[1]):
        s = s + np.where(inl[:, k], res[:, k], 0)
    return inl, inl.sum(1), s


def dlt(P, xy, i, j):
    """[T, 4, 4] two-view DLT of the pairs (i[t], j[t])"""
    rows = []
    for k in (i, j):
        rows.append(xy[k, 0, None] * P[k, 2, :] - P[k, 0, :])
        rows.append(xy[k, 1, None] * P[k, 2, :] - P[k, 1, :])
    return np.stack(rows, axis=1)


def multiview_matrix(P, xy, idx):
    dt = P.dtype
    M = np.zeros((4, 4), dt)
    for k in idx:
        p = np.array([xy[k, 0], xy[k, 1], 1], dt)
        p = p / np.sqrt((p * p).sum())
        T = P[k] - np.outer(p, p @ P[k])
        M = M + T.T @ T
    return M


def _rel(q, thr):
    d = np.abs(np.asarray(q, EXT) - EXT(thr)) / max(abs(float(thr)), 1e-300)
    d = d[np.isfinite(d)] if d.ndim else d
    return float(np.min(d)) if np.size(d) else np.inf


def _cos_margin(omc):
    v = np.asarray(omc, EXT).ravel()
    v = v[np.isfinite(v)]
    return float(np.min(np.maximum(v - ACOS_GUARD, 0) / ACOS_GUARD)) if v.size else np.inf


class Track:
    """One track's data in a dtype: P [n, 3, 4], centres [n, 3], xy [n, 2]"""
    def __init__(self, cam_q, cam_t, cams, xy, dtype):
        R = quat_to_mat(np.asarray(cam_q, np.float64)[cams], dtype)
        t = np.asarray(np.asarray(cam_t, np.float64)[cams], dtype)
        self.P = np.concatenate([R, t[:, :, None]], axis=2)
        self.C = -np.einsum("nrc,nr->nc", R, t)
        self.xy = np.asarray(np.asarray(xy, np.float64), dtype)
        self.n = len(cams)


def pairs_of(n):
    i, j = np.triu_indices(n, 1)
    return i, j          # row-major upper triangle = lexicographic


def sample_models(tr, i, j, opt):
    """-> X [T, 3], has [T], (depth margin, angle margin) over these trials"""
    dt = tr.P.dtype
    v = null_svd(dlt(tr.P, tr.xy, i, j))
    with np.errstate(all="ignore"):
        X = v[:, :3] / v[:, 3:4]
        di = (tr.P[i, 2, :3] * X).sum(1) + tr.P[i, 2, 3]
        dj = (tr.P[j, 2, :3] * X).sum(1) + tr.P[j, 2, 3]
        ang = tri_angle(tr.C[i], tr.C[j], X)
        dok = (di >= dt.type(DBL_EPS)) & (dj >= dt.type(DBL_EPS))
        has = dok & (ang >= dt.type(opt.min_tri_angle_rad))
    return X, has, di, dj, ang, dok


def refit(tr, inl, opt, max_res):
    """multi-view estimate over the observations inl -> dict(has, X, cnt, sum, mask) and its margin"""
    dt = tr.P.dtype
    idx = np.flatnonzero(inl)
    _, v = min_eig(multiview_matrix(tr.P, tr.xy, idx))
    margin = np.inf
    with np.errstate(all="ignore"):
        X = (v[:3] / v[3])[None]
        d = (tr.P[idx, 2, :3] * X).sum(1) + tr.P[idx, 2, 3]
    margin = min(margin, _rel(d, DBL_EPS))
    if not np.all(d >= dt.type(DBL_EPS)):
        return dict(has=False, why="depth"), margin
    a, b = np.triu_indices(len(idx), 1)
    ang = tri_angle(tr.C[idx[a]], tr.C[idx[b]], X)
    amax = np.max(ang) if ang.size else dt.type(0)
    margin = min(margin, _rel(amax, opt.min_tri_angle_rad) if opt.min_tri_angle_rad > 0 else np.inf)
    if not amax >= dt.type(opt.min_tri_angle_rad):
        return dict(has=False, why="angle"), margin
    res, omc = residuals(tr.P, tr.xy, X)
    m, cnt, s = support(res, max_res)
    margin = min(margin, _rel(res, float(max_res)), _cos_margin(omc))
    return dict(has=True, X=X[0], cnt=int(cnt[0]), sum=s[0], mask=m[0]), margin


def run_track(cam_q, cam_t, cams, xy, opt=None, dtype=EXT, want_records=False):
    """The whole rule for one track.  Returns dict(status, point, mask, num_inliers, num_trials, best_trial, margin, flags, records)."""
    opt = opt or Options()
    dt = np.dtype(dtype)
    n = len(cams)
    out = dict(status=0, point=None, mask=np.zeros(n, np.uint8), num_inliers=0, num_trials=0, best_trial=-1, margin=np.inf, flags=set(),
               records=[])
    if n < 2:
        out["status"] = 2
        return out
    if n > MAX_OBS:
        out["status"] = 3
        return out
    tr = Track(cam_q, cam_t, np.asarray(cams), xy, dt)
    max_res = dt.type(np.float64(opt.max_error_rad) * np.float64(opt.max_error_rad))
    pairs = n * (n - 1) // 2
    ratio_k = int(opt.min_inlier_ratio * 100000.0)
    max_trials = min(opt.max_num_trials, num_trials_bound(ratio_k, 100000, opt.confidence), pairs)
    min_trials = pairs if n <= opt.exhaustive_threshold else 0
    I, J = pairs_of(n)
    best_cnt, best_sum, best_trial, best_local = 0, dt.type(DBL_MAX), -1, False
    best_X, best_mask = None, None
    dyn, abort, num_trials = max_trials, False, max_trials
    margin, flags, records = np.inf, out["flags"], out["records"]

    def beats(ca, sa, cb, sb):
        nonlocal margin
        if ca == cb and ca > 0:
            big = max(abs(float(sa)), abs(float(sb)))
            margin = min(margin, abs(float(EXT(sa) - EXT(sb))) / big if big > 0 else np.inf)
        return ca > cb or (ca == cb and sa < sb)

    for t0 in range(0, max_trials, CHUNK):
        sl = slice(t0, min(t0 + CHUNK, max_trials))
        X, has, di, dj, ang, dok = sample_models(tr, I[sl], J[sl], opt)
        res, omc = residuals(tr.P, tr.xy, X)
        inl, cnt, ssum = support(res, max_res)
        for l in range(sl.stop - sl.start):
            t = t0 + l
            margin = min(margin, _rel(di[l], DBL_EPS), _rel(dj[l], DBL_EPS))
            if dok[l] and opt.min_tri_angle_rad > 0:
                margin = min(margin, _rel(ang[l], opt.min_tri_angle_rad))
            if not dok[l]:
                flags.add("behind_camera")
            elif not has[l]:
                flags.add("low_angle_pair")
            rec = [int(has[l]), int(cnt[l]), float(ssum[l]) if has[l] else 0.0, -2, 0.0]
            if has[l]:
                margin = min(margin, _rel(res[l], float(max_res)), _cos_margin(omc[l]))
                if cnt[l] == 0:
                    flags.add("zero_inlier_model")
                if beats(int(cnt[l]), ssum[l], best_cnt, best_sum):
                    best_cnt, best_sum, best_trial, best_local = int(cnt[l]), ssum[l], t, False
                    best_X, best_mask = X[l], inl[l]
                    if cnt[l] > 2:
                        r, mg = refit(tr, inl[l], opt, max_res)
                        margin = min(margin, mg)
                        rec[3] = -1
                        if r["has"]:
                            rec[3], rec[4] = r["cnt"], float(r["sum"])
                            if beats(r["cnt"], r["sum"], best_cnt, best_sum):
                                best_cnt, best_sum, best_local = r["cnt"], r["sum"], True
                                best_X, best_mask = r["X"], r["mask"]
                                flags.add("refit_won@%d" % t)
                            else:
                                flags.add("refit_lost@%d" % t)
                        else:
                            flags.add("refit_no_model")
                    dyn = num_trials_bound(best_cnt, n, opt.confidence)
                if t >= dyn and t >= min_trials:
                    abort = True
                    num_trials = t + 2 if t + 1 < max_trials else t + 1
            if want_records:
                records.append(rec)
            if abort:
                break
        if abort:
            break
    out["margin"] = margin
    if abort:
        flags.add("aborted")
    if best_cnt >= 2 and best_X is not None and np.all(np.isfinite(best_X)):
        out.update(status=1, point=best_X, mask=np.asarray(best_mask, np.uint8), num_inliers=best_cnt, num_trials=num_trials,
                   best_trial=best_trial | (LOCAL_BIT if best_local else 0))
        flags.add("final_local" if best_local else ("final_sample_refit_lost" if "refit_lost@%d" % best_trial in flags else "final_sample"))
    out["scan"] = dict(best_trial=best_trial, local=int(best_local), num_trials=num_trials, success=int(best_cnt >= 2), n=n)
    return out


def bar_matrix(cam_q, cam_t, cams, xy, code, opt=None):
    """The extended-precision M of the bar for a returned best_trial code -> (M, lambda_min, m)."""
    opt = opt or Options()
    tr = Track(cam_q, cam_t, np.asarray(cams), xy, np.dtype(EXT))
    t = code & ~LOCAL_BIT
    I, J = pairs_of(tr.n)
    i, j = I[t:t + 1], J[t:t + 1]
    A = dlt(tr.P, tr.xy, i, j)[0]
    if not code & LOCAL_BIT:
        M, m = A.T @ A, 2
    else:
        X = sample_models(tr, i, j, opt)[0]
        res, _ = residuals(tr.P, tr.xy, X)
        max_res = EXT(np.float64(opt.max_error_rad) * np.float64(opt.max_error_rad))
        idx = np.flatnonzero(res[0] <= max_res)
        M, m = multiview_matrix(tr.P, tr.xy, idx), len(idx)
    lam, _ = min_eig(M)
    return M, lam, m


def bar_check(X, M, lam, m):
    """-> (excess of the Rayleigh quotient, bar); both in units of trace(M)"""
    h = np.concatenate([np.asarray(X, EXT), [EXT(1)]])
    h = h / np.sqrt((h * h).sum())
    tr = np.trace(M)
    return float((h @ M @ h - lam) / tr), (256 + 16 * m) * 2.0 ** -53


# ------------------------------------------------------------------------------------------------------------ catalogue
# Lengths: 2 (one trial, no refit), 3 (first refit), 4, 11 / 12 (55 / 66 trials: either side of one 64-trial block), 15 / 16 / 17 (the
# exhaustive threshold), 64 / 65 (one or two observations per lane), 128 (the cap), 129 (status 3), 0 / 1 (status 2).
LENGTHS = (0, 1, 2, 3, 4, 11, 12, 15, 16, 17, 64, 65, 128, 129)
REQUIRED = ("all_pairs_low_angle", "behind_camera", "zero_inlier_model", "inliers16_abort_after_trial_1", "long_20pct_inliers",
            "refit_wins", "refit_loses", "refit_no_model", "same_camera_twice")
N_POOL_CAMS = 140
BASELINES = (0.02, 0.1, 0.5)


@functools.lru_cache(maxsize=None)
def cameras():
    """Three rows of cameras along x with spacing 0.02 / 0.1 / 0.5, looking down +z with small random rotations, and a few cameras
    for the constructed tracks.  Tcw: t = -R c."""
    rng = np.random.default_rng(20241)
    q, c = [], []
    for b in BASELINES:
        for i in range(N_POOL_CAMS):
            w = rng.uniform(-0.05, 0.05, 3)
            q.append(w); c.append([b * i + rng.uniform(-0.2, 0.2) * b, rng.uniform(-0.3, 0.3) * b * 3, rng.uniform(-0.3, 0.3) * b * 3])
    for x in (0.0, 0.001, 0.002, 1.0, 0.2, 0.004, 0.008, 0.012, 0.016, 0.03, 0.05, 0.07):          # the constructed tracks' cameras (identity rotation)
        q.append(np.zeros(3)); c.append([x, 0.0, 0.0])
    w = np.array(q); c = np.array(c)
    ang = np.linalg.norm(w, axis=1)
    s = np.where(ang > 0, np.sin(ang / 2) / np.where(ang > 0, ang, 1), 0.5)
    quat = np.concatenate([w * s[:, None], np.cos(ang / 2)[:, None]], axis=1)
    R = quat_to_mat(quat, np.float64)
    t = -np.einsum("nrc,nc->nr", R, c)
    return np.ascontiguousarray(quat), np.ascontiguousarray(t), c


SPECIAL0 = 3 * N_POOL_CAMS       # index of the first constructed camera


def _project(cam, X):
    quat, t, _ = cameras()
    R = quat_to_mat(quat[cam], np.float64)
    pc = np.einsum("nrc,c->nr", R, X) + t[cam]
    return pc[:, :2] / pc[:, 2:3]


def _random_track(rng, n, row, outlier_frac=0.2, noise=1e-3):
    start = int(rng.integers(0, N_POOL_CAMS - n + 1))
    cams = row * N_POOL_CAMS + start + rng.permutation(n)
    _, _, c = cameras()
    X = np.array([c[cams, 0].mean() + rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(4, 12)])
    xy = _project(cams, X) + rng.normal(0, noise, (n, 2))
    out = rng.random(n) < outlier_frac
    xy[out] += rng.uniform(-0.2, 0.2, (int(out.sum()), 2))
    return dict(cams=cams.astype(np.int32), xy=xy, tag="random")


@functools.lru_cache(maxsize=None)
def pool():
    """Every distinct track of the catalogue, noisy observations throughout (a noise-free track meets acos above 1)."""
    rng = np.random.default_rng(77031)
    tracks = []
    for k in range(200):                                   # ordinary tracks: lengths 2..33, the three baselines
        tracks.append(_random_track(rng, int(rng.integers(2, 34)), k % 3))
    for n in LENGTHS:
        for rep in range(1 if n >= 64 else 3):
            if n < 2:
                tr = dict(cams=np.arange(n, dtype=np.int32), xy=rng.normal(0, 0.1, (n, 2)), tag="len%d" % n)
            else:
                tr = _random_track(rng, n, 1 if n >= 64 else 2 - (rep == 1 and n > 4))
                tr["tag"] = "len%d" % n
            tracks.append(tr)
    S = SPECIAL0
    nz = lambda k: rng.normal(0, 1e-3, (k, 2))
    X = np.array([0.3, -0.2, 8.0])
    # all pairs below the minimum angle: three cameras 1 mm apart
    cams = np.array([S + 0, S + 1, S + 2])
    tracks.append(dict(cams=cams, xy=_project(cams, X) + nz(3) * 1e-2, tag="all_pairs_low_angle"))
    # a pair model behind the cameras: diverging rays from x = 0 and x = 1, then two views that agree with nothing
    cams = np.array([S + 0, S + 3])
    tracks.append(dict(cams=cams, xy=np.array([[0.0, 0.0], [0.3, 0.0]]) + nz(2), tag="behind_camera"))
    # an outlier pair whose rays are skew by ~11 degrees: a model with no inlier at all (the defined-meaning case), alone and
    # in front of a consistent track
    tracks.append(dict(cams=cams, xy=np.array([[0.0, 0.0], [-0.125, 0.2]]) + nz(2), tag="zero_inlier_model"))
    row = 2 * N_POOL_CAMS
    good = row + 10 + np.arange(6)
    Xg = np.array([cameras()[2][good, 0].mean(), 0.1, 7.0])
    cams = np.concatenate([[S + 0, S + 3], good])
    xy = np.concatenate([np.array([[0.0, 0.0], [-0.125, 0.2]]), _project(good, Xg)]) + nz(8)
    tracks.append(dict(cams=cams, xy=xy, tag="zero_inlier_model"))
    # 16 observations, inliers only: dyn = 1 after trial 0, abort in trial 1
    tr = _random_track(rng, 16, 2, outlier_frac=0.0); tr["tag"] = "inliers16_abort_after_trial_1"; tracks.append(tr)
    # a long track with 20 % inliers: 8 consistent views among 40
    n = 40
    cams = row + 20 + rng.permutation(n)
    X40 = np.array([cameras()[2][cams, 0].mean(), 0.4, 9.0])
    xy = _project(cams, X40) + nz(n)
    bad = rng.permutation(n)[:32]
    xy[bad] += rng.uniform(0.08, 0.3, (32, 2)) * rng.choice([-1.0, 1.0], (32, 2))
    tracks.append(dict(cams=cams, xy=xy, tag="long_20pct_inliers"))
    # two observations from the same camera
    tr = _random_track(rng, 6, 2, outlier_frac=0.0)
    tr["cams"] = np.concatenate([tr["cams"], tr["cams"][:1]]); tr["xy"] = np.concatenate([tr["xy"], tr["xy"][:1] + nz(1)])
    tr["tag"] = "same_camera_twice"; tracks.append(tr)
    # a refit without a model: the pair (x = 0, x = 0.2) sees its point at 1.5 deg times (1 + a little), the views of the cluster near
    # x = 0 agree with it within 2 deg, and the refit moves the point away until no pair of centres reaches 1.5 deg
    cams = np.array([S + 0, S + 4, S + 1, S + 2, S + 5, S + 6, S + 7, S + 8, S + 9, S + 10, S + 11])
    base = _project(cams, np.array([0.05, 0.02, 10.0]))
    quat, t, _ = cameras()
    jitter = np.array([[1e-4, -2e-4]] * 11) * (np.arange(11) % 4)[:, None]

    def with_bump(bump):
        xy = base + jitter
        xy[1, 0] -= bump
        return xy

    def pair_angle(bump):
        trk = Track(quat, t, cams, with_bump(bump), np.dtype(np.float64))
        return float(sample_models(trk, np.array([0]), np.array([1]), Options())[4][0])
    lo, hi = 0.004, 0.009                                  # the angle of the pair (0, 1) grows with the bump: bisect for 1.5 deg
    for _ in range(40):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if pair_angle(mid) < Options().min_tri_angle_rad else (lo, mid)
    for over in (1e-4, 3e-4, 1e-3, 2e-3):
        xy = with_bump(hi + over * 0.026)
        r = run_track(quat, t, cams, xy, dtype=np.float64)
        if "refit_no_model" in r["flags"] and r["margin"] > 1e-6:
            tracks.append(dict(cams=cams, xy=xy, tag="refit_no_model"))
            break
    for tr in tracks:
        tr["cams"] = np.asarray(tr["cams"], np.int32)
    return tracks


@functools.lru_cache(maxsize=None)
def reference(dtype_name="longdouble", opt_items=()):
    """the yardstick's result for every track of the pool; opt_items: option overrides as a tuple of (name, value)"""
    quat, t, _ = cameras()
    opt = Options(**dict(opt_items))
    return [run_track(quat, t, tr["cams"], tr["xy"], opt=opt, dtype=np.dtype(dtype_name), want_records=(dtype_name == "longdouble"))
            for tr in pool()]


DISCRETE = ("status", "num_inliers", "num_trials", "best_trial")


def same_discrete(a, b):
    return all(a[k] == b[k] for k in DISCRETE) and np.array_equal(a["mask"], b["mask"])


@functools.lru_cache(maxsize=None)
def fragile(opt_items=()):
    ext, f64 = reference("longdouble", opt_items), reference("float64", opt_items)
    return np.array([e["margin"] < FRAGILE_MARGIN or not same_discrete(e, f) for e, f in zip(ext, f64)])


@functools.lru_cache(maxsize=None)
def tags():
    """pool index lists by property: the constructed tags, plus refit_wins / refit_loses found among all tracks by their flags"""
    ext = reference("longdouble")
    by = {}
    for k, tr in enumerate(pool()):
        by.setdefault(tr["tag"], []).append(k)
    by["refit_wins"] = [k for k, e in enumerate(ext) if "final_local" in e["flags"]]
    by["refit_loses"] = [k for k, e in enumerate(ext) if "final_sample_refit_lost" in e["flags"]]
    return by


@functools.lru_cache(maxsize=None)
def cases():
    """name -> pool indices in batch order.  Batch shapes 1, 4, 5 and 257 tracks (one wave, a full workgroup, one more, more than
    a multiple of the workgroup), every length, and the special tracks among ordinary ones."""
    P = pool()
    by = tags()
    rng = np.random.default_rng(5)
    lengths = [k for k, tr in enumerate(P) if tr["tag"].startswith("len")]
    special = [k for name in REQUIRED for k in by.get(name, [])[:2]]
    mixed = list(rng.permutation(special + list(range(40))))
    rest = [k for k in range(len(P)) if k >= 200]
    b257 = list(range(200)) + rest + list(range(257 - 200 - len(rest))) if 200 + len(rest) < 257 else (list(range(200)) + rest)[:257]
    ext = reference("longdouble")
    one = next(k for k in range(200) if ext[k]["status"] == 1 and len(P[k]["cams"]) >= 3)
    return {"one": [one], "four": [0, 1, 2, 3], "five": [3, 4, 5, 6, lengths[8]], "lengths": lengths, "specials_mixed": [int(k) for k in mixed],
            "b257": [int(k) for k in rng.permutation(b257)]}


def case_arrays(name):
    """-> cam_q, cam_t, trk_ptr, obs_cam, obs_xy, pool indices"""
    quat, t, _ = cameras()
    idx = cases()[name]
    P = pool()
    ptr = np.zeros(len(idx) + 1, np.int32)
    ptr[1:] = np.cumsum([len(P[k]["cams"]) for k in idx])
    ocam = np.concatenate([P[k]["cams"] for k in idx]).astype(np.int32)
    oxy = np.concatenate([P[k]["xy"].reshape(-1, 2) for k in idx]).astype(np.float64)
    return quat, t, ptr, ocam, np.ascontiguousarray(oxy), idx
