"""Yardstick and checks of the post-BA track filter tests (tests/test_filter_cpu.py, tests/test_gpu_filter.py; cases in tests/filter_cases.py).

The yardstick is pure numpy in np.longdouble on the (value, bar) class V and seg_sum of tests/lin_yardstick.py, never the library and never
oracle/ba_oracle.py.  It restates the reference rule (src/geometry/track_processor.cc:19-26 and 253-319, colmap's CalculateTriangulationAngle)
in the expression order of xrsfm_amd/csrc/ba_filter.h:

    M(q) with q = (x, y, z, w) as it is given (no normalisation);  Pc = M P + t, no depth clamp;  xy = (X, Y) / Z;  the distortion d of the
    camera models 0 .. 4 (0 / 1: d = xy, the reference's quirk that doubles f; 2 / 3: k r^2 xy; 4: OpenCV k1 k2 p1 p2);
    e = f (xy + d) + c - uv;  re = sqrt(e0^2 + e1^2);  an observation is deleted when re > max_re or Z < 1e-3 or Z > 1e3 (a NaN compares
    false everywhere, as in C++);  centre = -(M^T t);
    per track, observations in camera order (a stable sort of the caller's order): n = 0 leaves (0, -1, -1) and counts nowhere;
    ndel >= n - 1 makes the track outlier 1, adds n to the first counter and leaves error and angle at -1;  otherwise the first counter
    gets ndel, the error is the sum of the kept re in camera order over their number, and the angle is that of UpdateTrackAngle: over the
    pairs (a, b > a) of kept observations in camera order, best = ang wherever ang > best, and the loop ends at the first best > min_angle
    (the reported angle is that pair's, not the maximum);  best < min_angle makes the track outlier 2 and adds 1 to the second counter.
    ang = min(a, pi - a), a = |acos((r1 + r2 - b2) / den)|, den = 2 sqrt(r1 r2), ang = 0 where den == 0, with pi the float64 constant.

Bars.  Every quantity is a pair (value, bar) of long doubles; the bars of +, -, *, /, sqrt and of a sum over L terms are the running-error
bounds of tests/lin_yardstick.py (eps = 2^-53 per float64 operation, valid for either association and for fused multiply-adds).  Added here:

  acos               carried like sin / cos there: the operand's bar times |acos'| = 1 / sqrt(1 - x^2), taken at the end of the operand's
                     interval nearer to +-1 (where |acos'| is largest: the mean-value bound), plus 4 eps |value| for the library function.
                     For a small angle a the operand's bar is a few eps, so the bar is about eps / a: a far point gets the wide bar its
                     conditioning costs, a near one a bar of a few ulps.
  beyond +-1         a pair whose operand interval reaches +-1 or beyond may give float64 a NaN, which `ang > best` skips (the reference's
                     std::min(NaN, .) is NaN and `NaN > max` is false: the same skip), or any angle down to 0.  Its angle is carried as
                     0 with the bar acos(|x| - bar(x)) (1 + 4 eps) + 2 pi eps: the interval [0, bar].  A skip and an angle of 0 are the same
                     to the rule (`0 > best` is false), which is why a clamp of the operand to [-1, 1] (oracle/ba_oracle.py) and the NaN
                     agree: the clamp gives acos(1) = 0, or acos(-1) = pi folded to pi - pi = 0.
  fold               pi - a is one float64 subtraction of the float64 constant pi: its bar is a's plus eps (pi + a).  min() is
                     continuous, so the fold is no decision.
  maximum            the running maximum over the pairs evaluated before the exit has the largest bar of those pairs; a pair that exits
                     has its own bar (every earlier pair lies below min_angle by more than its bar, or the track is fragile).

Three facts of float64 arithmetic make a bar zero, so that the value must come out bit for bit:
  (1) a camera whose q and t are integers of magnitude <= 1024 has integer entries of M and an integer centre, and every partial result is
      an integer below 2^53: exact in float64 under any contraction;
  (2) x - x = 0 exactly: where the point equals such an exact centre, the ray is exactly zero, r = 0 and den == 0 hold exactly;
  (3) two cameras with bit-identical (q, t) have bit-identical centres whatever the arithmetic; then b2 = 0, r1 and r2 are the same float64
      r, r + r - 0 = 2 r exactly, sqrt(r r) = r (IEEE square root of a square) and 2 r / 2 r = 1: acos(1) = 0 = min(0, pi - 0).
A bar of zero means that float64 has the long-double value; a decision on such a value cannot differ and is never fragile.

Decisions.  Every decision is taken on the long-double values.  A decision is FRAGILE when its bar is positive and its threshold lies within
the bar of its value: re against max_re, Z against float64(1e-3) and against 1e3 for an observation; for a track any of its observations'
decisions, `den == 0` (den within its bar of 0), and min_angle within the bar of any pair evaluated up to the long-double exit (which covers
the exit `best > min_angle` and the outlier test `best < min_angle`).  No case outside the exact-threshold group may hold one.

A note on `den == 0`.  A point on the centre of a camera with an orthogonal M has Z = 0 there, is deleted, and never reaches the pair loop;
the arm is reached only through a quaternion that is not normalised (M M^T != 1), which the rule takes as it is given.

The module also holds restate64(), a literal float64 loop restatement of the kernel and its host side with named switches (MUTATIONS) that
each break one rule; it shares no code with the long-double yardstick above nor with oracle/ba_oracle.py.
"""
import numpy as np

from tests.lin_yardstick import EPS, LD, V, seg_sum

F64 = np.float64
PI64 = F64(3.14159265358979323846)
Z_MIN, Z_MAX = F64(1e-3), F64(1e3)
CHECKS = ("obs_delete", "track_outlier", "num_filtered", "track_error", "track_angle")


# ------------------------------------------------------------------------------------------------ the long-double yardstick
def _quat_mat(q):
    x, y, z, w = (V(q[:, k]) for k in range(4))
    return [[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)],
            [2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x)],
            [2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)]]


def _small_integers(a):
    with np.errstate(invalid="ignore"):
        return np.all((a == np.rint(a)) & (np.abs(a) <= 1024), axis=1)


def centres(cam_q, cam_t):
    """-(M^T t) per camera as V [Nc][3]; bar 0 for the cameras of fact (1)."""
    M = _quat_mat(cam_q)
    t = [V(cam_t[:, k]) for k in range(3)]
    c = V.stack([-(M[0][k] * t[0] + M[1][k] * t[1] + M[2][k] * t[2]) for k in range(3)])
    exact = _small_integers(cam_q) & _small_integers(cam_t)
    return V(c.v, np.where(exact[:, None], LD(0), c.e))


def project(model, k, q, t, P, uv):
    """Per observation: the reprojection error re and the depth Z as V [N]."""
    M = _quat_mat(q)
    Pv = [V(P[:, i]) for i in range(3)]
    X, Y, Z = (M[i][0] * Pv[0] + M[i][1] * Pv[1] + M[i][2] * Pv[2] + V(t[:, i]) for i in range(3))
    xn, yn = X / Z, Y / Z
    r2 = xn * xn + yn * yn
    kk = [k[:, i] for i in range(8)]
    m = [model == i for i in range(5)]
    one_f = m[0] | m[2]
    fx, fy = V(kk[0]), V(np.where(one_f, kk[0], kk[1]))
    cx, cy = V(np.where(one_f, kk[1], kk[2])), V(np.where(one_f, kk[2], kk[3]))
    kr = V(np.where(m[2], kk[3], kk[4])) * r2
    du_r, dv_r = xn * kr, yn * kr
    rad = V(kk[4]) * r2 + V(kk[5]) * r2 * r2
    xy = xn * yn
    du_o = xn * rad + 2.0 * V(kk[6]) * xy + V(kk[7]) * (r2 + 2.0 * xn * xn)
    dv_o = yn * rad + 2.0 * V(kk[7]) * xy + V(kk[6]) * (r2 + 2.0 * yn * yn)
    pick = lambda a, b, c: V.where(m[0] | m[1], a, V.where(m[2] | m[3], b, c))
    du, dv = pick(xn, du_r, du_o), pick(yn, dv_r, dv_o)
    e0 = fx * (xn + du) + cx - V(uv[:, 0])
    e1 = fy * (yn + dv) + cy - V(uv[:, 1])
    return (e0 * e0 + e1 * e1).sqrt(), Z


def _near(x, thr):
    """threshold within a positive bar of the value"""
    return (x.e > 0) & (np.abs(x.v - LD(thr)) <= x.e)


def _sub(a, b):
    """a - b with fact (2): exact operands of one value give an exact zero"""
    d = a - b
    return V(d.v, np.where((a.e == 0) & (b.e == 0) & (a.v == b.v), LD(0), d.e))


def _acos(x):
    """acos of V with the bar at the interval's end nearer to +-1; `beyond`: the interval reaches +-1 (or the operand is NaN)"""
    edge = np.abs(x.v) + x.e
    beyond = ~(edge < 1)
    safe = np.where(beyond, LD(0), edge)
    val = np.arccos(np.where(beyond, LD(0), x.v))
    return V(val, x.e / np.sqrt(1 - safe * safe) + 4 * EPS * np.abs(val)), beyond


def tri_angles(c1, c2, P, same):
    """CalculateTriangulationAngle of pairs: c1, c2, P as V [n][3], same [n] = the two cameras have bit-identical (q, t).
    Returns (ang V [n], facts) with facts = dict(den_zero, den_fragile, beyond, fold, nan) of bool [n]."""
    b = [_sub(c1[:, k], c2[:, k]) for k in range(3)]
    a1 = [_sub(P[:, k], c1[:, k]) for k in range(3)]
    a2 = [_sub(P[:, k], c2[:, k]) for k in range(3)]
    sq = lambda v: v[0] * v[0] + v[1] * v[1] + v[2] * v[2]
    b2, r1, r2 = sq(b), sq(a1), sq(a2)
    den = (r1 * r2).sqrt() * 2.0
    den_zero = den.v == 0
    den_fragile = np.where(den_zero, den.e > 0, den.v <= den.e)
    arg = (r1 + r2 - b2) / V.where(den_zero, 1.0, den)
    nan = np.isnan(arg.v)
    a, beyond = _acos(arg)
    turned = V(np.full(a.shape, PI64)) - a
    fold = (turned.v < a.v) & ~beyond
    ang = V.where(fold, turned, a)
    lo = np.maximum(np.abs(arg.v) - arg.e, 0)
    wide = np.arccos(np.where(beyond & ~nan, lo, LD(0))) * (1 + 4 * EPS) + 2 * LD(np.pi) * EPS
    ang = V.where(beyond, V(np.zeros(a.shape, LD), np.where(nan, LD(0), wide)), ang)
    exact0 = den_zero | same
    ang = V.where(exact0, 0.0, ang)
    facts = dict(den_zero=den_zero, den_fragile=den_fragile & ~same, beyond=beyond & ~nan & ~exact0, fold=fold & ~exact0, nan=nan & ~exact0)
    return ang, facts


def caller_order(obs_cam, obs_pt, n_points):
    """(order, ptr): the caller's observations by track, inside a track by camera, equal cameras in the caller's order"""
    order = np.lexsort((np.asarray(obs_cam), np.asarray(obs_pt)))
    ptr = np.searchsorted(np.asarray(obs_pt)[order], np.arange(n_points + 1))
    return order, ptr


def reference(arr, max_re, min_angle):
    """The filter of the problem `arr`.  Returns dict(obs_delete, track_outlier, num_filtered: exact integers; track_error, track_angle: V
    [Np] with -1 (bar 0) where the rule leaves them unset; re, Z: V [No] in the caller's order; fragile_obs [No], fragile_track [Np];
    facts: what the coverage table counts)."""
    ci, pi = np.asarray(arr["obs_cam"], np.int64), np.asarray(arr["obs_pt"], np.int64)
    Nc, Np, No = arr["cam_q"].shape[0], arr["points"].shape[0], ci.shape[0]
    q, t, P = (np.asarray(arr[k], F64) for k in ("cam_q", "cam_t", "points"))
    intr = np.asarray(arr["cam_intr"])[ci]
    model = np.asarray(arr["intr_model"])[intr]
    max_re, min_angle = F64(max_re), F64(min_angle)
    with np.errstate(all="ignore"):
        re, Z = project(model, np.asarray(arr["intr_params"], F64)[intr], q[ci], t[ci], P[pi], np.asarray(arr["obs_uv"], F64))
        by_re, by_zmin, by_zmax = re.v > LD(max_re), Z.v < LD(Z_MIN), Z.v > LD(Z_MAX)
        delete = by_re | by_zmin | by_zmax
        fragile_obs = _near(re, max_re) | _near(Z, Z_MIN) | _near(Z, Z_MAX)
        C = centres(q, t)
    order, ptr = caller_order(ci, pi, Np)
    n = np.diff(ptr)
    ndel = np.bincount(pi, weights=delete, minlength=Np).astype(np.int64)
    dropped = (n > 0) & (ndel >= n - 1)
    live = (n > 0) & ~dropped
    outlier = np.where(dropped, 1, 0).astype(np.uint8)
    count1 = int(n[dropped].sum() + ndel[live].sum())
    kept = order[~delete[order] & live[pi[order]]]                              # camera order inside every track
    with np.errstate(all="ignore"):
        mean = seg_sum(V(re.v[kept], re.e[kept]), pi[kept], Np) / V(np.maximum(n - ndel, 1).astype(LD))
    err = V.where(live, mean, -1.0)
    ang_v, ang_e = np.full(Np, LD(-1)), np.zeros(Np, LD)
    fragile_track = np.bincount(pi, weights=fragile_obs, minlength=Np) > 0
    same_pose = np.concatenate([q, t], axis=1)
    facts = dict(by_re=by_re, by_zmin=by_zmin, by_zmax=by_zmax, model=model, n=n, ndel=ndel, exit_kind={}, below_max=np.zeros(Np, bool),
                 fold=np.zeros(Np, bool), beyond=np.zeros(Np, bool), den_zero=np.zeros(Np, bool), nan_pair=np.zeros(Np, bool), pairs=np.zeros(Np, np.int64))
    Pv = V(P)
    for j in np.nonzero(live)[0]:
        ids = order[ptr[j]:ptr[j + 1]]
        cams = ci[ids[~delete[ids]]]
        ia, ib = np.triu_indices(len(cams), 1)                               # row-major: the order of the two loops
        ca, cb = cams[ia], cams[ib]
        same = (same_pose[ca].view(np.uint64) == same_pose[cb].view(np.uint64)).all(axis=1)
        with np.errstate(all="ignore"):
            ang, f = tri_angles(C[ca], C[cb], Pv[np.full(len(ca), j)], same)
        over = np.nonzero(ang.v > LD(min_angle))[0]
        last = int(over[0]) if len(over) else len(ca) - 1
        seen = slice(0, last + 1)
        if len(over):
            best, bar = ang.v[last], ang.e[last]
            facts["exit_kind"][j] = "first" if last == 0 else "later"
            facts["below_max"][j] = bool(ang.v.max() > best)
        else:
            best, bar = (ang.v.max(), ang.e.max()) if len(ca) else (LD(0), LD(0))
            facts["exit_kind"][j] = "none"
        ang_v[j], ang_e[j] = best, bar
        if best < LD(min_angle):
            outlier[j] = 2
        fragile_track[j] |= bool((_near(ang[seen], min_angle) | f["den_fragile"][seen]).any())
        for k in ("fold", "beyond", "den_zero"):
            facts[k][j] = bool(f[k][seen].any())
        facts["nan_pair"][j] = bool(f["nan"][seen].any())
        facts["pairs"][j] = last + 1
    return dict(obs_delete=delete.astype(np.uint8), track_outlier=outlier, num_filtered=np.array([count1, int((outlier == 2).sum())]),
                track_error=err, track_angle=V(ang_v, ang_e), re=re, Z=Z, fragile_obs=fragile_obs, fragile_track=fragile_track, facts=facts)


# ------------------------------------------------------------------------------------------------ the checker
def _ratio(got, ref):
    """|got - value| / bar per element as float64; a bar of zero and a NaN value ask for the same bits (0, else inf)"""
    got = np.asarray(got, LD)
    with np.errstate(all="ignore"):
        err = np.abs(got - ref.v)
        out = np.where((err == 0) | (np.isnan(got) & np.isnan(ref.v)), LD(0), LD(np.inf))
        np.divide(err, ref.e, out=out, where=(ref.e > 0) & np.isfinite(err) & np.isfinite(ref.e))
    return np.asarray(out, F64)


def check(ref, got):
    """{check: ratios to the bar}: obs_delete, track_outlier and num_filtered bit for bit (0 / inf per element); track_error and track_angle
    per track against its own bar, -1.0 exactly where the rule leaves them unset."""
    out = {k: np.where(np.asarray(got[k]).astype(np.int64) == np.asarray(ref[k]).astype(np.int64), 0.0, np.inf) for k in CHECKS[:3]}
    for k in CHECKS[3:]:
        out[k] = _ratio(got[k], ref[k])
    return out


def worst(checks):
    return {k: (float(np.max(v)) if np.size(v) else 0.0) for k, v in checks.items()}


def failures(checks):
    return {k: (x, int(np.argmax(checks[k]))) for k, x in worst(checks).items() if not x <= 1.0}


# ------------------------------------------------------------------------------------------------ the float64 restatement
MUTATIONS = ("re_ge", "zmin_le", "zmax_le", "ndel_ge_n", "count_ndel", "mean_over_n", "single_focal", "max_all_pairs", "exit_ge", "outlier_le",
             "reversed_pairs", "no_fold", "centre_M_t", "clamp_z", "no_scatter")


def _mat64(q):
    x, y, z, w = (F64(v) for v in q)
    return [F64(1.0) - F64(2.0) * (y * y + z * z), F64(2.0) * (x * y - w * z), F64(2.0) * (x * z + w * y),
            F64(2.0) * (x * y + w * z), F64(1.0) - F64(2.0) * (x * x + z * z), F64(2.0) * (y * z - w * x),
            F64(2.0) * (x * z - w * y), F64(2.0) * (y * z + w * x), F64(1.0) - F64(2.0) * (x * x + y * y)]


def project64(q, t, model, k, P, mut=()):
    """(u, v, Z) of one point in one camera, float64, the kernel's expressions"""
    M = _mat64(q)
    X = M[0] * P[0] + M[1] * P[1] + M[2] * P[2] + t[0]
    Y = M[3] * P[0] + M[4] * P[1] + M[5] * P[2] + t[1]
    Z = M[6] * P[0] + M[7] * P[1] + M[8] * P[2] + t[2]
    Zd = max(Z, F64(1e-2)) if "clamp_z" in mut else Z
    xn, yn = X / Zd, Y / Zd
    r2 = xn * xn + yn * yn
    if model == 0:
        fx, fy, cx, cy, du, dv = k[0], k[0], k[1], k[2], xn, yn
    elif model == 1:
        fx, fy, cx, cy, du, dv = k[0], k[1], k[2], k[3], xn, yn
    elif model == 2:
        fx, fy, cx, cy, du, dv = k[0], k[0], k[1], k[2], xn * (k[3] * r2), yn * (k[3] * r2)
    elif model == 3:
        fx, fy, cx, cy, du, dv = k[0], k[1], k[2], k[3], xn * (k[4] * r2), yn * (k[4] * r2)
    else:
        fx, fy, cx, cy = k[0], k[1], k[2], k[3]
        rad, xy = k[4] * r2 + k[5] * r2 * r2, xn * yn
        du = xn * rad + F64(2.0) * k[6] * xy + k[7] * (r2 + F64(2.0) * xn * xn)
        dv = yn * rad + F64(2.0) * k[7] * xy + k[6] * (r2 + F64(2.0) * yn * yn)
    if "single_focal" in mut and model in (0, 1):
        du, dv = F64(0.0), F64(0.0)
    return fx * (xn + du) + cx, fy * (yn + dv) + cy, Z


def _angle64(c1, c2, P, mut, stats):
    b2 = r1 = r2 = F64(0.0)
    for k in range(3):
        b, a1, a2 = c1[k] - c2[k], P[k] - c1[k], P[k] - c2[k]
        b2 += b * b; r1 += a1 * a1; r2 += a2 * a2
    den = F64(2.0) * np.sqrt(r1 * r2)
    if den == 0.0:
        stats["den_zero"] += 1
        return F64(0.0)
    x = (r1 + r2 - b2) / den
    stats["arg_above_1"] += int(x > 1.0)
    stats["arg_is_1"] += int(x == 1.0)
    ang = np.abs(np.arccos(x))
    if "no_fold" in mut:
        return ang
    stats["fold"] += int(PI64 - ang < ang)
    return ang if np.isnan(ang) else min(ang, PI64 - ang)         # std::min(NaN, .) is NaN; fmin(NaN, NaN) too


def restate64(arr, max_re, min_angle, mut=()):
    """xrsfm_ba_filter_tracks in float64 loops: filter_tracks_impl's ordering and scatter, k_cam_centres, k_filter_tracks.  `mut`: names of
    MUTATIONS, each of which breaks one rule.  Returns the five outputs and `stats` (pairs with den == 0, an operand above 1, an operand of
    exactly 1, the fold taken)."""
    assert set(mut) <= set(MUTATIONS)
    max_re, min_angle = F64(max_re), F64(min_angle)
    ci, pi = np.asarray(arr["obs_cam"]), np.asarray(arr["obs_pt"])
    Nc, Np, No = arr["cam_q"].shape[0], arr["points"].shape[0], ci.shape[0]
    q, t, P, uv = (np.asarray(arr[k], F64) for k in ("cam_q", "cam_t", "points", "obs_uv"))
    cmodel = np.asarray(arr["intr_model"])[np.asarray(arr["cam_intr"])]
    cprm = np.asarray(arr["intr_params"], F64)[np.asarray(arr["cam_intr"])]
    ptr = np.zeros(Np + 1, np.int64)
    for i in range(No):
        ptr[pi[i] + 1] += 1
    ptr = np.cumsum(ptr)
    fill, order = ptr[:-1].copy(), np.zeros(No, np.int64)
    for i in range(No):
        order[fill[pi[i]]] = i; fill[pi[i]] += 1
    for j in range(Np):
        seg = order[ptr[j]:ptr[j + 1]]
        order[ptr[j]:ptr[j + 1]] = seg[np.argsort(ci[seg], kind="stable")]
    stats = dict(den_zero=0, arg_above_1=0, arg_is_1=0, fold=0)
    with np.errstate(all="ignore"):
        centre = np.zeros((Nc, 3))
        for c in range(Nc):
            M = _mat64(q[c])
            for k in range(3):
                centre[c, k] = -(M[3 * k] * t[c, 0] + M[3 * k + 1] * t[c, 1] + M[3 * k + 2] * t[c, 2]) if "centre_M_t" in mut else \
                    -(M[k] * t[c, 0] + M[3 + k] * t[c, 1] + M[6 + k] * t[c, 2])
        obs_del = np.zeros(No, np.uint8)
        out, err, ang_out, cnt = np.zeros(Np, np.uint8), np.full(Np, -1.0), np.full(Np, -1.0), [0, 0]
        for j in range(Np):
            beg, end = int(ptr[j]), int(ptr[j + 1])
            n = end - beg
            if n == 0:
                continue
            ndel, total = 0, F64(0.0)
            for o in range(beg, end):
                c = ci[order[o]]
                u, v, Z = project64(q[c], t[c], int(cmodel[c]), cprm[c], P[j], mut)
                e0, e1 = u - uv[order[o], 0], v - uv[order[o], 1]
                re = np.sqrt(e0 * e0 + e1 * e1)
                dele = (re >= max_re if "re_ge" in mut else re > max_re) or (Z <= Z_MIN if "zmin_le" in mut else Z < Z_MIN) \
                    or (Z >= Z_MAX if "zmax_le" in mut else Z > Z_MAX)
                obs_del[o] = 1 if dele else 0
                if dele:
                    ndel += 1
                else:
                    total += re
            if ndel >= (n if "ndel_ge_n" in mut else n - 1):
                out[j] = 1; cnt[0] += ndel if "count_ndel" in mut else n
                continue
            cnt[0] += ndel
            err[j] = total / F64(n if "mean_over_n" in mut else n - ndel)
            keep = [o for o in range(beg, end) if not obs_del[o]]
            if "reversed_pairs" in mut:
                keep = keep[::-1]
            best, done = F64(0.0), False
            for a in range(len(keep)):
                if done:
                    break
                for b in range(a + 1, len(keep)):
                    ang = _angle64(centre[ci[order[keep[a]]]], centre[ci[order[keep[b]]]], P[j], mut, stats)
                    if ang > best:
                        best = ang
                        if "max_all_pairs" not in mut and (best >= min_angle if "exit_ge" in mut else best > min_angle):
                            done = True
                            break
            ang_out[j] = best
            if best <= min_angle if "outlier_le" in mut else best < min_angle:
                out[j] = 2; cnt[1] += 1
    scattered = np.zeros(No, np.uint8)
    if "no_scatter" in mut:
        scattered[:] = obs_del
    else:
        scattered[order] = obs_del
    return dict(obs_delete=scattered, track_outlier=out, track_error=err, track_angle=ang_out, num_filtered=np.array(cnt), stats=stats)
