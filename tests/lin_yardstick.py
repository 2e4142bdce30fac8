"""Yardstick, cases and checks of the linearisation tests (tests/test_lin_cpu.py, tests/test_gpu_lin.py).

The yardstick is pure numpy in np.longdouble (x87 extended: eps = 2^-64 < 2e-19, asserted), never the library.  It restates the
first stage of an LM step from the reference formulas (ba_math.h: project / huber / quat_plus; ba_kernels.h: linearize_item and
cam_gradmax_one; ba_wide.h for the 9-wide camera blocks of bal9):

    Pc = M(q) P + t;  Z < 1e-2: r = (12, 12), J = 0;  otherwise r = f (xy + d(xy)) + c - uv with xy = (X, Y) / Z and the
    distortion d of the camera model (0 / 1: d = xy, the reference's quirk that doubles f; 2 / 3: k r^2 xy; 4: OpenCV k1 k2 p1 p2;
    5: BAL-style k1 r^2 + k2 r^4 with {f, k1, k2} variable);  s = |r|^2, Huber(a): rho = s, rho' = 1 for s <= a^2 and
    rho = 2 a sqrt(s) - a^2, rho' = a / sqrt(s) beyond;  robustified residual r sqrt(rho');  camera block
    F = sqrt(rho') [-2 (j x M P) | j | d r / d(f, k1, k2)] and point block E = sqrt(rho') j M, j = d r / d Pc, the columns of
    constant blocks zero, both times the Jacobi scales 1 / (1 + sqrt(column norm^2)) of the yardstick's own unscaled blocks;
    per track Hpp = sum E^T E (6 values) and g_p = sum E^T r, per camera diag Hcc = diag sum F^T F and g_c = sum F^T r;
    cost = 1/2 sum rho;  |x_points|^2 over the variable points that have an observation, each once;  gradient max-norm with the
    unscaled gradient g / scale: max |g_p| over those points, and over the cameras that have an observation
    |q - Plus(q, -g_q)|_inf (variable rotation), |g_t|_inf (variable translation), |g_i|_inf (variable intrinsics, bal9).

Bars.  Every quantity is carried as a pair (value, bar), both long double.  The bar is the first-order running-error bound of a
float64 evaluation of the same expression: every float64 operation adds eps = 2^-53 times the absolute values it combines, and the
bars of its operands pass through its derivative taken on absolute values.  No bar is tuned to a result:

  sum / difference   bar(x +- y) = bar(x) + bar(y) + eps (|x| + |y|): one rounding, counted on |x| + |y| >= |x +- y| so that it holds
                     for either association of a longer sum and for a fused multiply-add (which rounds once where the bound counts
                     twice).  A camera-frame coordinate M P + t so gets c eps (|M| |P| + |t|) with c = 3 additions + 1 product + the
                     5 operations of an entry of M: cancellation in M P + t (a scene far from the origin) widens the bar by exactly
                     the digits it costs.
  product            bar(x y) = |x| bar(y) + |y| bar(x) + eps |x y|; products by 2 and 4 and by the 0 / 1 masks of constant blocks are
                     exact (no eps term), so a constant block's columns and a clamped observation's Jacobian have bar 0: bit for bit.
  quotient, sqrt     bar(x / y) = bar(x) / |y| + |x / y| bar(y) / |y| + eps |x / y|;  bar(sqrt x) = bar(x) / (2 sqrt x) + eps sqrt x
                     (IEEE division and square root: one rounding each).  1 / Z carries the bar of Z through the distortion polynomial
                     and the focal length to r and to every Jacobian entry this way.
  sin, cos           4 eps |value| + the operand's bar (2 ulp library functions, twice over).
  sum over L terms   per track, per camera and for the cost: sum of the terms' bars + (L + log2(64) + 2) eps sum |term|.  Any
                     summation tree over L terms has depth <= L - 1, so the bound holds for every order the kernels use (segmented
                     wave reduction, strided wave reduction, sorted LDS runs, list order in groups of G with four loads in flight,
                     the two-level tail); log2(64) + 2 is the allowance for the tree steps that add an exact zero (dead lanes, the
                     0 / 1 mask inside the fma) and is never needed by a correct sum.  L = observations of the track / camera, the
                     number of observations for the cost, the number of counted points for |x_points|^2.
  maxima             |max_i a_i - max_i b_i| <= max_i |a_i - b_i|: the bar of a max-norm is the largest bar of its candidates.
  decisions          the clamp (Z < 1e-2) and the Huber switch (s > a^2) are taken on the long-double values; an observation whose
                     Z lies within its own bar of 1e-2, or whose s within its own bar of a^2 (a^2 itself rounded to float64, as the
                     kernels form it), is FRAGILE: float64 could decide either way.  No case may contain one (test_lin_cpu.py).

The bars are per element (observation and entry, track and entry, camera and entry); none is normalised by an array-wide maximum.
"""
import numpy as np

from oracle import ba_oracle as bo
from tests import helpers as H

LD = np.longdouble
assert np.finfo(LD).eps < 2e-19, "np.longdouble carries no more than float64 here: the yardstick needs x87 extended precision"
EPS = LD(2.0) ** -53
HUBER_A = 5.99
MIN_DEPTH, CLAMP_RES = 1e-2, 12.0
SUM_EXTRA = 6 + 2               # log2(64) + c, c = 2


# ------------------------------------------------------------------------------------------------ (value, bar) arithmetic
def _pow2(x):
    m, _ = np.frexp(abs(float(x)))
    return m == 0.5 or x == 0


class V:
    """Value and running-error bar of a float64 evaluation, elementwise (np.longdouble arrays, numpy broadcasting)."""
    __slots__ = ("v", "e")

    def __init__(self, v, e=None):
        self.v = np.asarray(v, LD)
        self.e = np.zeros(self.v.shape, LD) if e is None else np.asarray(e, LD) + np.zeros(self.v.shape, LD)

    @staticmethod
    def lift(x):
        return x if isinstance(x, V) else V(x)

    @property
    def shape(self):
        return self.v.shape

    def __getitem__(self, k):
        return V(self.v[k], self.e[k])

    def __neg__(self):
        return V(-self.v, self.e)

    def __add__(self, o):
        o = V.lift(o)
        return V(self.v + o.v, self.e + o.e + EPS * (np.abs(self.v) + np.abs(o.v)))

    __radd__ = __add__

    def __sub__(self, o):
        return self + (-V.lift(o))

    def __rsub__(self, o):
        return V.lift(o) + (-self)

    def __mul__(self, o):
        exact = not isinstance(o, V) and np.ndim(o) == 0 and _pow2(o)
        o = V.lift(o)
        p = self.v * o.v
        return V(p, np.abs(self.v) * o.e + np.abs(o.v) * self.e + (0 if exact else EPS * np.abs(p)))

    __rmul__ = __mul__

    def mask(self, m):
        """times an exact 0 / 1 factor"""
        m = np.asarray(m, LD)
        return V(self.v * m, self.e * m)

    def __truediv__(self, o):
        o = V.lift(o)
        q = self.v / o.v
        return V(q, self.e / np.abs(o.v) + np.abs(q) * o.e / np.abs(o.v) + EPS * np.abs(q))

    def __rtruediv__(self, o):
        return V.lift(o) / self

    def sqrt(self):
        s = np.sqrt(self.v)
        de = np.where(self.e > 0, self.e / (2 * np.where(s > 0, s, LD(1))), LD(0))
        de = np.where((self.e > 0) & ~(s > 0), LD(np.inf), de)
        return V(s, de + EPS * s)

    def sin(self):
        s = np.sin(self.v)
        return V(s, self.e + 4 * EPS * np.abs(s))

    def cos(self):
        c = np.cos(self.v)
        return V(c, self.e + 4 * EPS * np.abs(c))

    def abs(self):
        return V(np.abs(self.v), self.e)

    @staticmethod
    def where(m, a, b):
        a, b = V.lift(a), V.lift(b)
        return V(np.where(m, a.v, b.v), np.where(m, a.e, b.e))

    @staticmethod
    def stack(xs, axis=-1):
        xs = [V.lift(x) for x in xs]
        shp = np.broadcast_shapes(*(x.shape for x in xs))
        return V(np.stack([np.broadcast_to(x.v, shp) for x in xs], axis), np.stack([np.broadcast_to(x.e, shp) for x in xs], axis))


def seg_sum(x, idx, n):
    """Sum of the rows of x [N][...] per segment idx [N] -> [n][...] with the bar of a sum over L terms (module docstring)."""
    shp = (n,) + x.shape[1:]
    s = np.zeros(shp, LD); np.add.at(s, idx, x.v)
    a = np.zeros(shp, LD); np.add.at(a, idx, np.abs(x.v))
    e = np.zeros(shp, LD); np.add.at(e, idx, x.e)
    L = np.bincount(idx, minlength=n).astype(LD).reshape((n,) + (1,) * (x.v.ndim - 1))
    return V(s, e + np.where(L > 0, L + SUM_EXTRA, 0) * EPS * a)


def _dot(a, b):
    """sum_k a[k] b[k] over short lists of V, in list order"""
    s = a[0] * b[0]
    for x, y in zip(a[1:], b[1:]):
        s = s + x * y
    return s


# ------------------------------------------------------------------------------------------------ the yardstick
def _quat_mat(q):
    x, y, z, w = (V(q[:, k]) for k in range(4))
    return [[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)],
            [2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x)],
            [2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)]]


def project(model, k, q, t, P, uv):
    """Per observation (all inputs float64, one row each): model [N], k [N][8], q [N][4], t [N][3], P [N][3], uv [N][2].
    Returns dict(r [2], jp [2][3] = d r / d Pc, ji [2][3] = d r / d(f, k1, k2), rp [3] = M P, M [3][3], Z, clamped, fragile_z) of
    V lists; the entries of a clamped observation are (12, 12) and exact zeros."""
    M = _quat_mat(q)
    Pv = [V(P[:, i]) for i in range(3)]
    rp = [_dot(M[i], Pv) for i in range(3)]
    X, Y, Z = (rp[i] + V(t[:, i]) for i in range(3))
    thr = LD(np.float64(MIN_DEPTH))
    clamped = Z.v < thr
    fragile = np.abs(Z.v - thr) <= Z.e
    ok = ~clamped
    iz = 1.0 / V.where(ok, Z, 1.0)
    xn, yn = X * iz, Y * iz
    r2 = xn * xn + yn * yn
    kk = [k[:, i] for i in range(8)]
    m = [model == i for i in range(6)]
    two = m[0] | m[2] | m[5]                         # one focal length
    sel = lambda *pairs: sum(np.where(c, v, 0.0) for c, v in pairs)
    fx = V(kk[0])
    fy = V(np.where(two, kk[0], kk[1]))
    cx = V(sel((m[0] | m[2], kk[1]), (m[1] | m[3] | m[4], kk[2])))
    cy = V(sel((m[0] | m[2], kk[2]), (m[1] | m[3] | m[4], kk[3])))
    one, zero = V(np.ones(len(model))), V(np.zeros(len(model)))
    # models 2 / 3: k r^2 (x, y)
    kr = V(np.where(m[2], kk[3], kk[4]))
    rad = kr * r2
    du_r, dv_r = xn * rad, yn * rad
    D00_r = 1.0 + rad + 2.0 * kr * xn * xn; D11_r = 1.0 + rad + 2.0 * kr * yn * yn
    D01_r = 2.0 * kr * xn * yn
    # models 4 / 5: k1, k2 (and p1, p2 of OpenCV)
    k1 = V(np.where(m[5], kk[1], kk[4])); k2 = V(np.where(m[5], kk[2], kk[5])); p1 = V(kk[6]); p2 = V(kk[7])
    rad2 = k1 * r2 + k2 * r2 * r2
    rad_x = 2.0 * k1 * xn + 4.0 * k2 * r2 * xn
    rad_y = 2.0 * k1 * yn + 4.0 * k2 * r2 * yn
    xy, x2, y2 = xn * yn, xn * xn, yn * yn
    du_b, dv_b = xn * rad2, yn * rad2
    D00_b = 1.0 + rad2 + xn * rad_x; D01_b = xn * rad_y; D10_b = yn * rad_x; D11_b = 1.0 + rad2 + yn * rad_y
    du_o = xn * rad2 + 2.0 * p1 * xy + p2 * (r2 + 2.0 * x2)
    dv_o = yn * rad2 + 2.0 * p2 * xy + p1 * (r2 + 2.0 * y2)
    D00_o = 1.0 + rad2 + xn * rad_x + 2.0 * p1 * yn + 6.0 * p2 * xn
    D01_o = xn * rad_y + 2.0 * p1 * xn + 2.0 * p2 * yn
    D10_o = yn * rad_x + 2.0 * p2 * yn + 2.0 * p1 * xn
    D11_o = 1.0 + rad2 + yn * rad_y + 2.0 * p2 * xn + 6.0 * p1 * yn
    quirk, radial = m[0] | m[1], m[2] | m[3]
    pick = lambda a, b, c, d: V.where(quirk, a, V.where(radial, b, V.where(m[4], c, d)))
    du, dv = pick(xn, du_r, du_o, du_b), pick(yn, dv_r, dv_o, dv_b)
    D00, D11 = pick(one * 2.0, D00_r, D00_o, D00_b), pick(one * 2.0, D11_r, D11_o, D11_b)
    D01, D10 = pick(zero, D01_r, D01_o, D01_b), pick(zero, D01_r, D10_o, D10_b)
    r0 = fx * (xn + du) + cx - V(uv[:, 0])
    r1 = fy * (yn + dv) + cy - V(uv[:, 1])
    A00, A01, A10, A11 = fx * D00, fx * D01, fy * D10, fy * D11
    jp = [[A00 * iz, A01 * iz, -(A00 * xn + A01 * yn) * iz], [A10 * iz, A11 * iz, -(A10 * xn + A11 * yn) * iz]]
    ji = [[xn + du, fx * xn * r2, fx * xn * r2 * r2], [yn + dv, fx * yn * r2, fx * yn * r2 * r2]]
    clamp = lambda x, val: V.where(ok, x, val)
    return dict(r=[clamp(r0, CLAMP_RES), clamp(r1, CLAMP_RES)], jp=[[clamp(x, 0.0) for x in row] for row in jp],
                ji=[[V.where(ok & m[5], x, 0.0) for x in row] for row in ji], rp=rp, M=M, Z=Z, clamped=clamped, fragile_z=fragile)


def huber(s, a=HUBER_A):
    """rho, sqrt(rho'), the branch taken and whether s is fragile; b = a^2 as float64 forms it."""
    b64 = np.float64(a) * np.float64(a)
    b = V(np.full(s.shape, b64), EPS * LD(b64))
    out = s.v > LD(b64)
    fragile = np.abs(s.v - LD(b64)) <= s.e + b.e
    rr = V.where(out, s, 1.0).sqrt()
    rho = V.where(out, 2.0 * V(np.float64(a)) * rr - b, s)
    sw = V.where(out, (V(np.float64(a)) / rr).sqrt(), 1.0)
    return rho, sw, out, fragile


def reference(arr, use_scaling, a=HUBER_A, obs_mask=None):
    """The linearisation of the problem `arr` at its own state.  Returns a dict of V (r [No][2], Jc [No][2][W], Jp [No][2][3],
    Hpp [Np][6], gp [Np][3], Hcc_diag [Nc][W], gc [Nc][W], sc_c, sc_p, cost, sum_rho, xnorm2_pts, gradmax_pts, gradmax_cams) and
    of facts (clamped, huber_out, fragile [No]; W).  W = 9 when some camera keeps its intrinsics variable (bal9), else 6."""
    ci = np.asarray(arr["obs_cam"], np.int64); pi = np.asarray(arr["obs_pt"], np.int64)
    Nc, Np, No = arr["cam_q"].shape[0], arr["points"].shape[0], ci.shape[0]
    cc = np.asarray(arr["cam_const"]).astype(np.int64)
    wide = bool((cc & 4).any())
    W = 9 if wide else 6
    intr = np.asarray(arr["cam_intr"])[ci]
    model = np.asarray(arr["intr_model"])[intr]
    pj = project(model, np.asarray(arr["intr_params"], np.float64)[intr], np.asarray(arr["cam_q"], np.float64)[ci],
                 np.asarray(arr["cam_t"], np.float64)[ci], np.asarray(arr["points"], np.float64)[pi], np.asarray(arr["obs_uv"], np.float64))
    r, j, rp, M = pj["r"], pj["jp"], pj["rp"], pj["M"]
    s = r[0] * r[0] + r[1] * r[1]
    rho, sw, hout, fragile_s = huber(s, a)
    rt = V.stack([r[0] * sw, r[1] * sw])
    qv = ((cc & 1) == 0)[ci]; tv = ((cc & 2) == 0)[ci]; iv = ((cc & 4) != 0)[ci]
    pv = (np.asarray(arr["point_const"]) == 0)[pi]
    rows_c, rows_p = [], []
    for row in range(2):
        a0, b0, c0 = j[row]
        cross = [b0 * rp[2] - c0 * rp[1], c0 * rp[0] - a0 * rp[2], a0 * rp[1] - b0 * rp[0]]
        cols = [(-2.0 * x * sw).mask(qv) for x in cross] + [(x * sw).mask(tv) for x in (a0, b0, c0)]
        if wide:
            cols += [(x * sw).mask(iv) for x in pj["ji"][row]]
        rows_c.append(V.stack(cols))
        rows_p.append(V.stack([((a0 * M[0][k] + b0 * M[1][k] + c0 * M[2][k]) * sw).mask(pv) for k in range(3)]))
    F = V.stack(rows_c, axis=1); E = V.stack(rows_p, axis=1)            # [No][2][W], [No][2][3], unscaled
    sel = np.ones(No, bool) if obs_mask is None else np.asarray(obs_mask, bool)
    if use_scaling:
        sc_c = 1.0 / (1.0 + seg_sum(F[:, 0] * F[:, 0] + F[:, 1] * F[:, 1], ci, Nc).sqrt())
        sc_p = 1.0 / (1.0 + seg_sum(E[:, 0] * E[:, 0] + E[:, 1] * E[:, 1], pi, Np).sqrt())
        F = F * V(sc_c.v[ci][:, None, :], sc_c.e[ci][:, None, :])
        E = E * V(sc_p.v[pi][:, None, :], sc_p.e[pi][:, None, :])
    else:
        sc_c, sc_p = V(np.ones((Nc, W))), V(np.ones((Np, 3)))
    r0, r1 = rt[:, 0:1], rt[:, 1:2]
    pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
    Hpp = seg_sum(V.stack([E[:, 0, a_] * E[:, 0, b_] + E[:, 1, a_] * E[:, 1, b_] for a_, b_ in pairs]), pi, Np)
    gp = seg_sum(E[:, 0] * r0 + E[:, 1] * r1, pi, Np)
    Hcc = seg_sum(F[:, 0] * F[:, 0] + F[:, 1] * F[:, 1], ci, Nc)
    gc = seg_sum(F[:, 0] * r0 + F[:, 1] * r1, ci, Nc)
    sum_rho = seg_sum(V(rho.v[sel], rho.e[sel]), np.zeros(int(sel.sum()), np.int64), 1)[0]
    # scalars
    pt_obs = np.bincount(pi, minlength=Np) > 0
    pvar = pt_obs & (np.asarray(arr["point_const"]) == 0)
    Pw = V(np.asarray(arr["points"], np.float64)[pvar])
    xn2 = seg_sum(Pw[:, 0] * Pw[:, 0] + Pw[:, 1] * Pw[:, 1] + Pw[:, 2] * Pw[:, 2], np.zeros(int(pvar.sum()), np.int64), 1)[0]
    gmax_p = _max_norm([(gp / sc_p)[pvar]])
    act = np.bincount(ci, minlength=Nc) > 0
    qvar, tvar, ivar = act & ((cc & 1) == 0), act & ((cc & 2) == 0), act & ((cc & 4) != 0)
    gu = gc / sc_c
    cand = [gu[tvar][:, 3:6]]
    if wide:
        cand.append(gu[ivar][:, 6:9])
    if qvar.any():
        q = np.asarray(arr["cam_q"], np.float64)[qvar]
        cand.append(_quat_plus_diff([V(q[:, k]) for k in range(4)], [-gu[qvar][:, k] for k in range(3)]))
    return dict(r=rt, Jc=F, Jp=E, Hpp=Hpp, gp=gp, Hcc_diag=Hcc, gc=gc, sc_c=sc_c, sc_p=sc_p, sum_rho=sum_rho, cost=sum_rho * 0.5,
                xnorm2_pts=xn2, gradmax_pts=gmax_p, gradmax_cams=_max_norm(cand), W=W, clamped=pj["clamped"], huber_out=hout,
                fragile=pj["fragile_z"] | (fragile_s & ~pj["clamped"]), sw=sw, Z=pj["Z"], s=s, active_cam=act, pvar=pvar, pt_obs=pt_obs)


def _max_norm(parts):
    """max |.| over the entries of a list of V; its bar is the largest bar of an entry (0-d V; 0 with bar 0 when there is none)."""
    v = np.concatenate([np.abs(p.v).reshape(-1) for p in parts] + [np.zeros(1, LD)])
    e = np.concatenate([p.e.reshape(-1) for p in parts] + [np.zeros(1, LD)])
    return V(v.max(), e.max())


def _quat_plus_diff(q, d):
    """q - Plus(q, d) of ceres::EigenQuaternionParameterization (ba_math.h: quat_plus), [n][4] V; exactly 0 where d = 0."""
    n = (d[0] * d[0] + d[1] * d[1] + d[2] * d[2]).sqrt()
    nz = n.v > 0
    s = n.sin() / V.where(nz, n, 1.0)
    ax, ay, az = s * d[0], s * d[1], s * d[2]
    aw = n.cos()
    bx, by, bz, bw = q
    ow = aw * bw - (ax * bx + ay * by + az * bz)
    ox = aw * bx + bw * ax + (ay * bz - az * by)
    oy = aw * by + bw * ay + (az * bx - ax * bz)
    oz = aw * bz + bw * az + (ax * by - ay * bx)
    return V.stack([V.where(nz, b - o, 0.0) for b, o in ((bx, ox), (by, oy), (bz, oz), (bw, ow))])


# ------------------------------------------------------------------------------------------------ checks
def ratio(got, ref):
    """|got - ref.v| / ref.e elementwise as float64; where the bar is zero the value must be exact (0, else inf)."""
    err = np.abs(np.asarray(got, LD) - ref.v)
    out = np.where(err == 0, LD(0), LD(np.inf))
    np.divide(err, ref.e, out=out, where=ref.e > 0)
    return np.asarray(out, np.float64)


PER_OBS = ("r", "Jc", "Jp")
PER_TRACK = ("Hpp", "gp")
PER_CAM = ("Hcc_diag", "gc")
SCALARS = ("cost", "sum_rho", "xnorm2_pts", "gradmax_pts", "gradmax_cams")


def check_all(ref, got):
    """{check: ratios to the bar} for every key of `got` the yardstick knows; exact facts as 0 / inf:
    clamped_r / clamped_J (a clamped observation gives (12, 12) sqrt(rho') as float64 forms it, and a zero Jacobian)."""
    out = {}
    for k in PER_OBS + PER_TRACK + PER_CAM + SCALARS:
        if k in got and got[k] is not None:
            out[k] = ratio(got[k], ref[k]).reshape(-1)
    cl = ref["clamped"]
    if cl.any() and "r" in got:
        a = np.float64(HUBER_A)
        want = np.float64(CLAMP_RES) * np.sqrt(a / np.sqrt(np.float64(2 * CLAMP_RES * CLAMP_RES)))
        out["clamped_r"] = np.where(np.asarray(got["r"])[cl] == want, 0.0, np.inf).reshape(-1)
        out["clamped_J"] = np.where(np.concatenate([np.asarray(got["Jc"])[cl].reshape(-1), np.asarray(got["Jp"])[cl].reshape(-1)]) == 0, 0.0, np.inf)
    return out


def worst(checks):
    return {k: ((float(np.max(v)), int(np.argmax(v))) if np.size(v) else (0.0, -1)) for k, v in checks.items()}


def assert_inside(checks, what):
    w = worst(checks)
    bad = {k: x for k, x in w.items() if not x[0] <= 1.0}
    assert not bad, f"{what}: outside the bar (ratio, flat index): {bad}"
    return w


# ------------------------------------------------------------------------------------------------ the float64 restatement
def float64_restatement(arr, use_scaling, a=HUBER_A):
    """The oracle's linearisation in plain float64 (bo.evaluate, bo._Linearization; the scalars as bo.solve forms them), in the
    layout of capi.Context.debug_linearize / debug_wide plus debug_lin_scalars."""
    pr = H.to_oracle(arr)
    ci, pi = pr.obs_cam, pr.obs_pt
    Nc, Np = pr.cam_q.shape[0], pr.points.shape[0]
    cost, rt, Fc, Ep = bo.evaluate(pr, pr.cam_q, pr.cam_t, pr.points, a)
    W = Fc.shape[2]
    sc_c, sc_p = np.ones((Nc, W)), np.ones((Np, 3))
    if use_scaling:
        sc_c = 1 / (1 + np.sqrt(bo._scatter_add(Nc, ci, np.sum(Fc * Fc, axis=1))))
        sc_p = 1 / (1 + np.sqrt(bo._scatter_add(Np, pi, np.sum(Ep * Ep, axis=1))))
        Fc = Fc * sc_c[ci][:, None, :]; Ep = Ep * sc_p[pi][:, None, :]
    lin = bo._Linearization(pr, rt, Fc, Ep)
    Hpp = lin.Hpp
    act = np.bincount(ci, minlength=Nc) > 0
    qvar, tvar, ivar = act & ((pr.cam_const & 1) == 0), act & ((pr.cam_const & 2) == 0), act & ((pr.cam_const & 4) != 0)
    pvar = bo._active_points(pr) & (pr.point_const == 0)
    gc, gp = lin.gc / sc_c, lin.gp / sc_p
    m = 0.0
    if qvar.any():
        m = max(m, float(np.abs(pr.cam_q[qvar] - bo.quat_plus(pr.cam_q[qvar], -gc[qvar, 0:3])).max()))
    if tvar.any():
        m = max(m, float(np.abs(gc[tvar, 3:6]).max()))
    if W == 9 and ivar.any():
        m = max(m, float(np.abs(gc[ivar, 6:9]).max()))
    return dict(r=rt, Jc=Fc, Jp=Ep, Hpp=np.stack([Hpp[:, 0, 0], Hpp[:, 0, 1], Hpp[:, 0, 2], Hpp[:, 1, 1], Hpp[:, 1, 2], Hpp[:, 2, 2]], axis=1),
                gp=lin.gp, Hcc_diag=np.einsum("nii->ni", lin.Hcc), gc=lin.gc, cost=cost, sum_rho=2 * cost,
                xnorm2_pts=float((pr.points[pvar] ** 2).sum()), gradmax_pts=float(np.abs(gp[pvar]).max()) if pvar.any() else 0.0,
                gradmax_cams=m)


# ------------------------------------------------------------------------------------------------ cases
def _ragged():
    from tests import backsub_yardstick as BY
    return BY.ragged()


def models():
    """Every camera its own intrinsics, the five reference models in turn, on the ragged problem (track lengths 1..6)."""
    return H.with_models(_ragged(), seed=3)


def bal9_ragged():
    """bal9 (model 5, 9-wide camera blocks), ragged tracks, every seventh point constant, two cameras with constant intrinsics and
    one with a constant rotation."""
    b = H.make_bal9(14, 500, 5, seed=6, dropout=0.3, min_tri_angle_deg=0.5)
    b["point_const"] = (np.arange(500) % 7 == 0).astype(np.uint8)
    cc = b["cam_const"].copy(); cc[5] &= 3; cc[9] &= 3; cc[11] |= 1; b["cam_const"] = cc
    return b


def consts():
    """cam_const 3 / 1 / 2 on three cameras, every fifth point constant, camera 9 without an observation, points 10 and 50 without
    one, every 17th point from point 3 a single-observation track, every 29th point from point 3 behind its cameras (clamp branch)."""
    arr = H.make(11, 400, 4, seed=131)
    arr["point_const"] = (np.arange(400) % 5 == 0).astype(np.uint8)
    cc = np.zeros(11, np.uint8); cc[2] = 3; cc[5] = 1; cc[7] = 2
    arr["cam_const"] = cc
    arr["points"] = np.array(arr["points"], copy=True)
    arr["points"][3::29] += np.array([0.0, 0.0, -60.0])
    keep = (arr["obs_cam"] != 9) & (arr["obs_pt"] != 10) & (arr["obs_pt"] != 50)
    first = np.zeros(keep.shape[0], bool); first[np.unique(arr["obs_pt"], return_index=True)[1]] = True
    keep &= first | (arr["obs_pt"] % 17 != 3)
    for k in ("obs_cam", "obs_pt", "obs_uv"):
        arr[k] = np.ascontiguousarray(arr[k][keep])
    return arr


def consts_tfixed():
    """Every translation constant (cam_const 2; camera 3 entirely constant): the camera part of the gradient max-norm is its
    quaternion part |q - Plus(q, -g)|_inf alone, which the translation gradient outweighs wherever a translation is variable."""
    arr = H.make(8, 200, 4, seed=132)
    cc = np.full(8, 2, np.uint8); cc[3] = 3
    arr["cam_const"] = cc
    return arr


EDGE_DEPTHS = (1e-2 * (1 + 1e-9), 1e-2 * (1 - 1e-9), 1e-2 + 1e-6, 1e3, 1e5)
EDGE_S = (1 + 1e-9, 1 - 1e-9)           # |r|^2 / a^2
EDGE_RES = (1e4, 1e8)


def _uv_of(arr, cam, P):
    """float64 projection (residual at uv = 0) of the points P [n][3] into camera `cam`."""
    n = P.shape[0]
    one = dict(arr, points=P, point_const=np.zeros(n, np.uint8), obs_cam=np.full(n, cam, np.int32), obs_pt=np.arange(n, dtype=np.int32), obs_uv=np.zeros((n, 2)))
    r, valid = bo.project(H.to_oracle(one), want_jac=False)
    return r, valid


def edges(near=True, shift=0.0):
    """Six cameras (camera 5 with the identity rotation), 90 ordinary tracks and observations placed by hand; returns (problem,
    marks) with marks = {name: observation index}.
      depth_*   a point of its own at the camera-frame position (0.1 Z, 0.05 Z, Z) of camera 1, Z = 1e-2 (1 +- 1e-9) [near], 1e-2 + 1e-6,
                1e3, 1e5; a second observation from camera 2 keeps the track ordinary
      s_*       |r|^2 = a^2 (1 +- 1e-9) [near]: the observation moved along u to that distance from the projection
      res_*     residuals of 1e4 and 1e8 px along u
      zero      a point on the optical axis of camera 5 (q = identity, P = (-t0, -t1, 7 - t2): X = Y = 0 exactly), observed at the
                principal point: the residual is exactly 0 in every arithmetic
    near = False leaves the four observations out that sit 1e-9 from a threshold.  shift: the scene translated by `shift` along every
    axis with t compensating (t - M (shift, shift, shift), rounded to float64), so that M P + t cancels log10(shift) digits."""
    arr = H.make(6, 90, 3, seed=77)
    for k in ("cam_q", "cam_t", "points", "obs_uv", "obs_cam", "obs_pt", "point_const"):
        arr[k] = np.array(arr[k], copy=True)
    # camera 5: identity rotation; its observations are re-synthesised (projection + the noise they had)
    m5 = arr["obs_cam"] == 5
    r_old, _ = bo.project(H.to_oracle(arr), want_jac=False)
    arr["cam_q"][5] = (0.0, 0.0, 0.0, 1.0)
    # keep the points where they are: camera 5 now sees them under another angle; give it the observations of the new projection
    uv5, ok5 = _uv_of(arr, 5, arr["points"][arr["obs_pt"][m5]])
    arr["obs_uv"][m5] = np.where(ok5[:, None], uv5, arr["obs_uv"][m5]) - r_old[m5]
    f64 = np.float64
    marks, newP, new_obs = {}, [], []           # new_obs: (cam, new point index, uv or None, name)
    R = lambda c: bo.rotation_from_quat(arr["cam_q"][c][None])[0].astype(LD)
    def place(cam, pc):
        return ((R(cam).T @ (np.asarray(pc, LD) - arr["cam_t"][cam].astype(LD)))).astype(f64)
    depths = [z for i, z in enumerate(EDGE_DEPTHS) if near or i >= 2]
    for z in depths:
        newP.append(place(1, (0.1 * z, 0.05 * z, z)))
        new_obs.append((1, len(newP) - 1, "proj", f"depth_{z!r}")); new_obs.append((2, len(newP) - 1, "proj", None))
    newP.append(np.array([-arr["cam_t"][5][0], -arr["cam_t"][5][1], 7.0 - arr["cam_t"][5][2]]))
    new_obs.append((5, len(newP) - 1, "pp", "zero")); new_obs.append((4, len(newP) - 1, "proj", None))
    n0 = arr["points"].shape[0]
    arr["points"] = np.concatenate([arr["points"], np.array(newP)])
    arr["point_const"] = np.concatenate([arr["point_const"], np.zeros(len(newP), np.uint8)])
    oc = np.array([o[0] for o in new_obs], np.int32); op = np.array([n0 + o[1] for o in new_obs], np.int32)
    uvn = np.zeros((len(new_obs), 2))
    for i, (cam, pj, how, name) in enumerate(new_obs):
        if how == "pp":
            prm = arr["intr_params"][arr["cam_intr"][cam]]
            uvn[i] = (prm[1], prm[2])           # SIMPLE_RADIAL {f, cx, cy, k}
        else:
            r, ok = _uv_of(arr, cam, arr["points"][n0 + pj][None])
            uvn[i] = r[0] + (0.3, -0.2) if ok[0] else (100.0, 100.0)
    assert int(arr["intr_model"][arr["cam_intr"][5]]) == 2
    base = arr["obs_cam"].shape[0]
    arr["obs_cam"] = np.concatenate([arr["obs_cam"], oc]); arr["obs_pt"] = np.concatenate([arr["obs_pt"], op])
    arr["obs_uv"] = np.concatenate([arr["obs_uv"], uvn])
    for i, o in enumerate(new_obs):
        if o[3]:
            marks[o[3]] = base + i
    # residual edits on ordinary observations of camera 0 (in front of it, inside the Huber radius before the edit)
    r_now, valid = bo.project(H.to_oracle(arr), want_jac=False)
    free = [i for i in np.nonzero((arr["obs_cam"][:base] == 0) & valid[:base])[0] if (r_now[i] ** 2).sum() < 9.0]
    a = HUBER_A
    edits = [(f"s_{x!r}", a * float(np.sqrt(LD(x)))) for x in EDGE_S if near] + [(f"res_{x:g}", x) for x in EDGE_RES]
    for (name, d), i in zip(edits, free):
        arr["obs_uv"][i] = (arr["obs_uv"][i] + r_now[i]) - np.array([d, 0.0])      # projection - (d, 0): r = (d, 0) up to rounding
        marks[name] = int(i)
    if shift:
        d = np.full(3, shift, LD)
        arr["points"] = (arr["points"].astype(LD) + d).astype(f64)
        for c in range(6):
            arr["cam_t"][c] = (arr["cam_t"][c].astype(LD) - R(c) @ d).astype(f64)
    order = np.lexsort((arr["obs_pt"], arr["obs_cam"]))
    inv = np.empty_like(order); inv[order] = np.arange(order.shape[0])
    for k in ("obs_cam", "obs_pt", "obs_uv"):
        arr[k] = np.ascontiguousarray(arr[k][order])
    return arr, {k: int(inv[v]) for k, v in marks.items()}


def band(n_cams):
    """n_cams cameras, two-observation tracks (c, c + 1) along the band and five more (c, c + 2); one camera: five tracks of one
    observation."""
    if n_cams == 1:
        arr = H.make_tracks(2, [np.array([0])] * 5, seed=1)
        for k in ("cam_q", "cam_t", "cam_const", "cam_intr"):
            arr[k] = np.ascontiguousarray(arr[k][:1])
        return arr
    tracks = [np.array([c, c + 1]) for c in range(n_cams - 1)] + [np.array([c, c + 2]) for c in range(0, min(n_cams - 2, 5))]
    return H.make_tracks(n_cams, tracks, seed=n_cams)


PARTIALS6 = (0, 1, 2, 20, 21, 22, 83, 84, 85, 300)       # G +- 1 and 4 G +- 1 for G = 256 / 12 = 21, and a long list
PARTIALS9 = (0, 13, 14, 15, 55, 56, 57)                  # G = 256 / 18 = 14


def cams_single(counts, seed):
    """Single-observation tracks only: camera i holds counts[i] of them.  (The packing sorts the tracks by camera tuple, so a 6-wide
    context meets them as stride-1 regular tiles and as Gram tiles where two cameras share a tile, one partial per camera and tile;
    a bal9 context as one partial per observation where a tile holds one camera.)"""
    return H.make_tracks(len(counts), [np.array([c]) for c, n in enumerate(counts) for _ in range(n)], seed=seed)


def cams_partials(counts, seed):
    """Camera i holds counts[i] observations and as many partials in the camera-major list k_lin_tail / k_cam_segsum add up: every
    track is (i, a camera of its own), so that no two tracks of a tile share a tuple (no regular tile) and every tile sees more than
    10 cameras (no Gram tile): one partial per observation.  A last camera with 40 tracks closes the list, so that the tile that
    ends the packing holds none of the counted cameras."""
    counts = tuple(counts) + (40,)
    nxt, tracks = len(counts), []
    for c, n in enumerate(counts):
        for _ in range(n):
            tracks.append(np.array([c, nxt])); nxt += 1
    return H.make_tracks(nxt, tracks, seed=seed)


def _bal9(arr, seed):
    from xrsfm_amd import synth
    return synth.to_bal9(arr, seed)


_SHAPES = {}


def _shape(i):
    if not _SHAPES:
        _SHAPES["all"] = H.shape_problems()
    return _SHAPES["all"][i][0]


LONG = ((65,), (128,), (129,), (200,), (65, 128, 129, 200))
BAND = (1, 7, 8, 9, 1023, 1024, 1025, 2049)
# name -> factory
CASES = {
    **{f"shape{i}": (lambda i=i: _shape(i)) for i in range(21)},
    **{"long" + "_".join(map(str, L)): (lambda L=L: H.long_problem(L, seed=31 + len(L) + L[0])) for L in LONG},
    "models": models, "bal9_ragged": bal9_ragged,
    "consts": consts, "consts_tfixed": consts_tfixed,
    "edges": lambda: edges()[0], "edges_far": lambda: edges(near=False, shift=1e5)[0],
    **{f"band{n}": (lambda n=n: band(n)) for n in BAND},
    "cams_single": lambda: cams_single(PARTIALS6, 3), "cams_partials": lambda: cams_partials(PARTIALS6, 4),
    "bal9_cams_single": lambda: _bal9(cams_single(PARTIALS9, 5), 5), "bal9_cams_partials": lambda: _bal9(cams_partials(PARTIALS9, 6), 6),
}
FAMILIES = {"shapes": tuple(f"shape{i}" for i in range(21)), "long": tuple(n for n in CASES if n.startswith("long")),
            "models": ("models",), "consts": ("consts", "consts_tfixed"), "edges": ("edges", "edges_far"),
            "cams": tuple(n for n in CASES if n.startswith(("band", "cams_"))),
            "bal9": ("bal9_ragged", "bal9_cams_single", "bal9_cams_partials")}
assert sorted(n for f in FAMILIES.values() for n in f) == sorted(CASES)
_ARR, _REF = {}, {}


def family_of(name):
    return next(f for f, names in FAMILIES.items() if name in names)


def is_wide(name):
    return name.startswith("bal9")


def case(name):
    """The problem of a case (built once; callers must not modify it)."""
    if name not in _ARR:
        _ARR[name] = CASES[name]()
    return _ARR[name]


def case_reference(name, use_scaling):
    """The yardstick of a case (computed once and shared; callers must not modify it)."""
    if (name, use_scaling) not in _REF:
        _REF[(name, use_scaling)] = reference(case(name), use_scaling)
    return _REF[(name, use_scaling)]


# ------------------------------------------------------------------------------------------------ coverage, from the packing (no GPU)
def coverage(arr):
    """What the host-side packing makes of a problem: tiles per reduction branch of linearize_item (regular = strided_reduce,
    gram_ragged = sorted LDS runs, per_obs = one partial per observation, long = tiles of items of several tiles), the tile counts of
    its items and, per camera, the number of partials in the camera-major list (distinct positions its slots write to)."""
    from xrsfm_amd import capi
    prod = H.to_product(arr)
    pk = capi.debug_pack(prod); g = capi.debug_pack_gram(prod)
    stride = capi.debug_sgroup(prod)["tile_stride"]
    ncam = g["tile_ncam"]
    so, cp = pk["slot_obs"], g["slot_campos_g"]
    n_tiles = pk["tiles"]
    cam = np.where(so >= 0, np.asarray(arr["obs_cam"])[np.maximum(so, 0)], -1)
    pt = np.where(so >= 0, np.asarray(arr["obs_pt"])[np.maximum(so, 0)], -1).reshape(n_tiles, 64)
    lens = np.bincount(arr["obs_pt"], minlength=arr["points"].shape[0])
    long_tile = np.zeros(n_tiles, bool)
    item_tiles = []
    t = 0
    while t < n_tiles:
        ids = np.unique(pt[t][pt[t] >= 0])
        n = -(-int(lens[ids[0]]) // 64) if len(ids) == 1 and lens[ids[0]] > 64 else 1
        long_tile[t:t + n] = n > 1
        item_tiles.append(n); t += n
    assert len(item_tiles) == pk["items"] and sum(n > 1 for n in item_tiles) == pk["long_items"]
    assert not (stride[long_tile] > 0).any() and not (ncam[long_tile] > 0).any()
    klass = np.where(long_tile, "long", np.where(stride > 0, "regular", np.where(ncam > 0, "gram_ragged", "per_obs")))
    Nc = arr["cam_q"].shape[0]
    key = np.unique(np.stack([cam[cp >= 0], cp[cp >= 0]], axis=1), axis=0) if (cp >= 0).any() else np.zeros((0, 2), np.int64)
    partials = np.bincount(key[:, 0], minlength=Nc)
    assert partials.sum() == len(np.unique(cp[cp >= 0]))          # no position shared by two cameras
    return dict(tiles={k: int((klass == k).sum()) for k in ("regular", "gram_ragged", "per_obs", "long")}, item_tiles=set(item_tiles),
                partials=partials, obs_per_cam=np.bincount(arr["obs_cam"], minlength=Nc), grid=min(1024, max(Nc, 1)),
                models=set(int(m) for m in np.asarray(arr["intr_model"])[np.asarray(arr["cam_intr"])[arr["obs_cam"]]]),
                cam_const=set(int(c) & 3 for c in arr["cam_const"]), track_lens=set(int(x) for x in lens))
