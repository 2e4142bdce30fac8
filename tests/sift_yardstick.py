"""The yardstick of xrsfm_ba_detect_keypoints: the rule of xrsfm_amd/csrc/ba_sift_rule.h in pure numpy, once in
np.longdouble and once in float32, both from the SAME float32 taps and thresholds, a catalogue of small 8-bit images with fixed
seeds, and the bars.

Bars (eps = 2^-24; every value of a level lies in [0, 1] and every filter's weights sum to 1):
  Gaussian level   a pass of W taps adds at most (W + 1) eps (W products, W sums of partial sums <= 1, minus the first sum with
                   0, plus the rounding of the weights' own normalisation carried as one more unit); the x2 up-sample adds 3 eps
                   (two products and a sum, once per direction with exact weights 0.5: 3 roundings that are not exact); the byte
                   to float division 1 eps; the down-sample nothing.  The bar of a level is the sum over the operations on the way
                   to it, times FMA_FACTOR = 1: a kernel that contracts a * b + c rounds once where this count has two (as
                   lin_yardstick.py counts it), so contraction needs no widening.
  DoG level        the operations on the way to its newer Gaussian level plus its own one rounding of a value below 1 (eps).
  Key decision     a tested pixel is FRAGILE if a comparison on its decision path, evaluated in longdouble, has a margin below the
                   bars of the two quantities compared.  With e the largest DoG bar of the three levels read: |v| against T0: e;
                   v against a neighbour: 2 e; fxx, fyy, fss = a + b - 2 v: 4 e, the mixed terms 0.25 (a + b - c - d): e, the
                   gradient 0.5 (a - b): e; temp1 = fxx fyy - fxy^2: 4 e (|fxx| + |fyy|) + 2 e |fxy| + 4 eps |fxx fyy|; temp2 =
                   (fxx + fyy)^2: 16 e |fxx + fyy| + 4 eps temp2; the first pivot (the largest of |fxx|, |fxy|, |fxs|): 8 e
                   between the largest two; the second pivot and the guards on values after one and two elimination steps: those
                   values carry the growth of the elimination: an entry a - r m after a step with multiplier row m = pivot row / pivot
                   and ratio r = a_x / pivot (|r| <= 1) has the bar g = 4 e (1 + |m|) (1 + |r|), and one step more multiplies it by
                   (1 + |m'|) (1 + |r'|) again; two values are compared under the sum of their bars; the
                   offsets and the contrast: |H^-1| (12 e |x| + e) for the solve's sensitivity to the 4 e / e bars of its matrix and
                   right-hand side plus 64 eps cond(H) |x| for the float32 elimination, |x| the largest offset.
  Offsets, X, Y, S on keypoints found by both: within 16 times the float32 restatement's own measured deviation from longdouble
                   (measured_deviation()), as pose_yardstick.py and init_yardstick.py do.

Measured on the catalogue (float32 restatement against longdouble, this file's __main__; also in profiles/keypoint_detect.md):
the largest level deviation is 2.8e-7 (Gaussian) and 3.8e-7 (DoG) against bars from 1.7e-6 (first Gaussian level) to 2.8e-5;
the offsets deviate by at most 4.6e-4, X and Y by 4.6e-4 px, S by 6.8e-5; 1444 keypoints in the union, 36 of them fragile
(2.5 %), no mismatch.  The kernels on an MI355X: level deviations up to 3.8e-7, offsets and values within 0.1 of the 16x bar.
"""
import functools

import numpy as np

F = np.float32
EPS = 2.0 ** -24
FMA_FACTOR = 1.0
DEFAULTS = dict(first_octave=-1, num_octaves=4, peak_threshold=float(F(0.02) / F(3)), edge_threshold=10.0, max_num_features=8192, max_image_size=3200)
WHY = ("kept", "threshold", "centre_row", "neighbour", "edge_det", "edge_ratio", "contrast", "off_ds", "off_dx", "off_dy", "kept_guard")


def options(**kw):
    o = dict(DEFAULTS)
    o.update(kw)
    return o


# ------------------------------------------------------------------------------------------------- parameters, taps, geometry
def taps(sigma):
    """CreateFilterKernel in float32; the exponential in double on the float argument"""
    sigma = F(sigma)
    sz = int(np.ceil(float(F(4) * sigma) - 0.5))
    width = 2 * sz + 1
    if width > 33:
        sz, width = 16, 33
    elif width < 5:
        sz, width = 2, 5
    rv = F(1) / (sigma * sigma)
    k = np.zeros(width, F)
    ksum = F(0)
    for i in range(-sz, sz + 1):
        arg = F(-0.5) * F(i) * F(i) * rv
        k[i + sz] = F(np.exp(np.float64(arg)))
        ksum = F(ksum + k[i + sz])
    return (k * (F(1) / ksum)).astype(F)


@functools.lru_cache(None)
def params(first_octave=-1, peak_threshold=DEFAULTS["peak_threshold"], edge_threshold=10.0):
    p2 = lambda x: F(np.float64(2.0) ** np.float64(F(x)))           # powf(2, x), correctly rounded
    k = p2(F(1) / F(3))
    sigma0 = F(F(1.6) * k)
    dsigma0 = F(sigma0 * np.sqrt(F(F(1) - F(1) / F(k * k))))
    level_sigma = [F(dsigma0 * F(np.float64(k) ** i)) for i in range(5)]
    sa, sb = F(sigma0 * p2(F(-1) / F(3))), F(F(0.5) / p2(F(first_octave)))
    init = F(np.sqrt(F(sa * sa - sb * sb))) if float(sa) > float(sb) + 0.001 else F(0)
    key_sigma = [F(sigma0 * p2(F(j) / F(3))) for j in range(3)]
    T, e = F(peak_threshold), F(edge_threshold)
    return dict(sigma0=sigma0, step=k, level_sigma=level_sigma, init_sigma=init, key_sigma=key_sigma, T=T, T0=F(F(0.8) * T), E=F((e + F(1)) * (e + F(1)) / e))


def geometry(width, height, first_octave=-1, num_octaves=4):
    w_in = width & ~3
    up = 1 if first_octave < 0 else 0
    w0, h0 = w_in << up, height << up
    n = min(num_octaves, max(1, int(np.floor(np.log2(min(w0, h0)))) - 3))
    return [(((w0 >> o) + 3) // 4 * 4, h0 >> o) for o in range(n)]


# ------------------------------------------------------------------------------------------------- the pyramid
def _filter(a, tp, dt):
    sz, (h, w) = len(tp) // 2, a.shape
    t = tp.astype(dt)
    pad = np.pad(a, ((0, 0), (sz, sz)), mode="edge")
    v = np.zeros((h, w), dt)
    for i in range(len(tp)):
        v = v + pad[:, i:i + w] * t[i]
    pad = np.pad(v, ((sz, sz), (0, 0)), mode="edge")
    v = np.zeros((h, w), dt)
    for i in range(len(tp)):
        v = v + pad[i:i + h, :] * t[i]
    return v


def _upsample(a, dt):
    h, w = a.shape
    f, last = a.ravel(), w * h - 1
    dr, dc = np.meshgrid(np.arange(2 * h), np.arange(2 * w), indexing="ij")
    row, col = dr >> 1, dc >> 1
    index = row * w + col
    index2 = np.minimum(row + 1, h - 1) * w + col
    half = dt(0.5)
    v11, v12, v21, v22 = f[index], f[np.minimum(index + 1, last)], f[index2], f[np.minimum(index2 + 1, last)]
    odd = (dr & 1) == 1
    v1 = np.where(odd, v21 * half + half * v11, v11)
    v2 = np.where(odd, v22 * half + half * v12, v12)
    return np.where((dc & 1) == 1, v1 * half + v2 * half, v1).astype(dt)


def _pyramid(img, first_octave, num_octaves, dt):
    """[(G [6][h][w], D [5][h][w])] per octave"""
    P = params(first_octave)
    h, w = img.shape
    geo = geometry(w, h, first_octave, num_octaves)
    a = (img[:, :w & ~3].astype(F) / F(255)).astype(dt)              # the division is part of the input: both start from the same floats
    if first_octave < 0:
        a = _upsample(a, dt)
    if P["init_sigma"] > 0:
        a = _filter(a, taps(P["init_sigma"]), dt)
    out = []
    for o, (ws, hs) in enumerate(geo):
        if o > 0:
            src = out[-1][0][3]
            cols = np.minimum(np.arange(ws) << 1, src.shape[1] - 1)
            a = src[(np.arange(hs) << 1)[:, None], cols[None, :]]
        assert a.shape == (hs, ws), (a.shape, hs, ws)
        G = [a]
        for i in range(5):
            G.append(_filter(G[-1], taps(P["level_sigma"][i]), dt))
        out.append((np.stack(G), np.stack([G[j + 1] - G[j] for j in range(5)])))
    return out


def pyramid(img, first_octave=-1, num_octaves=4, long=True):
    return _pyramid(np.asarray(img), first_octave, num_octaves, np.longdouble if long else F)


def level_bars(first_octave=-1, num_octaves=4):
    """[octave] -> (bars of G[0..5], bars of D[0..4])"""
    P = params(first_octave)
    ops = 1.0 + (3.0 if first_octave < 0 else 0.0)
    if P["init_sigma"] > 0:
        ops += 2 * (len(taps(P["init_sigma"])) + 1)
    out = []
    for o in range(num_octaves):
        g = [ops]
        for i in range(5):
            g.append(g[-1] + 2 * (len(taps(P["level_sigma"][i])) + 1))
        gb = [FMA_FACTOR * EPS * x for x in g]
        out.append((gb, [gb[j + 1] + EPS for j in range(5)]))
        ops = g[3]
    return out


# ------------------------------------------------------------------------------------------------- the key decision
def decide(Pn, Cn, Nn, T0, T, E, dt=F, bar=None):
    """ComputeKEY_Kernel on N neighbourhoods [N][3][3] (previous, own, next level) at once.  Returns sign, dx, dy, ds, why and, with
    bar (the DoG bar e, longdouble only), fragile."""
    Pn, Cn, Nn = (np.asarray(x, dt) for x in (Pn, Cn, Nn))
    n = len(Cn)
    T0, T, E = dt(T0), dt(T), dt(E)
    v = Cn[:, 1, 1]
    alive = np.ones(n, bool)
    why = np.zeros(n, np.int32)
    frag = np.zeros(n, bool)
    e = dt(bar if bar is not None else 0)

    def reject(mask, code):
        nonlocal alive
        m = alive & mask
        why[m] = code
        alive = alive & ~mask

    frag_tag = np.zeros(n, np.int32)              # which comparison made the pixel fragile (the first), for the profile

    def near(a, b, tol, tag=1):
        if bar is not None:
            m = alive & (np.abs(a - b) < tol)
            frag_tag[m & ~frag] = tag
            frag[m] = True
    near(np.abs(v), T0, e, 1)
    reject(np.abs(v) <= T0, 1)
    nmax, nmin = np.maximum(Cn[:, 1, 0], Cn[:, 1, 2]), np.minimum(Cn[:, 1, 0], Cn[:, 1, 2])
    near(v, Cn[:, 1, 0], 2 * e, 2); near(v, Cn[:, 1, 2], 2 * e, 2)
    reject((v <= nmax) & (v >= nmin), 2)

    def cmp_row(r):
        nonlocal nmax, nmin
        for q in range(3):
            near(v, r[:, q], 2 * e, 3)
        up = v > nmax
        m3 = np.maximum(np.maximum(r[:, 0], r[:, 1]), r[:, 2])
        n3 = np.minimum(np.minimum(r[:, 0], r[:, 1]), r[:, 2])
        nmax = np.where(up, np.maximum(nmax, m3), nmax)
        nmin = np.where(up, nmin, np.minimum(nmin, n3))
        reject(np.where(up, v < nmax, v > nmin), 3)
    cmp_row(Cn[:, 0]); cmp_row(Cn[:, 2])
    two = dt(2); q4 = dt(0.25); hf = dt(0.5)
    vx2 = v * two
    fxx = Cn[:, 1, 0] + Cn[:, 1, 2] - vx2
    fyy = Cn[:, 0, 1] + Cn[:, 2, 1] - vx2
    fxy = q4 * (Cn[:, 2, 2] + Cn[:, 0, 0] - Cn[:, 2, 0] - Cn[:, 0, 2])
    temp1 = fxx * fyy - fxy * fxy
    temp2 = (fxx + fyy) * (fxx + fyy)
    b1 = 4 * e * (np.abs(fxx) + np.abs(fyy)) + 2 * e * np.abs(fxy) + dt(4 * EPS) * np.abs(fxx * fyy)
    b2 = 16 * e * np.abs(fxx + fyy) + dt(4 * EPS) * temp2
    near(temp1, 0, b1, 4)
    reject(temp1 <= 0, 4)
    near(temp2, E * temp1, b2 + E * b1, 5)
    reject(temp2 > E * temp1, 5)
    for lev in (Pn, Nn):
        for r in range(3):
            cmp_row(lev[:, r])
    fx, fy, fs = hf * (Cn[:, 1, 2] - Cn[:, 1, 0]), hf * (Cn[:, 2, 1] - Cn[:, 0, 1]), hf * (Nn[:, 1, 1] - Pn[:, 1, 1])
    fss = Nn[:, 1, 1] + Pn[:, 1, 1] - vx2
    fxs = q4 * (Nn[:, 1, 2] + Pn[:, 1, 0] - Nn[:, 1, 0] - Pn[:, 1, 2])
    fys = q4 * (Nn[:, 2, 1] + Pn[:, 0, 1] - Nn[:, 0, 1] - Pn[:, 2, 1])

    def signed(lead, row):
        s = np.where(lead > 0, dt(1), dt(-1))
        return [s * x for x in row]
    A0 = signed(fxx, (fxx, fxy, fxs, -fx)); A1 = signed(fxy, (fxy, fyy, fys, -fy)); A2 = signed(fxs, (fxs, fys, fss, -fs))
    maxa = np.maximum(np.maximum(A0[0], A1[0]), A2[0])
    lead = np.stack([A0[0], A1[0], A2[0]])
    lead_bar = np.stack([np.full(n, 4 * e), np.full(n, e), np.full(n, e)])
    order = np.argsort(lead, axis=0)
    top, second = (np.take_along_axis(lead, order[k:k + 1], 0)[0] for k in (2, 1))
    near(top, second, np.take_along_axis(lead_bar, order[2:3], 0)[0] + np.take_along_axis(lead_bar, order[1:2], 0)[0], 6)
    tiny = np.float64(1e-10) if dt is F else np.longdouble(np.float64(1e-10))
    guard = np.zeros(n, bool)                      # a guard tripped: kept with offsets 0
    near(maxa, tiny, 4 * e, 7)
    g0 = ~(maxa >= tiny)
    guard |= alive & g0
    sw1 = maxa == A1[0]
    sw2 = ~sw1 & (maxa == A2[0])
    A0n = [np.where(sw1, b, np.where(sw2, c, a)) for a, b, c in zip(A0, A1, A2)]
    A1 = [np.where(sw1, a, b) for a, b in zip(A0, A1)]
    A2 = [np.where(sw2, a, c) for a, c in zip(A0, A2)]
    A0 = A0n
    with np.errstate(all="ignore"):
        piv = np.where(A0[0] == 0, dt(1), A0[0])
        A0 = [A0[0], A0[1] / piv, A0[2] / piv, A0[3] / piv]
        A1 = [A1[0]] + [A1[k] - A1[0] * A0[k] for k in (1, 2, 3)]
        A2 = [A2[0]] + [A2[k] - A2[0] * A0[k] for k in (1, 2, 3)]
        m0 = np.maximum(np.abs(A0[1]), np.abs(A0[2]))                  # the largest multiplier entry of the pivot row
        ga, gb = (4 * e * (1 + m0) * (1 + np.abs(r[0] / piv)) for r in (A1, A2))
        g1 = np.maximum(ga, gb)
        near(np.abs(A2[1]), np.abs(A1[1]), ga + gb, 8)
        sw = np.abs(A2[1]) > np.abs(A1[1])
        A1, A2 = [np.where(sw, b, a) for a, b in zip(A1, A2)], [np.where(sw, a, b) for a, b in zip(A1, A2)]
        near(np.abs(A1[1]), tiny, g1, 9)
        gA = ~(np.abs(A1[1]) >= tiny)
        guard |= alive & ~g0 & gA
        p1 = np.where(A1[1] == 0, dt(1), A1[1])
        A1 = [A1[0], A1[1], A1[2] / p1, A1[3] / p1]
        A2 = [A2[0], A2[1], A2[2] - A2[1] * A1[2], A2[3] - A2[1] * A1[3]]
        g2 = g1 * (1 + np.abs(A1[2])) * (1 + np.abs(A2[1] / p1))
        near(np.abs(A2[2]), tiny, g2, 10)
        gB = ~(np.abs(A2[2]) >= tiny)
        guard |= alive & ~g0 & ~gA & gB
        p2 = np.where(A2[2] == 0, dt(1), A2[2])
        ds = A2[3] / p2
        dy = A1[3] - ds * A1[2]
        dx = A0[3] - ds * A0[2] - dy * A0[1]
    solved = ~(g0 | gA | gB)
    dx, dy, ds = (np.where(solved, x, dt(0)) for x in (dx, dy, ds))
    contrast = np.abs(v + hf * (dx * fx + dy * fy + ds * fs))
    if bar is not None:
        H = np.stack([np.stack([fxx, fxy, fxs], -1), np.stack([fxy, fyy, fys], -1), np.stack([fxs, fys, fss], -1)], -2).astype(np.float64)
        ok = alive & solved
        boff = np.zeros(n, dt)
        if ok.any():
            with np.errstate(all="ignore"):
                inv = np.linalg.pinv(H[ok])
            ninv = np.abs(inv).sum(-1).max(-1)
            nH = np.abs(H[ok]).sum(-1).max(-1)
            xm = np.maximum(np.maximum(np.abs(dx[ok]), np.abs(dy[ok])), np.abs(ds[ok])).astype(np.float64)
            boff[ok] = ninv * (12 * float(e) * xm + float(e)) + 64 * EPS * ninv * nH * xm
        gm = np.abs(fx) + np.abs(fy) + np.abs(fs)
        sel = alive & solved
        alive_keep, alive = alive, sel
        near(contrast, T, e + hf * boff * gm + 3 * e, 11)
        for d in (ds, dx, dy):
            near(np.abs(d), 1, boff, 12)
        alive = alive_keep
    sel = alive & solved
    reject(solved & ~(contrast > T), 6)
    reject(solved & ~(np.abs(ds) < 1), 7)
    reject(solved & ~(np.abs(dx) < 1), 8)
    reject(solved & ~(np.abs(dy) < 1), 9)
    why[alive & guard] = 10
    sign = np.where(alive, np.where(v > nmax, dt(1), dt(-1)), dt(0))
    return dict(sign=sign, dx=dx, dy=dy, ds=ds, why=why, fragile=frag, fragile_tag=frag_tag)


def _gather(D, rows, cols):
    """[N][3][3] neighbourhoods of a level"""
    rr = rows[:, None, None] + np.arange(-1, 2)[None, :, None]
    cc = cols[:, None, None] + np.arange(-1, 2)[None, None, :]
    return D[rr, cc]


def detect_levels(pyr, first_octave=-1, long=True, bars=None, peak_threshold=DEFAULTS["peak_threshold"], edge_threshold=10.0):
    """every tested pixel above the threshold's reach of every (octave, level): dict (o, j) -> rows, cols and the decision arrays"""
    P = params(first_octave, peak_threshold, edge_threshold)
    dt = np.longdouble if long else F
    out = {}
    for o, (G, D) in enumerate(pyr):
        h, w = D.shape[1:]
        for j in range(3):
            C = D[j + 1]
            e = max(bars[o][1][j:j + 3]) if bars is not None else 0.0
            inner = np.zeros((h, w), bool)
            inner[1:h - 1, 1:w - 1] = True
            rows, cols = np.nonzero(inner & (np.abs(C) > float(P["T0"]) - 2 * e))
            r = decide(_gather(D[j], rows, cols), _gather(C, rows, cols), _gather(D[j + 2], rows, cols), P["T0"], P["T"], P["E"], dt, e if bars is not None else None)
            r["rows"], r["cols"] = rows, cols
            out[(o, j)] = r
    return out


def budget(level_count, n_oct, max_num_features):
    take, total = np.zeros(n_oct * 3, bool), 0
    for o in range(n_oct - 1, -1, -1):
        for j in (2, 1, 0):
            take[o * 3 + j] = not total > max_num_features
            if take[o * 3 + j]:
                total += int(level_count[o * 3 + j])
    return take, total


def key_values(o, j, rows, cols, dx, dy, ds, first_octave, dt):
    P = params(first_octave)
    os_ = dt(2.0 ** (first_octave + o))
    x, y = (cols.astype(dt) + dt(0.5)) + dx, (rows.astype(dt) + dt(0.5)) + dy
    s = dt(P["key_sigma"][j]) * np.power(dt(P["step"]), ds)
    return os_ * (x - dt(0.5)) + dt(0.5), os_ * (y - dt(0.5)) + dt(0.5), os_ * s


def reference(img, long=True, **kw):
    """the whole rule on one image: level_count, take, and per kept keypoint loc, sign, offsets, keys; 'levels' the raw decisions"""
    o = options(**kw)
    img = np.asarray(img)
    fo, dt = o["first_octave"], (np.longdouble if long else F)
    pyr = _pyramid(img, fo, o["num_octaves"], dt)
    bars = level_bars(fo, len(pyr)) if long else None
    lev = detect_levels(pyr, fo, long, bars, o["peak_threshold"], o["edge_threshold"])
    n_oct = len(pyr)
    lc = np.zeros(o["num_octaves"] * 3, np.int32)
    for (oc, j), r in lev.items():
        lc[oc * 3 + j] = int((r["sign"] != 0).sum())
    take, total = budget(lc, n_oct, o["max_num_features"])
    loc, sign, off, keys = [], [], [], []
    for oc in range(n_oct):
        for j in range(3):
            r = lev[(oc, j)]
            k = np.nonzero(r["sign"] != 0)[0]
            if not take[oc * 3 + j] or len(k) == 0:
                continue
            k = k[np.lexsort((r["cols"][k], r["rows"][k]))]
            X, Y, S = key_values(oc, j, r["rows"][k], r["cols"][k], r["dx"][k], r["dy"][k], r["ds"][k], fo, dt)
            loc.append(np.stack([np.full(len(k), oc), np.full(len(k), j), r["rows"][k], r["cols"][k]], -1).astype(np.int32))
            sign.append(r["sign"][k].astype(np.int8))
            off.append(np.stack([r["dx"][k], r["dy"][k], r["ds"][k]], -1))
            keys.append(np.stack([X, Y, S], -1))
    cat = lambda xs, shape, t: np.concatenate(xs) if xs else np.zeros(shape, t)
    return dict(level_count=lc, take=take, total=total, loc=cat(loc, (0, 4), np.int32), sign=cat(sign, (0,), np.int8), off=cat(off, (0, 3), dt),
                keys=cat(keys, (0, 3), dt), levels=lev, pyramid=pyr, bars=bars, geometry=[(D.shape[2], D.shape[1]) for _, D in pyr])


# ------------------------------------------------------------------------------------------------- the catalogue
def blobs(width, height, seed, regions, ratio=0.3, amp=(0.3, 0.5), noise=0.01, jitter=0.1):
    """Sums of Gaussian blobs on mid grey plus 1 % noise, rounded to 8 bits.  regions: (x0, y0, x1, y1, pitch); in a region the blobs
    sit on a jittered lattice of that pitch with alternating signs, amplitude 0.3-0.5 and sigma = ratio * pitch (+-10 %).  The
    alternating lattice is what keeps the catalogue's fragile share small: the negative ring that the DoG of a lone blob carries
    (a circular ridge whose extrema the noise decides, many of them close to the edge threshold) falls onto the neighbours here."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:height, 0:width].astype(np.float64)
    a = np.full((height, width), 0.5)
    for (x0, y0, x1, y1, pitch) in regions:
        for iy, gy in enumerate(np.arange(y0 + pitch / 2, y1 - pitch / 4, pitch)):
            for ix, gx in enumerate(np.arange(x0 + pitch / 2, x1 - pitch / 4, pitch)):
                cx, cy = gx + rng.uniform(-jitter, jitter) * pitch, gy + rng.uniform(-jitter, jitter) * pitch
                s = pitch * ratio * rng.uniform(0.9, 1.1)
                r = int(np.ceil(6 * s))                # (beyond 6 sigma a blob is below 1e-8: nothing of 8 bits)
                ya, yb, xa, xb = max(int(cy) - r, 0), min(int(cy) + r + 1, height), max(int(cx) - r, 0), min(int(cx) + r + 1, width)
                if ya >= yb or xa >= xb:
                    continue
                a[ya:yb, xa:xb] += rng.uniform(*amp) * (1.0 if (ix + iy) % 2 else -1.0) * np.exp(
                    -((x[ya:yb, xa:xb] - cx) ** 2 + (y[ya:yb, xa:xb] - cy) ** 2) / (2 * s * s))
    a += noise * rng.standard_normal(a.shape)
    return np.clip(np.rint(a * 255), 0, 255).astype(np.uint8)


def _bands(width, height, rows):
    """rows: [(height share, [pitches])] -> regions that tile the image"""
    out, y = [], 0.0
    total = sum(r[0] for r in rows)
    for share, pitches in rows:
        y1 = y + height * share / total
        for k, p in enumerate(pitches):
            out.append((width * k / len(pitches), y, width * (k + 1) / len(pitches), y1, p))
        y = y1
    return out


CATALOGUE = {
    # name: (width, height, seed, rows of (height share, pitches), first_octave, extra options)
    "a44x40": (44, 40, 11, [(1, [4, 6]), (1.2, [9, 13])], -1, {}),
    "b50x33": (50, 33, 12, [(1, [5, 7]), (1.3, [11])], 0, {}),
    "c64x48": (64, 48, 13, [(1, [3.6, 5, 7]), (1.5, [10, 14])], -1, {}),
    "c64x48_o0": (64, 48, 13, [(1, [3.6, 5, 7]), (1.5, [10, 14])], 0, {}),
    "d64x48": (64, 48, 14, [(1, [4.5, 6])], -1, {}),
    # (the fourth octave answers to blobs of sigma 8-13 px only: the last row goes beyond the 1-6 px of the others)
    "e300x260": (300, 260, 15, [(1, [3.4, 4.2, 5.2, 6.6]), (1, [8.5, 11, 14, 18]), (2.2, [25, 32, 42])], -1, {}),
    "budget20": (64, 48, 14, [(1, [4.5, 6])], -1, dict(max_num_features=20)),
    "budget60": (64, 48, 14, [(1, [4.5, 6])], -1, dict(max_num_features=60)),
}


@functools.lru_cache(None)
def image(name):
    w, h, seed, rows, _, _ = CATALOGUE[name]
    a = blobs(w, h, seed, _bands(w, h, rows))
    a.setflags(write=False)
    return a


def entry_options(name):
    return options(first_octave=CATALOGUE[name][4], **CATALOGUE[name][5])


@functools.lru_cache(None)
def catalogue_reference(name, long=True, first_octave=None):
    """the reference of a catalogue image; first_octave: in the other mode than its own"""
    o = entry_options(name)
    if first_octave is not None:
        o["first_octave"] = first_octave
    return reference(image(name), long, **o)


def translated(dx, dy, name="c64x48", canvas=(96, 80)):
    """the content of a catalogue image on a mid-grey canvas at offset (dx, dy)"""
    a = np.full((canvas[1], canvas[0]), 128, np.uint8)
    src = image(name)
    a[dy:dy + src.shape[0], dx:dx + src.shape[1]] = src
    return a


def filter_reach(first_octave=-1, n_oct=4):
    """per octave, in that octave's pixels: the distance from an image border beyond which no clamped read can reach a DoG value
    the key test of a pixel reads: the half widths of the filters on the way (through the octaves: G[0] of an octave is every
    second pixel of G[3] of the one before), the up-sample's neighbour and the key test's own pixel"""
    P = params(first_octave)
    hw = [len(taps(s)) // 2 for s in P["level_sigma"]]
    base = (2 if first_octave < 0 else 0) + (len(taps(P["init_sigma"])) // 2 if P["init_sigma"] > 0 else 0)
    out = []
    for _ in range(n_oct):
        out.append(base + sum(hw) + 1)
        base = (base + sum(hw[:3]) + 1) // 2 + 1
    return out


# ------------------------------------------------------------------------------------------------- comparison
def compare(got_levels, ref):
    """got_levels: dict (o, j) -> set of (row, col, sign) a tested implementation found BEFORE the budget.  Against the longdouble
    reference: mismatches on non-fragile pixels, and the fragile share of the union."""
    mism, union, fragile = [], 0, 0
    for key, r in ref["levels"].items():
        want = {(int(a), int(b)): int(s) for a, b, s in zip(r["rows"], r["cols"], r["sign"]) if s != 0}
        frag = {(int(a), int(b)) for a, b, f in zip(r["rows"], r["cols"], r["fragile"]) if f}
        got = {(int(a), int(b)): int(s) for a, b, s in got_levels.get(key, ())}
        for px in set(want) | set(got):
            union += 1
            if px in frag:
                fragile += 1
            elif want.get(px, 0) != got.get(px, 0):
                mism.append((key, px, want.get(px, 0), got.get(px, 0)))
    return mism, union, fragile


def levels_of(loc, sign):
    out = {}
    for (o, j, r, c), s in zip(np.asarray(loc).tolist(), np.asarray(sign).tolist()):
        out.setdefault((o, j), []).append((r, c, int(s)))
    return out


def pre_budget_levels(ref32):
    """the (row, col, sign) sets of a reference()'s raw decisions"""
    return {k: [(int(a), int(b), int(s)) for a, b, s in zip(r["rows"], r["cols"], r["sign"]) if s != 0] for k, r in ref32["levels"].items()}


@functools.lru_cache(None)
def measured_deviation():
    """the float32 restatement's own largest deviation from longdouble over the catalogue, on keypoints found by both: dict of
    off (dx, dy, ds), xy (X, Y), s (S)"""
    dev = dict(off=0.0, xy=0.0, s=0.0, gauss=0.0, dog=0.0)
    for name in CATALOGUE:
        a, b = catalogue_reference(name, True), catalogue_reference(name, False)
        for (Ga, Da), (Gb, Db) in zip(a["pyramid"], b["pyramid"]):
            dev["gauss"] = max(dev["gauss"], float(np.abs(Ga - Gb).max()))
            dev["dog"] = max(dev["dog"], float(np.abs(Da - Db).max()))
        ia = {tuple(l): k for k, l in enumerate(a["loc"].tolist())}
        for k, l in enumerate(b["loc"].tolist()):
            if tuple(l) in ia:
                q = ia[tuple(l)]
                dev["off"] = max(dev["off"], float(np.abs(a["off"][q] - b["off"][k]).max()))
                dev["xy"] = max(dev["xy"], float(np.abs(a["keys"][q][:2] - b["keys"][k][:2]).max()))
                dev["s"] = max(dev["s"], float(abs(a["keys"][q][2] - b["keys"][k][2])))
    return dev


def check_values(loc, off, keys, ref, factor=16.0):
    """(number compared, worst ratio to the bar) of offsets [n][3] and keys [n][>=3] against a longdouble reference()"""
    dev = measured_deviation()
    ia = {tuple(l): k for k, l in enumerate(ref["loc"].tolist())}
    n, worst = 0, 0.0
    for k, l in enumerate(np.asarray(loc).tolist()):
        q = ia.get(tuple(l))
        if q is None:
            continue
        n += 1
        if off is not None:
            worst = max(worst, float(np.abs(ref["off"][q] - np.asarray(off[k][:3], np.longdouble)).max()) / (factor * dev["off"]))
        if keys is not None:
            worst = max(worst, float(np.abs(ref["keys"][q][:2] - np.asarray(keys[k][:2], np.longdouble)).max()) / (factor * dev["xy"]))
            worst = max(worst, float(abs(ref["keys"][q][2] - np.longdouble(keys[k][2]))) / (factor * dev["s"]))
    return n, worst


if __name__ == "__main__":
    print(measured_deviation())
    for name in CATALOGUE:
        a, b = catalogue_reference(name, True), catalogue_reference(name, False)
        m, u, f = compare(pre_budget_levels(b), a)
        print(name, "geometry", a["geometry"], "level_count", a["level_count"].tolist(), "total", a["total"], "mismatch", len(m), "union", u, "fragile", f)
