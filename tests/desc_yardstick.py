"""The yardstick of xrsfm_ba_extract_features: the rule of xrsfm_amd/csrc/ba_sift_desc_rule.h in pure numpy, once in
np.longdouble and once in float32, on the catalogue of tests/sift_yardstick.py, and the bars.  Every stage is checked on the INPUTS
THE TESTED IMPLEMENTATION ITSELF PRODUCED (its Gaussian levels, its gradient planes, its keys, its sums), so that a discrete
decision upstream does not turn a comparison downstream into noise.

Bars (eps = 2^-24, one rounding of a float32 operation; a library function counts with its published bound):
  A  grd = 0.5 sqrt(dx dx + dy dy): dx 1, dx dx 3, the sum 4, the root 4 / 2 + 2 (a root within 1 ulp): 4 eps grd.  rot = atan2(dy,
     dx): the roundings of dx and dy turn the angle by at most eps (|dx| + |dy|) / (2 grd) (2 grd is the length of the gradient),
     which is at most sqrt(2) eps, plus ATAN2_ULP = 2 ulp of |rot| for the function (the larger of the figures published for the
     device libraries); compared modulo 2 pi.  rot is exactly 0 where grd is 0.
  B  a sample's bin is one float32 multiply and a floor of the implementation's own rot: exact.  Membership sq_dist < win^2 + 0.5:
     sq_dist carries 4 eps, the threshold 4 eps: a sample within 4 eps (sq_dist + threshold) of the border makes its keypoint
     FRAGILE.  The arg-max is fragile when another bin lies within twice the bar of a smoothed vote of the maximum.  On the other
     keypoints the arg-max is equal and w lies within 16 times the float32 restatement's own measured deviation; the bar of a vote
     is 16 times its measured deviation relative to the largest vote.
  C  theta, its bin and the dropped theta == 8.0f are exact float32 functions of (key.w, rot).  The 128 sums lie within 16 times
     the restatement's measured deviation, relative to the keypoint's largest sum.  (The box of a cell bounds the support of its
     weight, which falls to 0 at the support's border: no fragility.)
  D  a norm is a sum of 128 non-negative products: 129 eps, halved by the root, plus 2 eps for rsqrt within 1 ulp and 1 for the
     product: 68 eps per normalisation; the second normalisation acts on values that carry the first: unit within 3 * 68 eps
     relative (the clamp is continuous).  desc_float = sqrt(v / sum |v|): the sum 128, the quotient 1, halved, the root 1: 66 eps
     relative.  A byte is rounding-fragile when 512 v in longdouble lies within 512 * 66 eps v of a half-integer; every other
     byte is equal, a fragile one may differ by 1; at most 5 % of the bytes may be fragile.

Measured on the catalogue (float32 restatement against longdouble, this file's __main__; also in profiles/feature_extract.md):
smoothed votes 3.0e-7 of the largest vote, w 8.2e-7 rad, descriptor sums 4.1e-6 of the keypoint's largest sum; 1224 keypoints, none
fragile, no arg-max mismatch; 0.04 % of the bytes rounding-fragile, none wrong.  The kernels on an MI355X: grd and rot within 0.48 and
0.70 of their bars, w within 0.06 and the sums within 0.07 of the 16x bars, unit and desc_float within 0.03 and 0.06 of theirs.
"""
import functools

import numpy as np

from tests import sift_yardstick as Y

F = np.float32
LD = np.longdouble
EPS = Y.EPS
ATAN2_ULP = 2.0
NAMES = ("a44x40", "b50x33", "c64x48", "c64x48_o0", "d64x48", "e300x260")
TEN = F(5.7295779513082320876798154814105)
RAD = F(1.0 / 5.7295779513082320876798154814105)
THIRD = F(1.0 / 3.0)
RPI = F(4.0 / 3.14159265358979323846)
PI = 3.14159265358979323846
UNIT_OPS, FLOAT_OPS = 3 * 68.0, 66.0


# ------------------------------------------------------------------------------------------------- A: gradient
def gradient(G, dt=LD):
    """G [h][w] float32 -> (grd, rot) [h][w][2] in dt; the border is (0, 0)"""
    g = np.asarray(G, F).astype(dt)
    h, w = g.shape
    dx, dy = np.zeros((h, w), dt), np.zeros((h, w), dt)
    dx[1:-1, 1:-1] = g[1:-1, 2:] - g[1:-1, :-2]
    dy[1:-1, 1:-1] = g[2:, 1:-1] - g[:-2, 1:-1]
    grd = dt(0.5) * np.sqrt(dx * dx + dy * dy)
    with np.errstate(all="ignore"):
        rot = np.where(grd == 0, dt(0), np.arctan2(dy, dx))
    return np.stack([grd, rot], -1), np.abs(dx), np.abs(dy)


def check_gradient(G3, got):
    """G3 [3][h][w]: G[1..3] of an octave; got [3][h][w][2].  -> worst ratios (grd, rot) to their bars; asserts rot == 0 at grd == 0"""
    worst = [0.0, 0.0]
    for j in range(3):
        ref, adx, ady = gradient(G3[j])
        g = np.asarray(got[j], F)
        assert np.all(g[[0, -1], :, :] == 0) and np.all(g[:, [0, -1], :] == 0), "border"
        assert np.all(g[..., 1][g[..., 0] == 0] == 0), "rot must be 0 where grd is 0"
        zero = ref[..., 0] == 0
        assert np.all(g[..., 0][zero] == 0)
        bar_g = 4 * EPS * ref[..., 0]
        worst[0] = max(worst[0], float((np.abs(g[..., 0].astype(LD) - ref[..., 0])[~zero] / bar_g[~zero]).max()))
        d = np.abs((g[..., 1].astype(LD) - ref[..., 1] + LD(PI)) % LD(2 * PI) - LD(PI))
        with np.errstate(all="ignore"):
            bar_r = EPS * (adx + ady) / (2 * ref[..., 0]) + ATAN2_ULP * np.spacing(np.maximum(np.abs(ref[..., 1]).astype(F), F(2.0 ** -20))).astype(LD)
        worst[1] = max(worst[1], float((d[~zero] / bar_r[~zero]).max()))
    return tuple(worst)


# ------------------------------------------------------------------------------------------------- keys
def octave_keys(loc, off, first_octave):
    """float32 (x, y, sigma) of the octave-space key from loc [n][4] and offsets [n][>=3] = (dx, dy, ds)"""
    P = Y.params(first_octave)
    loc, off = np.asarray(loc), np.asarray(off, F)
    x = (loc[:, 3].astype(F) + F(0.5)) + off[:, 0]
    y = (loc[:, 2].astype(F) + F(0.5)) + off[:, 1]
    sig = np.array([P["key_sigma"][j] for j in loc[:, 1]], F) if len(loc) else np.zeros(0, F)
    s = (sig * np.power(np.full(len(loc), P["step"], F), off[:, 2])).astype(F)
    return np.stack([x, y, s], -1).astype(F)


def mirror(w):
    """DownloadKeypoints: (float) fmod(2 pi - w, 2 pi) in double on the float w"""
    return np.fmod(2.0 * PI - np.asarray(w, F).astype(np.float64), 2.0 * PI).astype(F)


# ------------------------------------------------------------------------------------------------- B: orientation
def smooth(vote, dt):
    v = vote.astype(dt)
    for _ in range(6):
        v = dt(THIRD) * ((np.roll(v, 1) + v) + np.roll(v, -1))
    return v


def peak(v, dt):
    """-> (index, w, margin of the arg-max relative to the maximum, denominator)"""
    i = int(np.argmax(v))
    pre, nxt, mx = v[(i - 1) % 36], v[(i + 1) % 36], v[i]
    den = mx + mx - nxt - pre
    off = dt(0) if den == 0 else dt(0.5) * ((nxt - pre) / den)
    w = dt(RAD) * (dt(i) + dt(0.5) + off)
    others = np.delete(v, i)
    margin = float((mx - others.max()) / mx) if mx > 0 else 0.0
    return i, w, margin, den


def orientation(plane, key, dt=LD):
    """plane [h][w][2] float32 (grd, rot), key (x, y, sigma) float32 -> dict(vote [36] smoothed, index, w, margin, near: a sample
    within its bar of the circle's border, n: samples inside)"""
    h, w = plane.shape[:2]
    kx, ky, kz = (dt(F(v)) for v in key[:3])
    win = np.abs(kz) * dt(F(3.0))
    gs = kz * dt(F(1.5))
    if dt is F:
        thr = F(np.float64(win * win) + 0.5)
    else:
        thr = win * win + dt(0.5)
    factor = dt(-0.5) / (gs * gs)
    fl = lambda v: dt(np.floor(v))
    pad = 0 if dt is F else 1
    xmin, ymin = max(dt(1.5), fl(kx - win) + dt(0.5) - pad), max(dt(1.5), fl(ky - win) + dt(0.5) - pad)
    xmax, ymax = min(dt(w - 1.5), fl(kx + win) + dt(0.5) + pad), min(dt(h - 1.5), fl(ky + win) + dt(0.5) + pad)
    xs = np.arange(int(xmin), int(xmax) + 1); ys = np.arange(int(ymin), int(ymax) + 1)
    dx = (xs.astype(dt) + dt(0.5)) - kx; dy = (ys.astype(dt) + dt(0.5)) - ky
    sq = (dx * dx)[None, :] + (dy * dy)[:, None]
    inside = ~(sq >= thr)
    near = bool((np.abs(sq - thr) < 4 * EPS * (sq + thr)).any())
    sub = plane[ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1] if len(xs) and len(ys) else np.zeros((0, 0, 2), F)
    grd, rot = sub[..., 0][inside], sub[..., 1][inside]
    b = np.floor(rot.astype(F) * TEN).astype(np.int64)          # exact float32: one multiply, one floor
    b = np.where(b < 0, b + 36, b)
    wt = grd.astype(dt) * np.exp(sq[inside] * factor)
    vote = np.zeros(36, dt)
    np.add.at(vote, b, wt.astype(dt))                              # row by row, column by column: the reference's order
    v = smooth(vote, dt)
    i, ww, margin, den = peak(v, dt)
    return dict(vote=v, index=i, w=ww, margin=margin, near=near, n=int(inside.sum()), zero_den=bool(den == 0), clamped=(xmin == 1.5, ymin == 1.5, xmax == w - 1.5, ymax == h - 1.5))


# ------------------------------------------------------------------------------------------------- C: descriptor
def theta_of(kw, rot):
    """exact float32: (anglef, theta [..], bin [..], dropped [..])"""
    kw = F(kw)
    anglef = F(np.float64(kw) - 2.0 * PI) if np.float64(kw) > PI else kw
    th = ((anglef - np.asarray(rot, F)) * RPI).astype(F)
    th = np.where(th < 0, (th + F(8)).astype(F), th).astype(F)
    fo = np.floor(th)
    return anglef, th, fo.astype(np.int64), ~(th < F(8))


def descriptor(plane, key, dt=LD):
    """plane [h][w][2] float32, key (x, y, sigma, w) float32 -> dict(raw [128], dropped, zero_theta, clamped)"""
    h, w = plane.shape[:2]
    kx, ky, kz, kw = (dt(F(v)) for v in key[:4])
    spt = np.abs(kz * dt(F(3.0)))
    s, c = np.sin(kw), np.cos(kw)
    cspt, sspt, crspt, srspt = c * spt, s * spt, c / spt, s / spt
    bsz = np.abs(cspt) + np.abs(sspt)
    cell = np.arange(16)
    offx, offy = (cell & 3).astype(dt) - dt(1.5), (cell >> 2).astype(dt) - dt(1.5)
    ptx = cspt * offx - sspt * offy + kx
    pty = cspt * offy + sspt * offx + ky
    pad = 0 if dt is F else 1
    xmin = np.maximum(dt(1.5), np.floor(ptx - bsz) + dt(0.5) - pad); ymin = np.maximum(dt(1.5), np.floor(pty - bsz) + dt(0.5) - pad)
    xmax = np.minimum(dt(w - 1.5), np.floor(ptx + bsz) + dt(0.5) + pad); ymax = np.minimum(dt(h - 1.5), np.floor(pty + bsz) + dt(0.5) + pad)
    nx_ = int(max(0, (xmax - xmin).max() + 1)); ny_ = int(max(0, (ymax - ymin).max() + 1))
    X = xmin[:, None, None] + np.arange(nx_).astype(dt)[None, None, :] + np.zeros((1, ny_, 1), dt)
    Yy = ymin[:, None, None] + np.arange(ny_).astype(dt)[None, :, None] + np.zeros((1, 1, nx_), dt)
    ok = (X <= xmax[:, None, None]) & (Yy <= ymax[:, None, None])
    dx, dy = X - ptx[:, None, None], Yy - pty[:, None, None]
    nx = crspt * dx + srspt * dy
    ny = crspt * dy - srspt * dx
    ok &= (np.abs(nx) < 1) & (np.abs(ny) < 1)
    ci = np.nonzero(ok)                                            # ordered by cell, row, column: the reference's order within a cell
    xi, yi = X[ok].astype(np.int64), Yy[ok].astype(np.int64)
    grd, rot = plane[yi, xi, 0], plane[yi, xi, 1]
    nx, ny = nx[ok], ny[ok]
    dnx, dny = nx + offx[ci[0]], ny + offy[ci[0]]
    ww = np.exp(dt(-0.125) * (dnx * dnx + dny * dny))
    weight = ww * (dt(1) - np.abs(nx)) * (dt(1) - np.abs(ny)) * grd.astype(dt)
    _, th, fo, dropped = theta_of(key[3], rot)
    if dt is F:
        w1, w2 = ((fo.astype(F) + F(1) - th) * weight).astype(F), ((th - fo.astype(F)) * weight).astype(F)
    else:
        w1, w2 = (fo.astype(dt) + dt(1) - th.astype(dt)) * weight, (th.astype(dt) - fo.astype(dt)) * weight
    des = np.zeros(16 * 9, dt)
    keep = ~dropped
    np.add.at(des, (ci[0] * 9 + fo)[keep], w1[keep])
    np.add.at(des, (ci[0] * 9 + fo + 1)[keep], w2[keep])
    des = des.reshape(16, 9)
    des[:, 0] = des[:, 0] + des[:, 8]
    return dict(raw=des[:, :8].reshape(128).copy(), dropped=int(dropped.sum()), zero_theta=int((th == 0).sum()), samples=int(len(th)),
                clamped=(bool((xmin == 1.5).any()), bool((ymin == 1.5).any()), bool((xmax == w - 1.5).any()), bool((ymax == h - 1.5).any())))


# ------------------------------------------------------------------------------------------------- D: normalisation and bytes
def _sum4(v, dt):
    """the sum of a [128] vector four by four, then over the 32 groups in order"""
    q = v.reshape(32, 4)
    part = ((q[:, 0] + q[:, 1]) + q[:, 2]) + q[:, 3]
    s = dt(0)
    for p in part:
        s = dt(s + p)
    return s


def normalize(raw, dt=LD):
    r = np.asarray(raw, F).astype(dt)
    n1 = dt(1) / np.sqrt(_sum4(r * r, dt))
    u = np.minimum(dt(0.2) if dt is not F else F(0.2), r * n1)
    n2 = dt(1) / np.sqrt(_sum4(u * u, dt))
    return (u * n2).astype(dt)


def l1_root(unit, dt=LD):
    u = np.asarray(unit, F).astype(dt)
    return np.sqrt(u / _sum4(np.abs(u), dt)).astype(dt)


def to_bytes(v):
    """std::round (half away from zero) of 512 v in float32, clamped to 0 .. 255"""
    x = (F(512) * np.asarray(v, F)).astype(F)
    r = np.where(x >= 0, np.floor(x + F(0.5)), np.ceil(x - F(0.5)))
    half = (x - np.floor(x)) == F(0.5)
    r = np.where(half & (x >= 0), np.floor(x) + 1, r)
    return np.clip(r, 0, 255).astype(np.uint8)


def check_normalisation(raw, unit, desc_float, desc):
    """[n][128] each; unit from raw, desc_float and desc from unit.  -> dict of worst ratios and the fragile share of the bytes"""
    worst_u = worst_f = 0.0
    fragile = wrong = total = clamp_binds = full = 0
    for k in range(len(raw)):
        ur = normalize(raw[k])
        clamp_binds += int((np.asarray(raw[k], F).astype(LD) / np.sqrt(_sum4(np.asarray(raw[k], F).astype(LD) ** 2, LD)) > 0.2).any())
        worst_u = max(worst_u, float((np.abs(np.asarray(unit[k], F).astype(LD) - ur) / (UNIT_OPS * EPS * np.maximum(ur, LD(1e-30)))).max()))
        if desc is None:
            continue
        fr = l1_root(unit[k])
        if desc_float is not None:
            worst_f = max(worst_f, float((np.abs(np.asarray(desc_float[k], F).astype(LD) - fr) / (FLOAT_OPS * EPS * np.maximum(fr, LD(1e-30)))).max()))
        x = LD(512) * fr
        frag = np.abs((x - np.floor(x)) - LD(0.5)) <= 512 * FLOAT_OPS * EPS * fr
        want = np.clip(np.floor(x + LD(0.5)), 0, 255).astype(np.int64)
        d = np.abs(np.asarray(desc[k]).astype(np.int64) - want)
        wrong += int(((d > 0) & ~frag).sum() + (d > 1).sum())
        fragile += int(frag.sum()); total += 128
        full += int((np.asarray(desc[k]) == 255).any())
    return dict(unit=worst_u, floats=worst_f, fragile=fragile, wrong=wrong, total=total, clamp_binds=clamp_binds, byte_255=full)


# ------------------------------------------------------------------------------------------------- the catalogue in float32
def planes_of(G, dt=F):
    """G [6][h][w] of an octave -> [3][h][w][2] (grd, rot) of G[1..3] as float32 arrays computed in dt"""
    return np.stack([gradient(G[j + 1], dt)[0].astype(F) for j in range(3)])


@functools.lru_cache(None)
def catalogue_inputs(name):
    """the float32 restatement's own planes and keys of a catalogue image: dict(planes [octave] -> [3][h][w][2], loc, okeys [n][3])"""
    ref = Y.catalogue_reference(name, False)
    fo = Y.CATALOGUE[name][4]
    planes = [planes_of(G) for G, _ in ref["pyramid"]]
    return dict(planes=planes, loc=ref["loc"], okeys=octave_keys(ref["loc"], ref["off"].astype(F), fo), first_octave=fo)


@functools.lru_cache(None)
def catalogue_stages(name, long):
    """orientation and descriptor of every keypoint of a catalogue image from catalogue_inputs(), in one precision; the descriptor
    uses the FLOAT32 orientation in both, as the stages are checked each on the same inputs"""
    inp = catalogue_inputs(name)
    dt = LD if long else F
    out = []
    for (o, j, _, _), key in zip(inp["loc"].tolist(), inp["okeys"]):
        pl = inp["planes"][o][j]
        ori = orientation(pl, key, dt)
        w32 = F(ori["w"]) if not long else F(catalogue_stages(name, False)[len(out)]["ori"]["w"])
        out.append(dict(ori=ori, desc=descriptor(pl, np.array([key[0], key[1], key[2], w32], F), dt), w32=w32))
    return out


def orient_fragile(ori_ld, vote_bar):
    return ori_ld["near"] or ori_ld["margin"] < 2 * vote_bar or ori_ld["zero_den"]


@functools.lru_cache(None)
def measured_deviation():
    """the float32 restatement's largest deviation from longdouble over the catalogue: vote (relative to the largest vote), w on
    keypoints that are not fragile, raw (relative to the keypoint's largest sum); and the counts"""
    vote = 0.0
    for name in NAMES:
        for a, b in zip(catalogue_stages(name, True), catalogue_stages(name, False)):
            if not a["ori"]["near"]:
                vote = max(vote, float(np.abs(a["ori"]["vote"] - b["ori"]["vote"].astype(LD)).max() / a["ori"]["vote"].max()))
    dev = dict(vote=vote, w=0.0, raw=0.0, keys=0, fragile=0, index_mismatch=0)
    for name in NAMES:
        for a, b in zip(catalogue_stages(name, True), catalogue_stages(name, False)):
            dev["keys"] += 1
            dev["raw"] = max(dev["raw"], float(np.abs(a["desc"]["raw"] - b["desc"]["raw"].astype(LD)).max() / a["desc"]["raw"].max()))
            if orient_fragile(a["ori"], 16 * vote):
                dev["fragile"] += 1
                continue
            dev["index_mismatch"] += int(a["ori"]["index"] != b["ori"]["index"])
            dev["w"] = max(dev["w"], float(abs(a["ori"]["w"] - LD(b["ori"]["w"]))))
    return dev


# ------------------------------------------------------------------------------------------------- checking an implementation
def check_orientation(planes, loc, okeys, factor=16.0):
    """planes [octave] -> [3][h][w][2], loc [n][4], okeys [n][4] of an implementation.  -> dict(fragile, compared, worst ratio of w to
    its bar, mismatched arg-max: list)"""
    dev = measured_deviation()
    out = dict(fragile=0, compared=0, worst=0.0, mismatch=[])
    for k, ((o, j, _, _), key) in enumerate(zip(np.asarray(loc).tolist(), okeys)):
        ref = orientation(planes[o][j], key[:3])
        if orient_fragile(ref, factor * dev["vote"]):
            out["fragile"] += 1
            continue
        out["compared"] += 1
        got_index = int(np.floor(float(key[3]) * float(TEN)))
        d = float(abs(ref["w"] - LD(F(key[3]))))
        if d > factor * dev["w"] and got_index != ref["index"]:
            out["mismatch"].append((k, ref["index"], got_index))
        out["worst"] = max(out["worst"], d / (factor * dev["w"]))
    return out


def check_descriptor(planes, loc, okeys, raw, factor=16.0):
    """raw [n][128] from the implementation's planes and its okeys (its w included) -> worst ratio to the bar, dropped samples"""
    dev = measured_deviation()
    worst, dropped = 0.0, 0
    for (o, j, _, _), key, r in zip(np.asarray(loc).tolist(), okeys, raw):
        ref = descriptor(planes[o][j], key)
        dropped += ref["dropped"]
        worst = max(worst, float(np.abs(ref["raw"] - np.asarray(r, F).astype(LD)).max() / ref["raw"].max()) / (factor * dev["raw"]))
    return worst, dropped


if __name__ == "__main__":
    import time
    t0 = time.time()
    print(measured_deviation(), "seconds", round(time.time() - t0, 1))
    for name in NAMES:
        st = catalogue_stages(name, True)
        raw = np.stack([s["desc"]["raw"] for s in catalogue_stages(name, False)]).astype(F)
        unit = np.stack([normalize(r, F) for r in raw]).astype(F)
        fl = np.stack([l1_root(u, F) for u in unit]).astype(F)
        print(name, "keys", len(st), "dropped", sum(s["desc"]["dropped"] for s in st), "theta 0", sum(s["desc"]["zero_theta"] for s in st),
              "clamped", np.array([s["desc"]["clamped"] for s in st]).sum(0).tolist(), "octaves", sorted(set(catalogue_inputs(name)["loc"][:, 0].tolist())),
              check_normalisation(raw, unit, fl, to_bytes(fl)))
