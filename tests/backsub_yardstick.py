"""Yardstick, cases and checks of the back-substitution tests (tests/test_backsub_cpu.py, tests/test_gpu_backsub.py).

The yardstick is pure numpy in np.longdouble (x87 extended: eps = 2^-64 < 2e-19, asserted), never the library.  Its inputs are the
linearisation (r, Jc, Jp in Jacobi-scaled coordinates), the Jacobi scales and the camera part y_c of the step; what it checks is
the arithmetic of the back-substitution alone (oracle/ba_oracle.py: _back_substitute and the model / candidate / step-norm lines of
solve):

    u      = (Hpp + D)^-1 (g_p - sum_o E_o^T F_o y_c),   D = clip(diag Hpp, 1e-6, 1e32) / radius
    m_o    = F_o y_c + E_o u,   model decrease = sum_o m_o . (r_o - m_o / 2)
    cand P = P - u s_p (variable points),   cand q = Plus(q, -y s_c),   cand t = t - y s_c,   cand {f, k1, k2} likewise (bal9)
    squared step = sum |cand - x|^2 over the variable blocks

Every bar is a count of float64 operations times eps = 2^-53 (L = track length, n = observations of an item, T = points of an
item, |.| = 2-norm); none is tuned to a result:

  point step       |(Hpp+D) u - a| <= (32 + 18 L) eps (|Hpp+D| |u| + |g_p| + sum_o |E_o| |F_o| |y_c|), a = g_p - sum_o E_o^T F_o y_c:
                   a backward error, independent of cond(Hpp+D).  18 L: Hpp, g_p and the sum are each L-term sums of 2-3-term
                   products formed in float64; 32: the 3x3 factorisation and the two triangular products.  Asserted for every
                   kernel that factors the damped point block itself (k_backsub<true>, k9_backsub: u = C (C^T a) from the
                   Cholesky factor), low-parallax points and single-observation tracks included.
  point step,      the same with |Hpp+D| |(Hpp+D)^-1| |a| in place of |Hpp+D| |u|: the residual bound of a solve through an explicit
  inverse form     inverse, u = X a with X = fl((Hpp+D)^-1), c eps |A| |X| |a| (Higham, Accuracy and Stability of Numerical
                   Algorithms, section 14.1).  |u| <= |(Hpp+D)^-1| |a|, so it is never the tighter one.  It is the bar of the two
                   implementations that multiply by a stored inverse and cannot meet a condition-independent bound: the float64
                   restatement of the oracle (np.linalg.inv) and k_backsub<false> (stored cofactor inverse Hinv).  For those
                   the backward-error ratio is printed next to it and not asserted.
  candidate point  |cand - (P - u s_p)| <= 8 eps (|P| + |u s_p|) per component (product, sum, possibly one FMA; the scales are
                   recomputed from an unscaled linearisation and differ from the kernel's by a few eps); constant points unchanged.
  step partial     relative (64 + 3 T) eps against sum |cand - P|^2 of the kernel's own candidates (3 T non-negative terms, the
                   wave reduction adds log2(64) more additions per term).
  model partial    absolute (32 + n) eps sum_o a_o (|r_o| + a_o), a_o = |F_o| |y_c| + |E_o| |u| >= |m_o|, with the kernel's own u.
  total            sum of the partials against the model decrease formed from y_c and the yardstick's u, within the summed bars.
  cameras          q: 16 eps absolute (|q| = 1; sin, cos, 16 products); t, {f, k1, k2}: 4 eps (|x| + |y s|); constant blocks and
                   cameras without observations unchanged; the per-camera partials relative 16 eps (at most 10 terms).
"""
import numpy as np

from oracle import ba_oracle as bo
from tests import helpers as H

LD = np.longdouble
assert np.finfo(LD).eps < 2e-19, "np.longdouble carries no more than float64 here: the yardstick needs x87 extended precision"
EPS = 2.0 ** -53
HUBER_A = 5.99
LM_MIN, LM_MAX = 1e-6, 1e32


# ------------------------------------------------------------------------------------------------ cases
def ragged():
    """The construction of test_gpu_parity.py::test_ragged_tracks: 14 cameras, track lengths 1..6, shuffled."""
    arr = H.make(14, 700, 6, seed=180, mode="unordered", min_tri_angle_deg=0.5)
    rng = np.random.default_rng(9)
    n = arr["obs_cam"].shape[0]
    keep = rng.random(n) < 0.55
    first = np.zeros(n, bool); first[np.unique(arr["obs_pt"], return_index=True)[1]] = True
    keep |= first
    perm = rng.permutation(int(keep.sum()))
    for k in ("obs_cam", "obs_pt", "obs_uv"):
        arr[k] = np.ascontiguousarray(arr[k][keep][perm])
    lens = np.bincount(arr["obs_pt"], minlength=700)
    assert lens.min() == 1 and lens.max() == 6 and (lens == 1).sum() > 5
    return arr


def full_tile():
    """70 cameras; among 400 short tracks: one track of 64 observations (fills a tile), a track of 63 observations and ten tracks
    of 1.  What the packing makes of them (a track head on lane 63, a last tile that ends in dead lanes) is asserted from the
    packing itself by test_backsub_cpu.py::test_catalogue_coverage."""
    n_cams = 70
    rng = np.random.default_rng(12)
    tracks = [np.sort(rng.choice(n_cams, 3, replace=False)) for _ in range(400)]
    tracks.append(np.arange(64))
    tracks.append(np.arange(63))
    tracks.append(np.array([0]))
    tracks += [np.array([int(c)]) for c in rng.integers(0, n_cams, 9)]
    return H.make_tracks(n_cams, tracks, seed=12)


def consts_models():
    """All five camera models, every fifth point constant, cam_const 3 / 1 / 2 on three cameras, one camera without an observation,
    points pushed behind their cameras (clamp branch: J = 0)."""
    arr = H.with_models(H.make(11, 400, 4, seed=131), seed=3)
    n_pts = arr["points"].shape[0]
    arr["point_const"] = (np.arange(n_pts) % 5 == 0).astype(np.uint8)
    cc = np.zeros(11, np.uint8); cc[2] = 3; cc[5] = 1; cc[7] = 2
    arr["cam_const"] = cc
    arr["points"] = np.array(arr["points"], copy=True)
    arr["points"][3::29] += np.array([0.0, 0.0, -60.0])
    keep = arr["obs_cam"] != 9                       # camera 9 keeps its place and loses its observations
    for k in ("obs_cam", "obs_pt", "obs_uv"):
        arr[k] = np.ascontiguousarray(arr[k][keep])
    return arr


def bal9_ragged_consts():
    b = H.make_bal9(40, 2000, 6, seed=6, dropout=0.3, min_tri_angle_deg=0.5)
    b["point_const"] = (np.arange(2000) % 7 == 0).astype(np.uint8)
    cc = b["cam_const"].copy(); cc[5] &= 3; cc[9] &= 3; cc[11] |= 1; b["cam_const"] = cc
    return b


def bal9_long():
    return H.make_bal9(72, 60, 68, seed=8, mode="unordered", min_tri_angle_deg=0.5)


_SHAPES = {}


def _shape(i):
    if not _SHAPES:
        _SHAPES["all"] = H.shape_problems()
    return _SHAPES["all"][i][0]


# name -> (factory, radii, run under every variant).  Radii: 1, 1e4 and 1e16 for the H.make families, 1 and 3e3 (the radius of
# test_shape_tiles_match_oracle) for the shape catalogue, full_tile and long; bal9 at 1, 3e3 (test_gpu_bal9.py) and 1e16.
CASES = {
    "regular": (lambda: H.make(8, 300, 4), (1.0, 1e4, 1e16), True),
    "ragged": (ragged, (1.0, 1e4, 1e16), True),
    "full_tile": (full_tile, (1.0, 3e3), True),
    "long": (lambda: H.long_problem((65, 128, 129, 200), 5), (1.0, 3e3), True),
    "consts_models": (consts_models, (1.0, 1e4, 1e16), True),
    **{f"shape{i}": ((lambda i=i: _shape(i)), (1.0, 3e3), False) for i in (0, 7, 12, 16, 20)},
    "bal9_ragged_consts": (bal9_ragged_consts, (1.0, 3e3, 1e16), False),
    "bal9_long": (bal9_long, (1.0, 3e3, 1e16), False),
}
FAMILIES = {"make": ("regular", "ragged", "consts_models"), "full_tile": ("full_tile",), "long": ("long",),
            "shapes": tuple(f"shape{i}" for i in (0, 7, 12, 16, 20)), "bal9": ("bal9_ragged_consts", "bal9_long")}
_ARR = {}


def case(name):
    """The problem of a case (built once; callers must not modify it)."""
    if name not in _ARR:
        _ARR[name] = CASES[name][0]()
    return _ARR[name]


# ------------------------------------------------------------------------------------------------ work items without a GPU
def items_from_pack(arr):
    """The work items of the packing from debug_pack alone (no GPU): a tile is 64 slots; a track of more than 64 observations
    owns ceil(L / 64) consecutive tiles (one item), every other tile is an item of its own.  Returns dict(item_tiles [n][2],
    item_obs, item_points, slot_obs, stats)."""
    from xrsfm_amd import capi
    st = capi.debug_pack(H.to_product(arr))
    so = st["slot_obs"]
    pt = np.where(so >= 0, np.asarray(arr["obs_pt"])[np.maximum(so, 0)], -1).reshape(-1, 64)
    n_tiles = pt.shape[0]
    lens = np.bincount(arr["obs_pt"], minlength=arr["points"].shape[0])
    tiles, t = [], 0
    while t < n_tiles:
        ids = np.unique(pt[t][pt[t] >= 0])
        n = 1
        if len(ids) == 1 and lens[ids[0]] > 64:
            while t + n < n_tiles and (pt[t + n][pt[t + n] >= 0] == ids[0]).all() and (pt[t + n] >= 0).any():
                n += 1
            assert n == -(-int(lens[ids[0]]) // 64)
        tiles.append((t, n)); t += n
    assert len(tiles) == st["items"] and sum(n > 1 for _, n in tiles) == st["long_items"]
    item_obs = [so[64 * a:64 * (a + n)][so[64 * a:64 * (a + n)] >= 0] for a, n in tiles]
    return dict(item_tiles=np.array(tiles, np.int32), item_obs=item_obs, item_points=[np.unique(arr["obs_pt"][o]) for o in item_obs],
                slot_obs=so, slot_pt=pt, stats=st)


def coverage(arr):
    """What the packing of one problem contains (test_catalogue_coverage sums it over the cases)."""
    it = items_from_pack(arr)
    pt = it["slot_pt"]
    lens = np.bincount(arr["obs_pt"], minlength=arr["points"].shape[0])
    pc = np.asarray(arr["point_const"]) != 0
    head63 = dead = mixed = False
    for a, n in it["item_tiles"]:
        if n > 1:
            continue
        row = pt[a]
        valid = row >= 0
        head63 |= bool(valid[63] and row[63] != row[62])
        last = np.nonzero(valid)[0].max()
        dead |= bool(last < 63 and valid[:last + 1].all())
        ids = np.unique(row[valid])
        mixed |= bool(pc[ids].any() and (~pc[ids]).any())
    pr = H.to_oracle(arr)
    _, valid = bo.project(pr, want_jac=False)
    act = np.bincount(arr["obs_cam"], minlength=arr["cam_q"].shape[0]) > 0
    return dict(n_tiles=set(int(n) for _, n in it["item_tiles"]), track64=bool((lens == 64).any()), head63=head63, track1=bool((lens == 1).any()),
                dead_lanes=dead, const_in_mixed_tile=mixed, cam_const=set(int(c) & 3 for c in arr["cam_const"]), inactive_cam=bool((~act).any()),
                models=set(int(m) for m in np.asarray(arr["intr_model"])[arr["cam_intr"]]), clamped=int((~valid).sum()))


# ------------------------------------------------------------------------------------------------ inputs
def jacobi_scales(Jc, Jp, ci, pi, n_cams, n_pts):
    """1 / (1 + column norm) from an UNSCALED linearisation (test_gpu_parity.py::_lin_oracle)."""
    sc_c = 1 / (1 + np.sqrt(bo._scatter_add(n_cams, ci, np.sum(Jc * Jc, axis=1))))
    sc_p = 1 / (1 + np.sqrt(bo._scatter_add(n_pts, pi, np.sum(Jp * Jp, axis=1))))
    return sc_c, sc_p


def oracle_inputs(arr, radius):
    """CPU stand-in for the library's inputs: the oracle's scaled linearisation and the camera step of bo._solve_exact."""
    pr = H.to_oracle(arr)
    _, rt, Fc, Ep = bo.evaluate(pr, pr.cam_q, pr.cam_t, pr.points)
    ci, pi = pr.obs_cam, pr.obs_pt
    sc_c, sc_p = jacobi_scales(Fc, Ep, ci, pi, pr.cam_q.shape[0], pr.points.shape[0])
    Fs = Fc * sc_c[ci][:, None, :]; Es = Ep * sc_p[pi][:, None, :]
    lin = bo._Linearization(pr, rt, Fs, Es)
    Dc2 = np.clip(np.einsum("nii->ni", lin.Hcc), LM_MIN, LM_MAX) / radius
    Dp2 = np.clip(np.einsum("nii->ni", lin.Hpp), LM_MIN, LM_MAX) / radius
    yc, _, _ = bo._solve_exact(pr, lin, Dc2, Dp2)
    return dict(r=rt, Jc=Fs, Jp=Es, sc_c=sc_c, sc_p=sc_p, y=yc, radius=radius)


def float64_restatement(arr, inp, items):
    """The back-substitution as the oracle states it, in plain float64 (bo._back_substitute and the model / candidate / step-norm
    lines of bo.solve), in the form the library's caller-order wrapper returns."""
    pr = H.to_oracle(arr)
    ci, pi = pr.obs_cam, pr.obs_pt
    lin = bo._Linearization(pr, inp["r"], inp["Jc"], inp["Jp"])
    yc, sc_c, sc_p = inp["y"], inp["sc_c"], inp["sc_p"]
    Dp2 = np.clip(np.einsum("nii->ni", lin.Hpp), LM_MIN, LM_MAX) / inp["radius"]
    Hinv = np.linalg.inv(lin.Hpp + np.einsum("ni,ij->nij", Dp2, np.eye(3)))
    yp = bo._back_substitute(pr, lin, Hinv, yc)
    mres = -(np.einsum("nki,ni->nk", lin.Fs, yc[ci]) + np.einsum("nki,ni->nk", lin.Es, yp[pi]))
    term = -np.sum(mres * (lin.rt + 0.5 * mres), axis=1)
    cam_act = np.zeros(pr.cam_q.shape[0], bool); cam_act[ci] = True
    qvar = ((pr.cam_const & 1) == 0) & cam_act; tvar = ((pr.cam_const & 2) == 0) & cam_act
    ivar = ((pr.cam_const & bo.INTR_VARIABLE) != 0) & cam_act
    packed = bo._active_points(pr)
    pvar = (pr.point_const == 0) & packed
    dc = -yc * sc_c; dp = -yp * sc_p
    dc[~qvar, 0:3] = 0.0; dc[~tvar, 3:6] = 0.0; dp[~pvar] = 0.0
    q, t, P = pr.cam_q, pr.cam_t, pr.points
    q2 = q.copy(); q2[qvar] = bo.quat_plus(q[qvar], dc[qvar, 0:3])
    t2 = t + dc[:, 3:6]
    P2 = P + dp
    cur = pr.intr_params[pr.cam_intr][:, 0:3]
    i2 = cur.copy()
    if dc.shape[1] == 9:
        dc[~ivar, 6:9] = 0.0
        i2 = cur + dc[:, 6:9]
    step2 = ((q2 - q) ** 2).sum(1) * qvar + ((t2 - t) ** 2).sum(1) * tvar + ((i2 - cur) ** 2).sum(1) * ivar
    xn2 = (q ** 2).sum(1) * qvar + (t ** 2).sum(1) * tvar + (cur ** 2).sum(1) * ivar
    return dict(point_step=yp, cand_points=P2, packed=packed, cand_cam_q=q2, cand_cam_t=t2, cand_intr=i2, campart=np.stack([step2, xn2]),
                part_model=np.array([term[o].sum() for o in items["item_obs"]]),
                part_step2=np.array([((P2 - P)[p] ** 2).sum() for p in items["item_points"]]),
                item_obs=items["item_obs"], item_points=items["item_points"])


# ------------------------------------------------------------------------------------------------ the yardstick
def _norm2(M):
    return np.linalg.norm(np.asarray(M, np.float64), 2, axis=(-2, -1))


def _vnorm(v):
    return np.sqrt(np.sum(np.asarray(v, LD) ** 2, axis=-1))


def _solve3(A, b):
    """x = A^-1 b for stacked symmetric positive definite 3x3 A in np.longdouble: LDL^T and two steps of refinement."""
    def once(rhs):
        d0 = A[:, 0, 0]; l10 = A[:, 1, 0] / d0; l20 = A[:, 2, 0] / d0
        d1 = A[:, 1, 1] - l10 * l10 * d0
        l21 = (A[:, 2, 1] - l20 * l10 * d0) / d1
        d2 = A[:, 2, 2] - l20 * l20 * d0 - l21 * l21 * d1
        z0 = rhs[:, 0]; z1 = rhs[:, 1] - l10 * z0; z2 = rhs[:, 2] - l20 * z0 - l21 * z1
        x2 = z2 / d2; x1 = z1 / d1 - l21 * x2; x0 = z0 / d0 - l10 * x1 - l20 * x2
        return np.stack([x0, x1, x2], axis=1)
    x = once(b)
    for _ in range(2):
        x = x + once(b - np.einsum("nij,nj->ni", A, x))
    return x


def _ratio(err, bar):
    """err / bar elementwise; where the bar is zero the value must be exact (0 -> 0, anything else -> inf)."""
    err = np.asarray(err, LD); bar = np.asarray(bar, LD)
    out = np.where(err == 0, LD(0), LD(np.inf))
    np.divide(err, bar, out=out, where=bar > 0)
    return out.astype(np.float64)


def _exact(a, b):
    """0 where a == b (same value, no NaN), inf elsewhere."""
    return np.where(np.asarray(a) == np.asarray(b), 0.0, np.inf)


def check_all(arr, inp, got):
    """Every check of the module docstring.  inp: r [No][2], Jc [No][2][W], Jp [No][2][3], sc_c [Nc][W], sc_p [Np][3], y [Nc][W],
    radius.  got: the caller-order outputs (capi.Context.debug_backsub_caller_order, or float64_restatement).  Returns
    {check: (ratio to its bar, per point / item / camera)} and the scalar facts "model_change" (yardstick) and "model_sum"."""
    ci = np.asarray(arr["obs_cam"], np.int64); pi = np.asarray(arr["obs_pt"], np.int64)
    Nc, Np = arr["cam_q"].shape[0], arr["points"].shape[0]
    W = inp["Jc"].shape[2]
    E = inp["Jp"].astype(LD); F = inp["Jc"].astype(LD); r = inp["r"].astype(LD); y = inp["y"].astype(LD)
    eye = np.eye(3, dtype=LD)
    v = np.einsum("nki,ni->nk", F, y[ci])
    Hpp = np.zeros((Np, 3, 3), LD); np.add.at(Hpp, pi, np.einsum("nki,nkj->nij", E, E))
    g = np.zeros((Np, 3), LD); np.add.at(g, pi, np.einsum("nki,nk->ni", E, r))
    wty = np.zeros((Np, 3), LD); np.add.at(wty, pi, np.einsum("nki,nk->ni", E, v))
    D = np.clip(np.einsum("nii->ni", Hpp), LD(LM_MIN), LD(LM_MAX)) / LD(inp["radius"])
    Hd = Hpp + D[:, :, None] * eye
    a = g - wty
    u_ref = _solve3(Hd, a)
    out = {}

    # point step: backward error with the kernel's u
    u = got["point_step"].astype(LD)
    L = np.bincount(pi, minlength=Np)
    nE, nF, ny, nu = _norm2(inp["Jp"]), _norm2(inp["Jc"]), _vnorm(y), _vnorm(u)
    sEF = np.zeros(Np, LD); np.add.at(sEF, pi, nE * nF * ny[ci])
    res = _vnorm(np.einsum("nij,nj->ni", Hd, u) - a)
    nHinv = _norm2(np.stack([_solve3(Hd, np.broadcast_to(eye[k], (Np, 3))) for k in range(3)], axis=2))
    out["point_step"] = _ratio(res, (32 + 18 * L) * EPS * (_norm2(Hd) * nu + _vnorm(g) + sEF))
    out["point_step_inverse"] = _ratio(res, (32 + 18 * L) * EPS * (_norm2(Hd) * nHinv * _vnorm(a) + _vnorm(g) + sEF))
    pconst = (np.asarray(arr["point_const"]) != 0) | ~got["packed"]
    out["const_point_step"] = _exact(got["point_step"][pconst], 0.0).max(axis=1, initial=0.0)

    # candidate points
    P = np.asarray(arr["points"], np.float64)
    us = u * inp["sc_p"].astype(LD)
    rat = _ratio(np.abs(got["cand_points"].astype(LD) - (P.astype(LD) - us)), 8 * EPS * (np.abs(P) + np.abs(us)))
    out["cand_point"] = rat[~pconst].max(axis=1, initial=0.0)
    out["const_cand_point"] = _exact(got["cand_points"][pconst], P[pconst]).max(axis=1, initial=0.0)

    # per item: squared point step and model decrease
    dP2 = np.sum((got["cand_points"].astype(LD) - P.astype(LD)) ** 2, axis=1)
    m = v + np.einsum("nki,ni->nk", E, u[pi])
    term = np.sum(m * (r - m / 2), axis=1)
    ao = nF * ny[ci] + nE * nu[pi]
    tbar = ao * (_vnorm(r) + ao)
    n_it = len(got["item_obs"])
    s_ref = np.zeros(n_it, LD); s_T = np.zeros(n_it); m_ref = np.zeros(n_it, LD); m_bar = np.zeros(n_it, LD)
    for i in range(n_it):
        o, p = got["item_obs"][i], got["item_points"][i]
        s_ref[i] = dP2[p].sum(); s_T[i] = len(p)
        m_ref[i] = term[o].sum(); m_bar[i] = (32 + len(o)) * EPS * tbar[o].sum()
    out["part_step2"] = _ratio(np.abs(got["part_step2"].astype(LD) - s_ref), (64 + 3 * s_T) * EPS * s_ref)
    out["part_model"] = _ratio(np.abs(got["part_model"].astype(LD) - m_ref), m_bar)

    # total model decrease against the yardstick's own u
    m_r = v + np.einsum("nki,ni->nk", E, u_ref[pi])
    model_change = np.sum(m_r * (r - m_r / 2))
    model_sum = np.sum(got["part_model"].astype(LD))
    out["model_total"] = _ratio(np.abs(model_sum - model_change)[None], m_bar.sum()[None])
    out["model_change"] = float(model_change); out["model_sum"] = float(model_sum)

    # cameras
    cc = np.asarray(arr["cam_const"])
    act = np.bincount(ci, minlength=Nc) > 0
    qvar = act & ((cc & 1) == 0); tvar = act & ((cc & 2) == 0); ivar = act & ((cc & 4) != 0) & (W == 9)
    q = np.asarray(arr["cam_q"], np.float64); t = np.asarray(arr["cam_t"], np.float64)
    cur = np.asarray(arr["intr_params"], np.float64)[arr["cam_intr"]][:, 0:3]
    ys = y * inp["sc_c"].astype(LD)
    q_ref = bo.quat_plus(q.astype(LD), -ys[:, 0:3])
    assert q_ref.dtype == LD
    cq, ct, cin = got["cand_cam_q"], got["cand_cam_t"], got["cand_intr"]
    out["cand_q"] = (np.abs(cq.astype(LD) - q_ref).max(axis=1) / (16 * EPS)).astype(np.float64)[qvar]
    out["const_q"] = _exact(cq[~qvar], q[~qvar]).max(axis=1, initial=0.0)
    out["cand_t"] = _ratio(np.abs(ct.astype(LD) - (t.astype(LD) - ys[:, 3:6])), 4 * EPS * (np.abs(t) + np.abs(ys[:, 3:6])))[tvar].max(axis=1, initial=0.0)
    out["const_t"] = _exact(ct[~tvar], t[~tvar]).max(axis=1, initial=0.0)
    if W == 9:
        out["cand_intr"] = _ratio(np.abs(cin.astype(LD) - (cur.astype(LD) - ys[:, 6:9])),
                                  4 * EPS * (np.abs(cur) + np.abs(ys[:, 6:9])))[ivar].max(axis=1, initial=0.0)
    out["const_intr"] = _exact(cin[~ivar], cur[~ivar]).max(axis=1, initial=0.0)
    sq = lambda x: np.sum(x.astype(LD) ** 2, axis=1)
    step2 = sq(cq.astype(LD) - q.astype(LD)) * qvar + sq(ct.astype(LD) - t.astype(LD)) * tvar + sq(cin.astype(LD) - cur.astype(LD)) * ivar
    xn2 = sq(q) * qvar + sq(t) * tvar + sq(cur) * ivar
    out["campart_step2"] = _ratio(np.abs(got["campart"][0].astype(LD) - step2), 16 * EPS * step2)
    out["campart_xnorm2"] = _ratio(np.abs(got["campart"][1].astype(LD) - xn2), 16 * EPS * xn2)
    return out


def worst(checks):
    """{check: (largest ratio, its index)} of check_all's result (the scalar facts dropped)."""
    return {k: ((float(np.max(v)), int(np.argmax(v))) if np.size(v) else (0.0, -1)) for k, v in checks.items() if isinstance(v, np.ndarray)}


def assert_inside(checks, what, explicit_inverse=False):
    """Every ratio <= 1, the total model decrease positive on both sides; the message names the worst point / item / camera.
    explicit_inverse: the implementation multiplies by a stored inverse of the damped point block (the float64 restatement,
    k_backsub<false>): its point step answers to the inverse-form bar only."""
    w = worst(checks)
    bad = {k: x for k, x in w.items() if not x[0] <= 1.0 and not (explicit_inverse and k == "point_step")}
    assert not bad, f"{what}: outside the bar (ratio, index): {bad}"
    assert checks["model_change"] > 0 and checks["model_sum"] > 0, (what, checks["model_change"], checks["model_sum"])
    return w
