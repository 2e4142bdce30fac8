"""Yardstick, cases and checks of the reduced-system assembly tests (tests/test_schur_cpu.py, tests/test_gpu_schur.py).

The yardstick is pure numpy in np.longdouble (x87 extended: eps = 2^-64 < 2e-19, asserted), never the library.  Its inputs are the
kernel's own scaled linearisation, float64 values treated as exact: r [No][2], Jc = F [No][2][cw] and Jp = E [No][2][3]
(debug_linearize on the 6-wide path, debug_wide on bal9), plus the radius.  What it checks is the arithmetic of the assembly alone
(ba_chol.h: k_schur_pairs / pairs_V / pairs_diag, the segmented sums, k_tile_fill; ba_wide.h: the k9 twins; ba_kernels.h: k_point_prep,
k_schur_prep, k_schur_matvec, k_cam_factor); tests/test_gpu_lin.py holds the linearisation to its own bars.  With cw = 6 or 9:

    per observation   W_o = F_o^T E_o
    per track j       Hpp_j = sum E^T E,  g_pj = sum E^T r,  A_j = Hpp_j + diag(clip(diag Hpp_j, 1e-6, 1e32) / radius),  X_j = A_j^-1
    per camera c      Hcc_c = sum F^T F (the full block),  g_c = sum F^T r
    diagonal block    S_cc = Hcc_c + diag(clip(diag Hcc_c, 1e-6, 1e32) / radius) - sum_{o of c} W_o X W_o^T
    off-diagonal      S_ab = - sum_{tracks seen by a and b} W_a X_j W_b^T
    right-hand side   b_c = g_c - sum_{o of c} W_o X g_p
    PCG product       y = S x

The values are formed from the long-double Cholesky factor A = L L^T by substitution, V = W L^-T and L^-1 g_p, so that
W X W^T = V V^T and W X g_p = V (L^-1 g_p): the rows of W lie in the range of Hpp, and a product with the entries of X would cancel
cond(A) of the yardstick's own digits.  What is left of its own error is the factorisation's, 2^-11 of the float64 bar below.

Bars.  One per entry of each block and per component of b and y, every one a count of float64 operations times eps = 2^-53 (first
order; the (value, bar) class V of tests/lin_yardstick.py carries Hpp, g_p, diag Hcc and g_c).  None is normalised by an array-wide
maximum, none is tuned to a result.  |.| is the entrywise absolute value, Wabs_o = |F_o|^T |E_o| >= |W_o|.

  sum over L terms     (L + log2(64) + 2) eps sum |term| + the terms' own bars: it holds for any summation order (MFMA accumulation,
                       strided and segmented wave reductions, LDS pre-reduction of up to 4 tiles, per-pair records summed per camera,
                       the two-level segsum).  L = observations of the camera for Hcc, g_c and the Schur term of the diagonal block
                       (the kernels sum F^T F - V V^T per observation: the terms are charged |F|^T |F| + |W X W^T|, which bounds the
                       sum of the differences and the difference of the sums alike); L = tracks shared by the pair for an off-diagonal
                       block; L = track length for Hpp and g_p.
  Hpp, g_p, Hcc, g_c   running error of E^T E, E^T r, F^T F, F^T r per observation (two products and a sum) under the sum bar.
  damping              d = clip(h) / radius: bar(h) / radius where the clip passes h through, + 3 eps |d| (1 / radius, the product,
                       or the division of k_point_prep / k_tile_fill), + eps (|h| + |d|) for the sum (the kernels form
                       fma(clip, 1 / radius, h), or h + clip / radius).  Delta A_j = bar(Hpp_j) + these on the diagonal.
  fast_rsqrt, fast_rcp RSQ = 3 eps each (ba_math.h: hardware estimate, two Newton steps; the last step y fma(-h y, y, 1.5) rounds h y,
                       the fma and the product: 2.5 eps, counted as 3).
  point-block term,    the default path forms C = L^-T (point_factor(): A = L L^T, three fast_rsqrt, no division), V = W C, and
  factor form          subtracts V_a V_b^T.  With Y = W X and V = W C (long-double values), the bar of one term W_a X W_b^T is
                         |Y_a| P |Y_b|^T,  P = Delta A + CF eps |L| |L^T|,  CF = 4 + 2 RSQ = 10
                             a perturbation of A moves X by -X dA X, hence the term by -Y_a dA Y_b^T: Hpp's bar and the damping
                             passed through, and the backward error of the 3x3 Cholesky factorisation (Higham, Accuracy and
                             Stability of Numerical Algorithms, theorem 10.3: (n + 1) eps |L| |L^T|; the pivots' reciprocal roots come
                             from fast_rsqrt and enter every entry of their column)
                         + R_a |V_b|^T + |V_a| R_b^T,  R = |W| Q + 5 eps Wabs |C|,  Q = CI eps |C| |L^T| |C|,  CI = 4
                             R bounds the error of the computed V: the inversion of the triangular factor (ibid. section 14.1:
                             |C^ - C| <= c eps |C| |L^T| |C|), the two roundings of an entry of W and the three of a 3-term product sum
                         + 3 eps |V_a| |V_b|^T      the product sum V_a V_b^T itself.
                       This is the bound |W_a| M_j |W_b|^T with M_j = c eps (|C| |L^T| |C| |C^T| + transpose) of the issue that asked for
                       this yardstick, with two changes.  (i) The factorisation's backward error and the input bars are added: the
                       kernel performs those operations first, and they scale the same way with cond(A_j).  (ii) Wherever an error is
                       multiplied by an exact factor, that factor enters as |W X| or |W C|, not as |W| |X| or |W| |C|: the rows of W lie in
                       the range of Hpp, so W X and W C stay bounded where X and C grow with the radius.  |W X| <= |W| |X|: the bar is
                       never wider than the entrywise form, and with the entrywise form no case with a two-view or single-view track
                       had an informative b beyond radius 1e4 (measured: two_cams at 1e4, 50 % of b).
  point-block term,    for the implementations that form X explicitly: XRSFM_BA_PREP_FUSED=0 (k_point_prep: cofactor inverse, then a
  inverse form         Cholesky factor Hc of the inverse, V = W Hc), k_schur_prep / k_schur_matvec on the PCG path (W X W^T from the
                       stored cofactor inverse) and the float64 restatement of the oracle (np.linalg.inv).  The error of an explicit
                       inverse has no structure that W could cancel: the factor-form bar plus |W_a| M_j |W_b|^T with
                         M_j = CV eps |X| |L| |L^T| |X|, CV = 16   an inverse through a factorisation, c eps |X| |A| |X| with
                                                                 |A| <= |L| |L^T| (ibid. section 14.1)
                             + 4 eps (cofabs / |det|) + 8 eps |X| detabs / |det|   running error of the cofactor formula: a cofactor is
                                                                 two products and a difference (cofabs = |p1| + |p2|), the determinant
                                                                 three more products and two sums (detabs = sum |a_0k| cofabs_0k)
                             + 4 eps |Hc| |Hc^T|                 the Cholesky factor of the computed inverse
                       and 13 eps Wabs_a (|X| + |Hc| |Hc^T|) Wabs_b^T for the products (13 = 2 * 2 for the two W, 2 * 3 for the two
                       V, 3 for V_a V_b^T).  It contains the factor form's bar, so it is never the tighter of the two; it is used for
                       those three only.
  b                    W X g_p = V (C^T g_p): bar(g_c) + per observation |Y| P |X g_p| + |Y| bar(g_p) + R |C^T g_p|
                       + |V| ((Q^T + 3 eps |C^T|) |g_p| + 3 eps |C^T g_p|), in the inverse form also |W| M_j |g_p|
                       + 13 eps Wabs (|X| + |Hc| |Hc^T|) |g_p|; then the sum bar + eps (|g_c| + |sum|).
  diagonal block       per observation 2 eps |F|^T |F| + the term's bar + eps (|F|^T |F| + |W X W^T|), the sum bar, and on the
                       diagonal the damping bar formed from the linearisation's own diag Hcc (camlin) + eps (|S_cc| + |d|).
  y = S x              sum_b bar(S_cb) |x_b| with the inverse-form bars + (cw (n_c + 1) + 8) eps sum_b |S_cb| |x_b| (n_c = blocks in
                       the camera's block row) + eps sum_{o of c} (L_j + 8) Wabs_o (|X| + |C| |C^T|) sum_{o' of j} Wabs_o'^T |x_c(o')|:
                       k_schur_matvec never forms S; it adds W_o'^T x over the L_j observations of a track, multiplies by X and by
                       W_o, and adds the damping D x on the host.
  decisions            the clips are taken on the long-double values.  A diagonal entry of Hpp or Hcc within its own bar of 1e-6 (or
                       of 1e32) is FRAGILE: float64 could clip either way.  No case may contain one.  Constant blocks (and cameras or
                       points without an observation) have a diagonal of exactly 0 with bar 0 and are not fragile.

A bar that grows with the conditioning of A_j can become vacuous (it is unbounded for a rank-2 point block at a radius where
A_j == Hpp_j in float64).  An entry is INFORMATIVE when its bar is at most 1e-9 x the largest |entry| of its own block (of its own
camera's b) in the yardstick.  test_schur_cpu.py asserts, from the yardstick alone, at least 99 % informative entries among the
structural blocks and 100 % for b
  * under the factor-form bar for every (case, scaling, radius) of the catalogue, and
  * under the inverse-form bar for every case with a check held to it (has_inverse_check: the XRSFM_BA_PREP_FUSED=0 variant of the
    four all-variant cases, the PCG checks) at the radii INV_RADII = 1 and 100.  The inverse-form bar is about 16 eps cond(A_j)^2
    relative to an entry (an unstructured error of X, seen through |W| on both sides), so it is informative while cond(A_j) is a
    few hundred: at every radius up to 100 on every such case (measured: 100 % of blocks and b), and not beyond.  Those checks
    run at INV_RADII and, after them, at the case's own radii (inverse_radii()).
EXEMPT from the informative-share condition, and so stated: the inverse-form checks at a case's own radii above 100 (3e3 on the
shape catalogue, 1e4 to 1e16 on long, ragged, consts_models, and both radii of low_parallax, 1e4 and 1e12, which the issue sets).
There the kernels are still compared with their bar, entry by entry, but a pass is evidence only for the entries whose share
test_schur_cpu.py prints (shapes at 3e3: 99.9 % / 97.6 % at the least; low_parallax: 23 % / 12 %), and for the sums and the index
arithmetic.  The default path and every factor-form variant have no exemption.
Uninformative entries are still compared with their bar.

check_system's "diag_symmetric" compares each diagonal block with its own transpose as the C side returns it.  It says nothing about
the off-diagonal part: capi.Context.debug_reduced_system builds S from blk and its mirror image, symmetric by construction.
"""
import numpy as np

from tests import backsub_yardstick as BY
from tests import helpers as H
from tests.lin_yardstick import EPS, LD, SUM_EXTRA, V, seg_sum

assert np.finfo(LD).eps < 2e-19, "np.longdouble carries no more than float64 here: the yardstick needs x87 extended precision"
E64 = float(EPS)
LM_MIN, LM_MAX = 1e-6, 1e32
HUBER_A = 5.99
RSQ = 3                     # eps of one fast_rsqrt / fast_rcp
CF, CI, CV = 4 + 2 * RSQ, 4, 16
C_PROD = 13
C_W, C_VV = 5, 3          # roundings of W and of V = W C per entry of V; of a 3-term product sum
C_DAMP = 3
INFORMATIVE = 1e-9
_DIAG6 = (0, 3, 5)
_SYM = np.array([[0, 1, 2], [1, 3, 4], [2, 4, 5]])


# ------------------------------------------------------------------------------------------------ small dense pieces (long double)
def _chol3(A):
    """Lower Cholesky factor of stacked 3x3 A (pivots kept above 1e-300, as point_factor() does)."""
    tiny = LD(1e-300)
    l00 = np.sqrt(np.maximum(A[:, 0, 0], tiny))
    l10 = A[:, 1, 0] / l00; l20 = A[:, 2, 0] / l00
    l11 = np.sqrt(np.maximum(A[:, 1, 1] - l10 * l10, tiny))
    l21 = (A[:, 2, 1] - l20 * l10) / l11
    l22 = np.sqrt(np.maximum(A[:, 2, 2] - l20 * l20 - l21 * l21, tiny))
    L = np.zeros(A.shape, A.dtype)
    L[:, 0, 0], L[:, 1, 0], L[:, 2, 0], L[:, 1, 1], L[:, 2, 1], L[:, 2, 2] = l00, l10, l20, l11, l21, l22
    return L


def _inv_lower(L):
    M = np.zeros(L.shape, L.dtype)
    i0, i1, i2 = 1 / L[:, 0, 0], 1 / L[:, 1, 1], 1 / L[:, 2, 2]
    m10 = -L[:, 1, 0] * i0 * i1
    m21 = -L[:, 2, 1] * i1 * i2
    m20 = -(L[:, 2, 0] * i0 + L[:, 2, 1] * m10) * i2
    M[:, 0, 0], M[:, 1, 1], M[:, 2, 2], M[:, 1, 0], M[:, 2, 1], M[:, 2, 0] = i0, i1, i2, m10, m21, m20
    return M


def _solve_lt(W, L):
    """V with V L^T = W for stacked W [n][m][3] and lower L [n][3][3], by substitution: no product with the entries of L^-1, which
    cancel by cond(L) where the rows of W lie in the range of A."""
    l = lambda i, j: L[:, i, j][:, None]
    v0 = W[:, :, 0] / l(0, 0)
    v1 = (W[:, :, 1] - v0 * l(1, 0)) / l(1, 1)
    v2 = (W[:, :, 2] - v0 * l(2, 0) - v1 * l(2, 1)) / l(2, 2)
    return np.stack([v0, v1, v2], axis=2)


def _mm(*Ms):
    out = Ms[0]
    for M in Ms[1:]:
        out = np.matmul(out, M)
    return out


def _t(M):
    return np.swapaxes(M, -1, -2)


def _cofactor_bar(A):
    """Running error of sym3_inverse (ba_math.h) on |A|, in units of eps, float64 [n][3][3]."""
    a, b, c, d, e, f = (A[:, i, j] for i, j in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)))
    ab = np.abs
    cof = {(0, 0): d * f - e * e, (0, 1): c * e - b * f, (0, 2): b * e - c * d, (1, 1): a * f - c * c, (1, 2): b * c - a * e, (2, 2): a * d - b * b}
    cofabs = {(0, 0): ab(d * f) + e * e, (0, 1): ab(c * e) + ab(b * f), (0, 2): ab(b * e) + ab(c * d), (1, 1): ab(a * f) + c * c,
              (1, 2): ab(b * c) + ab(a * e), (2, 2): ab(a * d) + b * b}
    det = a * cof[0, 0] + b * cof[0, 1] + c * cof[0, 2]
    detabs = ab(a) * cofabs[0, 0] + ab(b) * cofabs[0, 1] + ab(c) * cofabs[0, 2]
    out = np.zeros(A.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        for (i, j), v in cof.items():
            x = 4 * cofabs[i, j] / ab(det) + 8 * ab(v / det) * detabs / ab(det)
            out[:, i, j] = out[:, j, i] = np.asarray(x, np.float64)
    return np.where(np.isfinite(out), out, np.inf)


# ------------------------------------------------------------------------------------------------ the yardstick
def _track_pairs(ci, pi):
    """Every pair of observations of one track, as (pa, pb) with cam[pa] < cam[pb]."""
    order = np.lexsort((ci, pi))
    pts, start, lens = np.unique(pi[order], return_index=True, return_counts=True)
    pa, pb = [], []
    for L in np.unique(lens):
        if L < 2:
            continue
        idx = order[start[lens == L][:, None] + np.arange(L)[None, :]]          # [tracks][L], cameras ascending
        i, j = np.triu_indices(int(L), 1)
        pa.append(idx[:, i].ravel()); pb.append(idx[:, j].ravel())
    if not pa:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    pa, pb = np.concatenate(pa), np.concatenate(pb)
    assert (ci[pa] < ci[pb]).all(), "a track observes one camera twice"
    return pa, pb


def prepare(arr, lin, bars=None):
    """The radius-independent part.  lin: r [No][2], Jc [No][2][cw], Jp [No][2][3] (float64, taken as exact).
    bars (tests/lba_step_yardstick.py): the same three keys, the bars of a linearisation that is itself a computed quantity; lin may
    then hold long-double values.  They travel through Hpp, g_p, diag Hcc and g_c by the (value, bar) arithmetic and, to first
    order, through W = F^T E and F^T F (dW, dFtF: system() adds them where W and F^T F enter)."""
    ci = np.asarray(arr["obs_cam"], np.int64); pi = np.asarray(arr["obs_pt"], np.int64)
    Nc, Np = arr["cam_q"].shape[0], arr["points"].shape[0]
    Jc, Jp, r = (np.ascontiguousarray(lin[k], np.float64) for k in ("Jc", "Jp", "r"))
    cw = Jc.shape[2]
    F, E = np.asarray(lin["Jc"], LD), np.asarray(lin["Jp"], LD)
    Fv, Ev, rv = V(F), V(E), V(np.asarray(lin["r"], LD))
    extra = {}
    if bars is not None:
        eF, eE = np.asarray(bars["Jc"], np.float64), np.asarray(bars["Jp"], np.float64)
        Fv, Ev, rv = V(F, bars["Jc"]), V(E, bars["Jp"]), V(rv.v, bars["r"])
        aF, aE = np.abs(Jc), np.abs(Jp)
        extra = dict(dW=np.einsum("nki,nkj->nij", aF, eE) + np.einsum("nki,nkj->nij", eF, aE),
                     dFtF=np.einsum("nki,nkj->nij", aF, eF) + np.einsum("nki,nkj->nij", eF, aF))
    r0, r1 = rv[:, 0:1], rv[:, 1:2]
    pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
    Hpp = seg_sum(V.stack([Ev[:, 0, a] * Ev[:, 0, b] + Ev[:, 1, a] * Ev[:, 1, b] for a, b in pairs]), pi, Np)
    gp = seg_sum(Ev[:, 0] * r0 + Ev[:, 1] * r1, pi, Np)
    Hcc_diag = seg_sum(Fv[:, 0] * Fv[:, 0] + Fv[:, 1] * Fv[:, 1], ci, Nc)
    gc = seg_sum(Fv[:, 0] * r0 + Fv[:, 1] * r1, ci, Nc)
    pa, pb = _track_pairs(ci, pi)
    keys, pid = (np.unique(np.stack([ci[pa], ci[pb]], axis=1), axis=0, return_inverse=True) if pa.size
                 else (np.zeros((0, 2), np.int64), np.zeros(0, np.int64)))
    return dict(ci=ci, pi=pi, Nc=Nc, Np=Np, cw=cw, F=F, E=E, W=np.einsum("nki,nkj->nij", F, E),
                Wabs=np.einsum("nki,nkj->nij", np.abs(Jc), np.abs(Jp)), FtF=np.einsum("nki,nkj->nij", F, F),
                FtFabs=np.einsum("nki,nkj->nij", np.abs(Jc), np.abs(Jc)), Hpp=Hpp, gp=gp, Hcc_diag=Hcc_diag, gc=gc,
                pa=pa, pb=pb, pid=np.asarray(pid).reshape(-1), keys=keys, n_obs_cam=np.bincount(ci, minlength=Nc),
                track_len=np.bincount(pi, minlength=Np), **extra)


def _damping(h, radius):
    """d = clip(h) / radius as (value, bar) and the fragile flags, h a V.  radius: a float64 taken as exact, or a 0-d V whose bar
    passes through the quotient."""
    lo, hi = LD(LM_MIN), LD(LM_MAX)
    rv, re = (radius.v, radius.e) if isinstance(radius, V) else (LD(radius), LD(0))
    d = np.clip(h.v, lo, hi) / rv
    passes = (h.v > lo) & (h.v < hi)
    fragile = ((np.abs(h.v - lo) <= h.e) | (np.abs(h.v - hi) <= h.e)) & ~((h.v == 0) & (h.e == 0))
    return V(d, np.where(passes, h.e, 0) / rv + np.abs(d) * re / rv + C_DAMP * EPS * np.abs(d)), fragile


def _seg(x, idx, n):
    out = np.zeros((n,) + x.shape[1:], x.dtype)
    np.add.at(out, idx, x)
    return out


def system(prep, radius):
    """The reduced system at one radius.  Returns dict(diag, blk, b: values (long double); diag_bar, blk_bar, b_bar: {"factor",
    "inverse"} -> float64 bars; keys [m][2] (camera a < camera b of blk); fragile (count); pieces for the product bar)."""
    p = prep
    ci, pi, Nc, Np, cw = p["ci"], p["pi"], p["Nc"], p["Np"], p["cw"]
    f64 = lambda x: np.asarray(x, np.float64)
    # the damped point block
    Hpp = p["Hpp"]
    dp, frag_p = _damping(Hpp[:, list(_DIAG6)], radius)
    A = Hpp.v[:, _SYM].copy(); dA = Hpp.e[:, _SYM].copy()
    for k, i6 in enumerate(_DIAG6):
        A[:, k, k] += dp.v[:, k]
        dA[:, k, k] += dp.e[:, k] + EPS * (np.abs(Hpp.v[:, i6]) + np.abs(dp.v[:, k]))
    L = _chol3(A); C = _t(_inv_lower(L)); X = _mm(C, _t(C)); Hc = _chol3(X)
    aX, aL, aC, aH = f64(np.abs(X)), f64(np.abs(L)), f64(np.abs(C)), f64(np.abs(Hc))
    CCt, HHt, LLt = _mm(aC, _t(aC)), _mm(aH, _t(aH)), _mm(aL, _t(aL))
    nz = lambda x: np.nan_to_num(x, nan=np.inf, posinf=np.inf)
    with np.errstate(over="ignore", invalid="ignore"):
        P = f64(dA) + CF * E64 * LLt                                 # Delta A: inputs and the factorisation's backward error
        Q = CI * E64 * _mm(aC, _t(aL), aC)                           # |C^ - C|
        M_inv = nz(E64 * (CV * _mm(aX, LLt, aX) + _cofactor_bar(f64(A)) + 4 * HHt))
    K_inv = aX + HHt
    forms = ("factor", "inverse")

    W, Wabs = p["W"], p["Wabs"]
    aW = f64(np.abs(W))
    Vl = _solve_lt(W, L[pi])                                         # V = W L^-T [No][cw][3], by substitution
    aV = f64(np.abs(Vl)); aY = f64(np.abs(np.matmul(Vl, _t(C[pi]))))  # |W X| = |V C^T|
    with np.errstate(over="ignore", invalid="ignore"):
        YP = nz(np.matmul(aY, P[pi]))
        R = nz(np.matmul(aW, Q[pi])) + C_W * E64 * nz(np.matmul(Wabs, aC[pi]))      # |V^ - V|
    dead = aW.max(axis=(1, 2)) == 0                                  # observations of a constant block pair: exact zeros
    dW = p.get("dW")                                                 # the bars of a computed linearisation (prepare(bars=...))

    def term_bar(a, b, form):                                         # observations a, b of one track
        with np.errstate(over="ignore", invalid="ignore"):
            out = np.matmul(YP[a], _t(aY[b])) + np.matmul(R[a], _t(aV[b])) + np.matmul(aV[a], _t(R[b])) + C_VV * E64 * np.matmul(aV[a], _t(aV[b]))
            if dW is not None:                                        # dW_a |X W_b^T| + |W_a X| dW_b^T
                out = out + np.matmul(dW[a], _t(aY[b])) + np.matmul(aY[a], _t(dW[b]))
            if form == "inverse":
                out = out + nz(_mm(aW[a], M_inv[pi[a]], _t(aW[b]))) + C_PROD * E64 * nz(_mm(Wabs[a], K_inv[pi[a]], _t(Wabs[b])))
        return np.where((dead[a] | dead[b])[:, None, None], 0.0, nz(out))
    allo = np.arange(ci.shape[0])
    # diagonal blocks
    Too = np.matmul(Vl, _t(Vl))
    mag = p["FtFabs"] + f64(np.abs(Too))
    L_c = p["n_obs_cam"].astype(np.float64)[:, None, None]
    diag = _seg(p["FtF"] - Too, ci, Nc)
    sum_c = np.where(L_c > 0, L_c + SUM_EXTRA, 0) * E64 * _seg(mag, ci, Nc)
    dc, frag_c = _damping(p["Hcc_diag"], radius)
    ar = np.arange(cw)
    diag_bar = {}
    for form in forms:
        e = _seg(2 * E64 * p["FtFabs"] + term_bar(allo, allo, form) + E64 * mag, ci, Nc) + sum_c
        if dW is not None:
            e = e + _seg(p["dFtF"], ci, Nc)
        e[:, ar, ar] += f64(dc.e) + E64 * (f64(np.abs(diag[:, ar, ar])) + f64(np.abs(dc.v)))
        diag_bar[form] = e
    diag[:, ar, ar] += dc.v
    # off-diagonal blocks
    pa, pb, pid, keys = p["pa"], p["pb"], p["pid"], p["keys"]
    m = keys.shape[0]
    Tab = np.matmul(Vl[pa], _t(Vl[pb])) if pa.size else np.zeros((0, cw, cw), LD)
    blk = -_seg(Tab, pid, m)
    L_b = np.bincount(pid, minlength=m).astype(np.float64)[:, None, None]
    sum_b = (L_b + SUM_EXTRA) * E64 * _seg(f64(np.abs(Tab)), pid, m)
    blk_bar = {form: _seg(term_bar(pa, pb, form), pid, m) + sum_b for form in forms}
    # right-hand side: W X g_p = V (C^T g_p)
    gp, gc = p["gp"], p["gc"]
    uc = _solve_lt(gp.v[:, None, :], L)[:, 0, :]                     # C^T g_p = L^-1 g_p, per point, by substitution
    ag, axg, auc = f64(np.abs(gp.v)), f64(np.abs(np.einsum("nij,nj->ni", C, uc))), f64(np.abs(uc))
    u = np.einsum("nij,nj->ni", Vl, uc[pi])
    ssum = _seg(u, ci, Nc)
    b = gc.v - ssum
    L1 = p["n_obs_cam"].astype(np.float64)[:, None]
    with np.errstate(over="ignore", invalid="ignore"):
        duc = nz(np.einsum("nji,nj->ni", Q + C_VV * E64 * aC, ag))    # |(C^T g)^ - C^T g|
        tb_f = np.einsum("nij,nj->ni", YP, axg[pi]) + np.einsum("nij,nj->ni", aY, f64(gp.e)[pi]) + np.einsum("nij,nj->ni", R, auc[pi]) \
            + np.einsum("nij,nj->ni", aV, duc[pi] + C_VV * E64 * auc[pi])
        if dW is not None:
            tb_f = tb_f + np.einsum("nij,nj->ni", dW, axg[pi])
        tb_i = tb_f + nz(np.einsum("nij,njk,nk->ni", aW, M_inv[pi], ag[pi])) + C_PROD * E64 * nz(np.einsum("nij,njk,nk->ni", Wabs, K_inv[pi], ag[pi]))
    b_bar = {}
    for form, tb in (("factor", tb_f), ("inverse", tb_i)):
        tb = np.where(dead[:, None], 0.0, nz(tb))
        b_bar[form] = f64(gc.e) + _seg(tb, ci, Nc) + np.where(L1 > 0, L1 + SUM_EXTRA, 0) * E64 * _seg(f64(np.abs(u)), ci, Nc) \
            + E64 * (f64(np.abs(gc.v)) + f64(np.abs(ssum)))
    return dict(diag=diag, blk=blk, b=b, keys=keys, diag_bar=diag_bar, blk_bar=blk_bar, b_bar=b_bar, cw=cw, radius=radius,
                fragile=int(frag_p[p["track_len"] > 0].sum()) + int(frag_c.sum()), X=X, aX=aX, CCt=CCt,
                damp_c=np.asarray(dc.v, np.float64), A=A, dA=dA)


def product(prep, sysm, x):
    """y = S x and its bar (module docstring), x [Nc][cw] float64."""
    p, s = prep, sysm
    ci, pi, Nc, cw = p["ci"], p["pi"], p["Nc"], p["cw"]
    xl = np.asarray(x, np.float64).astype(LD); ax = np.abs(np.asarray(x, np.float64))
    ka, kb = s["keys"][:, 0], s["keys"][:, 1]
    y = np.einsum("nij,nj->ni", s["diag"], xl)
    np.add.at(y, ka, np.einsum("nij,nj->ni", s["blk"], xl[kb]))
    np.add.at(y, kb, np.einsum("nji,nj->ni", s["blk"], xl[ka]))
    f64 = lambda v: np.asarray(v, np.float64)
    aD, aB = f64(np.abs(s["diag"])), f64(np.abs(s["blk"]))
    bar = np.einsum("nij,nj->ni", s["diag_bar"]["inverse"], ax)
    mag = np.einsum("nij,nj->ni", aD, ax)
    np.add.at(bar, ka, np.einsum("nij,nj->ni", s["blk_bar"]["inverse"], ax[kb]))
    np.add.at(bar, kb, np.einsum("nji,nj->ni", s["blk_bar"]["inverse"], ax[ka]))
    np.add.at(mag, ka, np.einsum("nij,nj->ni", aB, ax[kb]))
    np.add.at(mag, kb, np.einsum("nji,nj->ni", aB, ax[ka]))
    n_c = (np.bincount(ka, minlength=Nc) + np.bincount(kb, minlength=Nc)).astype(np.float64)[:, None]
    Wabs = p["Wabs"]
    tsum = _seg(np.einsum("nij,ni->nj", Wabs, ax[ci]), pi, p["Np"])                      # sum_o' Wabs^T |x|, per track
    Kx = np.einsum("nij,nj->ni", s["aX"] + s["CCt"], tsum)
    trk = _seg((p["track_len"][pi].astype(np.float64) + SUM_EXTRA)[:, None] * np.einsum("nij,nj->ni", Wabs, Kx[pi]), ci, Nc)
    return y, bar + (cw * (n_c + 1) + SUM_EXTRA) * E64 * mag + E64 * trk


def product_inputs(n_cams, cw, seed=17):
    """The two x of the PCG product check: random, and zero except on one camera (a wrong neighbour block is not averaged away)."""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(n_cams, cw))
    one = np.zeros((n_cams, cw)); one[n_cams // 2] = rng.normal(size=cw)
    return x, one


# ------------------------------------------------------------------------------------------------ checks
def _ratio(err, bar):
    err = np.asarray(err, LD); bar = np.asarray(bar, LD)
    out = np.where(err == 0, LD(0), LD(np.inf))
    np.divide(err, bar, out=out, where=bar > 0)
    return np.asarray(out, np.float64)


def blocks_of(red):
    """diag [Nc][cw][cw], ({(a, b): block [cw][cw]} with a < b), b [Nc][cw] of a capi.Context.debug_reduced_system result."""
    S, rc, bb = red["S"], np.asarray(red["blk_rc"]), red["b"]
    nc, cw = bb.shape
    D = S.toarray() if S.shape[0] <= 2000 else None
    get = (lambda i, j: D[cw * i:cw * i + cw, cw * j:cw * j + cw]) if D is not None else (lambda i, j: S[cw * i:cw * i + cw, cw * j:cw * j + cw].toarray())
    diag = np.stack([get(i, i) for i in range(nc)])
    blk = {(int(min(a, b)), int(max(a, b))): get(int(min(a, b)), int(max(a, b))) for a, b in rc}
    return diag, blk, bb


def check_system(sysm, diag, blk, b, form):
    """{check: ratio to the bar per entry}.  blk: {(a, b): block}, a < b; its keys must be the structural pairs exactly."""
    keys = [tuple(int(v) for v in k) for k in sysm["keys"]]
    assert sorted(blk) == sorted(keys), ("structural blocks", len(blk), len(keys))
    got = np.stack([blk[k] for k in keys]) if keys else np.zeros((0, sysm["cw"], sysm["cw"]))
    out = dict(diag=_ratio(np.abs(np.asarray(diag, np.float64).astype(LD) - sysm["diag"]), sysm["diag_bar"][form]),
               blk=_ratio(np.abs(got.astype(LD) - sysm["blk"]), sysm["blk_bar"][form]),
               b=_ratio(np.abs(np.asarray(b, np.float64).astype(LD) - sysm["b"]), sysm["b_bar"][form]))
    out["diag_symmetric"] = np.where(np.asarray(diag) == np.swapaxes(np.asarray(diag), 1, 2), 0.0, np.inf)
    return out


def check_constants(arr, sysm, diag, blk, b):
    """Bit for bit: the rows and columns of constant camera parameters (cam_const bits 1 / 2, on bal9 a cleared bit 4) and of
    cameras without an observation are zero except the diagonal 1e-6 / radius; their b is 0."""
    cc = np.asarray(arr["cam_const"]).astype(np.int64)
    Nc, cw = b.shape
    act = np.bincount(arr["obs_cam"], minlength=Nc) > 0
    const = np.zeros((Nc, cw), bool)
    const[:, 0:3] = ((cc & 1) != 0)[:, None]; const[:, 3:6] = ((cc & 2) != 0)[:, None]
    if cw == 9:
        const[:, 6:9] = ((cc & 4) == 0)[:, None]
    const |= ~act[:, None]
    want = np.float64(LM_MIN) / np.float64(sysm["radius"])
    bad = 0
    for c in np.nonzero(const.any(axis=1))[0]:
        for k in np.nonzero(const[c])[0]:
            row = diag[c, k].copy(); col = diag[c, :, k].copy()
            bad += int(row[k] != want); row[k] = 0; col[k] = 0
            bad += int((row != 0).any()) + int((col != 0).any()) + int(b[c, k] != 0)
    for (a, bb), B in blk.items():
        bad += int((B[const[a]] != 0).any()) + int((B[:, const[bb]] != 0).any())
    return bad, int(const.sum())


def informative(sysm, form):
    """Shares of informative entries: (structural blocks, b)."""
    with np.errstate(invalid="ignore"):
        d = sysm["diag_bar"][form] <= INFORMATIVE * np.abs(sysm["diag"]).max(axis=(1, 2), keepdims=True).astype(np.float64)
        o = sysm["blk_bar"][form] <= INFORMATIVE * np.abs(sysm["blk"]).max(axis=(1, 2), keepdims=True).astype(np.float64)
        bb = sysm["b_bar"][form] <= INFORMATIVE * np.abs(sysm["b"]).max(axis=1, keepdims=True).astype(np.float64)
    return (int(d.sum()) + int(o.sum())) / max(d.size + o.size, 1), int(bb.sum()) / max(bb.size, 1)


def worst(checks):
    return {k: ((float(np.max(v)), int(np.argmax(v))) if np.size(v) else (0.0, -1)) for k, v in checks.items()}


def assert_inside(checks, what):
    w = worst(checks)
    bad = {k: x for k, x in w.items() if not x[0] <= 1.0}
    assert not bad, f"{what}: outside the bar (ratio, flat index): {bad}"
    return w


# ------------------------------------------------------------------------------------------------ float64 restatements
def _lin64(arr, lin):
    ci = np.asarray(arr["obs_cam"], np.int64); pi = np.asarray(arr["obs_pt"], np.int64)
    Nc, Np = arr["cam_q"].shape[0], arr["points"].shape[0]
    F, E, r = (np.asarray(lin[k], np.float64) for k in ("Jc", "Jp", "r"))
    add = lambda n, idx, x: _seg(x, idx, n)
    return dict(ci=ci, pi=pi, Nc=Nc, Np=Np, F=F, E=E, W=np.einsum("nki,nkj->nij", F, E), Hpp=add(Np, pi, np.einsum("nki,nkj->nij", E, E)),
                gp=add(Np, pi, np.einsum("nki,nk->ni", E, r)), gc=add(Nc, ci, np.einsum("nki,nk->ni", F, r)),
                FtF=np.einsum("nki,nkj->nij", F, F))


def _assemble64(l, V_, u, radius, keys_of):
    """Blocks from per-observation V [No][cw][3] (V V^T = W X W^T) and u = the point's 3-vector with V u = W X g_p."""
    ci, pi, Nc = l["ci"], l["pi"], l["Nc"]
    diag = _seg(l["FtF"] - np.matmul(V_, _t(V_)), ci, Nc)
    cw = diag.shape[1]
    ar = np.arange(cw)
    diag[:, ar, ar] += np.clip(_seg(np.einsum("nki,nki->ni", l["F"], l["F"]), ci, Nc), LM_MIN, LM_MAX) / radius
    b = l["gc"] - _seg(np.einsum("nij,nj->ni", V_, u[pi]), ci, Nc)
    pa, pb, pid, keys = keys_of
    blk = -_seg(np.matmul(V_[pa], _t(V_[pb])), pid, keys.shape[0]) if pa.size else np.zeros((0, cw, cw))
    return diag, {tuple(int(v) for v in k): blk[i] for i, k in enumerate(keys)}, b


def restatement_inverse(arr, lin, radius, prep):
    """The oracle's formulas in float64 through np.linalg.inv (helpers.reduced_system_oracle), from the given linearisation."""
    l = _lin64(arr, lin)
    D = np.clip(np.einsum("nii->ni", l["Hpp"]), LM_MIN, LM_MAX) / radius
    Hinv = np.linalg.inv(l["Hpp"] + np.einsum("ni,ij->nij", D, np.eye(3)))
    ci, pi, Nc = l["ci"], l["pi"], l["Nc"]
    WH = np.matmul(l["W"], Hinv[pi])
    diag = _seg(l["FtF"], ci, Nc)
    cw = diag.shape[1]; ar = np.arange(cw)
    diag[:, ar, ar] += np.clip(diag[:, ar, ar], LM_MIN, LM_MAX) / radius
    diag -= _seg(np.matmul(WH, _t(l["W"])), ci, Nc)
    diag = np.triu(diag) + _t(np.triu(diag, 1))
    b = l["gc"] - _seg(np.einsum("nij,nj->ni", WH, l["gp"][pi]), ci, Nc)
    pa, pb, pid, keys = prep["pa"], prep["pb"], prep["pid"], prep["keys"]
    blk = -_seg(np.matmul(WH[pa], _t(l["W"][pb])), pid, keys.shape[0]) if pa.size else np.zeros((0, cw, cw))
    return diag, {tuple(int(v) for v in k): blk[i] for i, k in enumerate(keys)}, b


def point_factor64(h6, radius):
    """float64 transcription of point_factor() (ba_math.h) with a plain 1 / sqrt for fast_rsqrt: C upper, [n][3][3]."""
    ir = 1.0 / radius
    clip = lambda v: np.minimum(np.maximum(v, LM_MIN), LM_MAX)
    h00 = clip(h6[:, 0]) * ir + h6[:, 0]; h11 = clip(h6[:, 3]) * ir + h6[:, 3]; h22 = clip(h6[:, 5]) * ir + h6[:, 5]
    r0 = 1.0 / np.sqrt(h00)
    l10 = h6[:, 1] * r0; l20 = h6[:, 2] * r0
    r1 = 1.0 / np.sqrt(np.maximum(h11 - l10 * l10, 1e-300))
    l21 = (h6[:, 4] - l20 * l10) * r1
    r2 = 1.0 / np.sqrt(np.maximum(h22 - l20 * l20 - l21 * l21, 1e-300))
    m10 = -l10 * r0 * r1
    m21 = -l21 * r1 * r2
    m20 = -(l20 * r0 + l21 * m10) * r2
    C = np.zeros((h6.shape[0], 3, 3))
    C[:, 0, 0], C[:, 0, 1], C[:, 0, 2], C[:, 1, 1], C[:, 1, 2], C[:, 2, 2] = r0, m10, m20, r1, m21, r2
    return C


def restatement_factor(arr, lin, radius, prep):
    """The default path's arithmetic in float64: C from point_factor64, V = W C, blocks from V_a V_b^T, b from V (C^T g_p)."""
    l = _lin64(arr, lin)
    H = l["Hpp"]
    C = point_factor64(np.stack([H[:, 0, 0], H[:, 0, 1], H[:, 0, 2], H[:, 1, 1], H[:, 1, 2], H[:, 2, 2]], axis=1), radius)
    V_ = np.matmul(l["W"], C[l["pi"]])
    u = np.einsum("nji,nj->ni", C, l["gp"])
    diag, blk, b = _assemble64(l, V_, u, radius, (prep["pa"], prep["pb"], prep["pid"], prep["keys"]))
    return np.triu(diag) + _t(np.triu(diag, 1)), blk, b


def oracle_lin(arr, use_scaling=True):
    """CPU stand-in for the kernel's linearisation: the oracle's (r, Jc, Jp), Jacobi-scaled like iteration 0 of a solve."""
    from tests import lin_yardstick as LY
    out = LY.float64_restatement(arr, use_scaling)
    return dict(r=out["r"], Jc=out["Jc"], Jp=out["Jp"])


# ------------------------------------------------------------------------------------------------ cases
def pair_small():
    """Three tracks over the cameras 0..10 (a tile of 11 cameras: per-pair records) among 3-camera tracks."""
    tracks = [np.arange(11) for _ in range(3)] + [np.array([c, (c + 1) % 12, (c + 2) % 12]) for c in range(12) for _ in range(2)]
    return H.make_tracks(12, [np.sort(t) for t in tracks], seed=41)


def bal9_gram_tiles(k_cams, ragged):
    """The problem of test_gpu_bal9.py::test_bal9_gram_tiles_of_every_camera_count."""
    kw = dict(mode="unordered", min_tri_angle_deg=0.5)
    n_cams = k_cams + (3 if ragged else 0)
    if ragged:
        kw["dropout"] = 0.3
    return H.make_bal9(n_cams, 260, min(k_cams + (2 if ragged else 0), n_cams), seed=300 + 10 * k_cams + int(ragged), **kw)


INV_RADII = (1.0, 100.0)                # where the inverse-form bar is informative on every case (module docstring)
R_SINGLE = (1.0, 1e4, 1e8)              # cases with single-observation tracks (singular to float64 from radius 1e10 on)
R_FULL = (1.0, 1e4, 1e8, 1e16)
ALL_VARIANTS = ("shape0", "ragged", "shape12", "long")          # Gram-only, ragged, per-pair tiles, long items
# name -> dict(make, radii, env the case needs (set before the context exists), scalings (6-wide), pcg)
CASES = {}


def _add(name, make, radii, env=None, scalings=(True,), pcg=False, wide=False):
    CASES[name] = dict(make=make, radii=tuple(radii), env=dict(env or {}), scalings=tuple(scalings), pcg=pcg, wide=wide)


for _i in range(21):
    _add(f"shape{_i}", (lambda i=_i: BY._shape(i)), (3e3,), scalings=(True, False) if _i in (0, 12) else (True,), pcg=True)
_add("long", lambda: H.long_problem((65, 128, 129, 200), 5), R_FULL, scalings=(True, False), pcg=True)
_add("consts_models", BY.consts_models, R_SINGLE, pcg=True)
_add("ragged", BY.ragged, R_SINGLE)
_add("full_tile", BY.full_tile, R_SINGLE)
_add("two_cams", lambda: H.make(2, 150, 2), R_FULL)
_add("pose", lambda: H.make_pose_problem(200), R_SINGLE)
_add("low_parallax", lambda: H.make(8, 300, 2, min_tri_angle_deg=0.0), (1e4, 1e12), pcg=True)
_add("same_tuple", lambda: H.make(40, 2000, 4), R_FULL, env={"XRSFM_BA_SGROUP": "4"})
_add("ten_cams", lambda: H.make(60, 1500, 10), R_FULL)
_add("pair_v0", pair_small, R_FULL, env={"XRSFM_BA_PAIR_V": "0"})
_add("pair_v1", pair_small, R_FULL, env={"XRSFM_BA_PAIR_V": "1"})
_add("packed", lambda: H.make(40, 600, 3, seed=21), R_FULL, env={"XRSFM_BA_PACKED": "1"})
_add("bal9_ragged_consts", BY.bal9_ragged_consts, R_SINGLE, wide=True)
_add("bal9_long", BY.bal9_long, R_FULL, wide=True)
for _k in range(2, 9):
    _add(f"bal9_k{_k}", (lambda k=_k: bal9_gram_tiles(k, False)), (2e3,), wide=True)
    _add(f"bal9_k{_k}r", (lambda k=_k: bal9_gram_tiles(k, True)), (2e3,), wide=True)
FAMILIES = {"shapes": tuple(f"shape{i}" for i in range(21)), "long": ("long",),
            "make": ("consts_models", "ragged", "full_tile", "two_cams", "pose", "same_tuple", "ten_cams", "packed"),
            "low_parallax": ("low_parallax",), "pair": ("pair_v0", "pair_v1"), "bal9": tuple(n for n in CASES if n.startswith("bal9"))}
assert sorted(n for f in FAMILIES.values() for n in f) == sorted(CASES)
ENV_KEYS = ("XRSFM_BA_PREP_FUSED", "XRSFM_BA_JFREE", "XRSFM_BA_GRAM4", "XRSFM_BA_GRAM_MERGE", "XRSFM_BA_SGROUP", "XRSFM_BA_PAIR_V", "XRSFM_BA_PACKED")
_ARR = {}


def has_inverse_check(name):
    """A check of this case is held to the inverse-form bar (XRSFM_BA_PREP_FUSED=0 on the all-variant cases, the PCG path)."""
    return name in ALL_VARIANTS or CASES[name]["pcg"]


def inverse_radii(name):
    """The radii of the inverse-form checks of a case: INV_RADII (informative share asserted), then the case's own (exempt above 100)."""
    return INV_RADII + tuple(r for r in CASES[name]["radii"] if r not in INV_RADII)


def family_of(name):
    return next(f for f, names in FAMILIES.items() if name in names)


def case(name):
    """The problem of a case (built once; callers must not modify it)."""
    if name not in _ARR:
        _ARR[name] = CASES[name]["make"]()
    return _ARR[name]
