"""Yardstick, catalogue and checker of the resident-solver step tests (tests/test_lba_step_cpu.py, tests/test_gpu_lba_step.py).

lba_resident_solve (xrsfm_amd/csrc/ba_lba.h; k_lba_resident, k_lba_batch) runs a whole Levenberg-Marquardt loop in one workgroup,
with its own linearisation, gather of the reduced system, 60x60 Cholesky, back-substitution and trust-region book-keeping.  A run
with max_iterations = k returns the state after exactly k attempted steps, so every step is visible through the public calls (and,
for the resident path, through the iteration rows of xrsfm_ba_debug_resident_rows).  The yardstick restates one step in
np.longdouble on the (value, bar) arithmetic of tests/lin_yardstick.py (V, reference, seg_sum, _quat_plus_diff, ratio), the
reduced system of tests/schur_yardstick.py (prepare, system) and the operation counts of tests/backsub_yardstick.py; the decision
rules are those of tests/pose_step_yardstick.py (decide, grow).  It never calls the library.

One step from the float64 state (q, t, P), the scales s_c, s_p, the radius R and the options:

  linearisation   lin_yardstick.reference at the state, unscaled: r, F, E with their bars, cost = 1/2 sum rho, |x_points|^2.  The scales
                  s = 1 / (1 + sqrt(diag)) come from the FIRST linearisation of the run only; F s_c and E s_p carry the bars of both
                  factors.  Constant blocks and cameras / points without an observation have exactly zero columns (bar 0).
                  Gradient max-norm from the scaled sums divided by the scales, as the kernel forms it.
  damped system   schur_yardstick.prepare / system on the scaled blocks: A_j = Hpp_j + clip(diag Hpp_j, 1e-6, 1e32) / R,
                  S_cc = Hcc_c + clip(diag Hcc_c) / R - sum W X W^T, S_ab = - sum W_a X W_b^T, b = g_c - sum W X g_p, values through the
                  long-double factor of A_j.  Bars: that module's factor-form bars (the resident kernel and the engine's default path
                  both use point_factor()), to which prepare(bars=...) adds the first-order propagation of the linearisation's own
                  bars: they enter Hpp, g_p, diag Hcc, g_c through the (value, bar) arithmetic, W = F^T E through
                  dW = |F|^T bar(E) + bar(F)^T |E| (dW_a |X W_b^T| + |W_a X| dW_b^T per term, dW |X g_p| in b) and F^T F through
                  |F|^T bar(F) + bar(F)^T |F|.  The radius is a (value, bar) too: |d| bar(R) / R on every damping term.  The sum bar
                  there holds for any order, so it covers the kernel's chunks and slices and the engine's segmented sums alike.
                  A diagonal within its own bar of a clip bound is FRAGILE (schur_yardstick).
  solve           long-double Cholesky S = L L^T, y = S^-1 b, componentwise forward bar
                      |dy| <= |S^-1| (bar(S) |y| + bar(b) + GAMMA(n) |L| |L^T| |y|),   n = 6 n_cams <= 60.
                  Componentwise on purpose: constant cameras leave decoupled rows with the diagonal 1e-6 / R, which make a normwise
                  condition number meaningless; here such a row has y = 0 with bar 0.
                  GAMMA(n) = (3 n + 1 + n (RSQ + 2)) eps:  3 n + 1 is the backward error of a Cholesky solve of order n (Higham,
                  Accuracy and Stability of Numerical Algorithms, Thm 10.4: (S + dS) y^ = b, |dS| <= gamma_{3n+1} |L| |L^T|, for any
                  order of the inner sums).  That theorem's factor divides by the pivot's root; the kernels multiply by its
                  reciprocal instead, which adds per eliminated column the reciprocal root (1 / sqrt in ba_lba.h: 2 roundings;
                  fast_rsqrt in the engine's tile factorisation, ba_chol.h: RSQ = 3 eps by schur_yardstick's count, the larger is
                  taken) and the two scaled products (S_ij inv) (S_kj inv) of the update: RSQ + 2 = 5 more roundings on an entry
                  per column, and an entry passes through at most n columns.  (8 n + 1) eps in all, 481 eps at n = 60; derived, not fitted.
  step            u_j = A_j^-1 (g_pj - sum_o E_o^T F_o y_c) (long double, two refinement steps), candidate P_c = P - u s_p,
                  q_c = Plus(q, -y s_c), t_c = t - y s_c on the variable blocks, model decrease sum_o m_o . (r_o - m_o / 2) with
                  m_o = F_o y_c + E_o u.  Bars (|.| = 2-norm, L = track length):
                      |du_j| <= |A_j^-1| ((32 + 18 L) eps (|A_j| |u_j| + |g_pj| + sum |E| |F| |y_c|)      backsub_yardstick's backward error
                                        + |bar(g_pj)| + sum (|bar E| |F| |y| + |E| |bar F| |y|) + |bar A_j| |u_j|)   in every component,
                                 + sum_o |W_o X_j|^T bar(y_c)        the bar of y entry by entry: du = -X W^T dy, and W X stays bounded
                                                                     where X grows with the radius (schur_yardstick); the 2-norm form
                                                                     |A^-1| |E| |F| |bar y| was 1e3 times wider on 4-view tracks
                      bar(P_c) = 8 eps (|P| + |u s_p|) + s_p |du| + |u| bar(s_p)                          backsub_yardstick's candidate bar
                      bar(model) = (32 + n_obs) eps sum a_o (|r_o| + a_o), a_o = |F| |y| + |E| |u|           its model bar, one item
                                   + sum (|r_o - m_o| bar(m_o) + |m_o| |bar r_o|), bar(m_o) = |bar F| |y| + |F| |bar y| + |bar E| |u| + |E| |du|
                  The cameras' candidates carry the bars of the (value, bar) arithmetic (sin, cos: 4 eps).  Squared step and |x|^2 over
                  the variable blocks of cameras and points that have an observation, through the sum bar.
  decisions       in the kernel's order: model > 0 and finite (a chain that meets anything else raises Unsupported); parameter-, then
                  function-tolerance exit (both keep the point: reasons 2, 3); rho = (cost - cost_c) / model > 1e-3; on success
                  R / max(1/3, 1 - (2 rho - 1)^3) capped at 1e16, decrease factor back to 2, then the gradient test at the new point
                  (reason 1); on rejection R / decrease (an exact division by a power of two), the factor doubles; the iteration limit
                  gives reason 5.  A decision whose margin lies inside its bar is FRAGILE.

Seating follows pose_step_yardstick.py.  Iteration j starts from the float64 state the code under test returned for
max_iterations = j - 1, taken as exact, so no bar accumulates.  The scales come from the yardstick's first linearisation at the
initial state, the radius and the decrease factor from the yardstick's own chain (carried as V).  If the yardstick accepts the step
the code under test must have moved; its cameras and points are compared with the candidate bars, and cost_c, rho and the new radius
are then taken at the state it returned (the decision must come out the same).  If the point is kept the state must be bit-equal to
the previous one, and the decision must hold with cost_c widened by |grad cost| . bar(candidate): the gradient over points and
translations is the linearisation's own unscaled g_p, g_t at the candidate, over the quaternions it is taken by central differences
(h = 2^-20) per camera.  The chain is valid only while the counters agree and stops at the first difference.

The iteration rows of the resident path {cost, change, gmax, step, rho, radius, it} are checked row by row: cost against the cost
bar at the returned point, gmax against the gradient max-norm bar, change against cost - cost_c with both bars, rho against change /
model, radius against the chain, step against the norm of the difference of the returned states (accepted step; exact in long
double) or the yardstick's step norm (rejected step) with the bar ((N + 8 + 4) / 2 + 1) eps relative: N squared differences,
each a rounded difference and a rounded square, summed in any order, and one square root.

So that the check cannot go vacuous, bar(delta) <= 1e-6 max |delta| (DELTA_CAP) is required of the camera step and of the point step
of every case and iteration (test_lba_step_cpu.py); a case that misses it gets a shorter chain or another seed, never another cap.
"""
import dataclasses

import numpy as np

from tests import backsub_yardstick as BY
from tests import helpers as H
from tests import lin_yardstick as Y
from tests import pose_step_yardstick as PY
from tests import schur_yardstick as SY

V, LD, EPS = Y.V, Y.LD, Y.EPS
Unsupported, Report = PY.Unsupported, PY.Report
DELTA_CAP = PY.DELTA_CAP
CONVERGENCE, NO_CONVERGENCE = 0, 1
FIELDS = PY.FIELDS
ROW_FIELDS = ("cost", "change", "gmax", "step", "rho", "radius")
DEFAULTS = dict(initial_radius=1e4, huber_a=5.99, function_tolerance=1e-6, parameter_tolerance=1e-8, gradient_tolerance=1e-10)
LBA_TOL = dict(function_tolerance=1e-4, parameter_tolerance=1e-5)        # the local BA's own tolerances (test_gpu_lba_resident.py)


def GAMMA(n):
    """The backward-error constant of the Cholesky solve of order n (module docstring)."""
    return (3 * n + 1 + n * (SY.RSQ + 2)) * EPS


# ------------------------------------------------------------------------------------------------ linearisation
def _arr_at(case, st):
    return dict(case.arr, cam_q=st["q"], cam_t=st["t"], points=st["P"])


def linearise(case, st):
    """lin_yardstick.reference at the float64 state st = dict(q, t, P), unscaled."""
    return Y.reference(_arr_at(case, st), False, case.opts["huber_a"])


def scales(ref):
    """(s_c [Nc][6], s_p [Np][3]) as V from an unscaled linearisation."""
    return 1.0 / (1.0 + ref["Hcc_diag"].sqrt()), 1.0 / (1.0 + ref["Hpp"][:, [0, 3, 5]].sqrt())


def _gather(x, idx):
    return V(x.v[idx][:, None, :], x.e[idx][:, None, :])


def scaled_system(case, st, ref, sc):
    """schur_yardstick.prepare on the scaled blocks F s_c, E s_p with their bars, and the gradient max-norm."""
    arr = _arr_at(case, st)
    ci = np.asarray(arr["obs_cam"], np.int64); pi = np.asarray(arr["obs_pt"], np.int64)
    Fs, Es, r = ref["Jc"] * _gather(sc[0], ci), ref["Jp"] * _gather(sc[1], pi), ref["r"]
    prep = SY.prepare(arr, dict(r=r.v, Jc=Fs.v, Jp=Es.v), bars=dict(r=r.e, Jc=Fs.e, Jp=Es.e))
    prep.update(Fe=np.asarray(Fs.e, np.float64), Ee=np.asarray(Es.e, np.float64), r=r)
    cc = np.asarray(arr["cam_const"]).astype(np.int64)
    act = ref["active_cam"]
    qvar, tvar = act & ((cc & 1) == 0), act & ((cc & 2) == 0)
    gu_c, gu_p = prep["gc"] / sc[0], prep["gp"] / sc[1]
    cand = [gu_p[ref["pvar"]], gu_c[tvar][:, 3:6]]
    if qvar.any():
        q = np.asarray(st["q"], np.float64)[qvar]
        cand.append(Y._quat_plus_diff([V(q[:, k]) for k in range(4)], [-gu_c[qvar][:, k] for k in range(3)]))
    prep.update(gmax=Y._max_norm(cand), qvar=qvar, tvar=tvar, pvar=ref["pvar"], xnorm2_pts=ref["xnorm2_pts"])
    return prep


# ------------------------------------------------------------------------------------------------ the solve
def _chol(S):
    n = S.shape[0]
    L = np.zeros((n, n), LD)
    for j in range(n):
        d = S[j, j] - (L[j, :j] * L[j, :j]).sum()
        if not d > 0:
            raise Unsupported("S is not positive definite")
        L[j, j] = np.sqrt(d)
        if j + 1 < n:
            L[j + 1:, j] = (S[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def _llt_solve(L, B):
    """S^-1 B for S = L L^T, B [n] or [n][m]."""
    n = L.shape[0]
    Y_ = np.array(B, LD)
    for i in range(n):
        Y_[i] = (Y_[i] - L[i, :i] @ Y_[:i]) / L[i, i]
    for i in range(n - 1, -1, -1):
        Y_[i] = (Y_[i] - L[i + 1:, i] @ Y_[i + 1:]) / L[i, i]
    return Y_


def dense(sysm, Nc):
    """S, bar(S) [n][n], b, bar(b) [n] in camera order from schur_yardstick.system's blocks (factor-form bars; a bar of the diagonal
    block is taken as the larger of the entry's and its mirror image's, since the kernels form one triangle only)."""
    n = 6 * Nc
    S, Se = np.zeros((n, n), LD), np.zeros((n, n), LD)
    db = sysm["diag_bar"]["factor"]
    for c in range(Nc):
        S[6 * c:6 * c + 6, 6 * c:6 * c + 6] = sysm["diag"][c]
        Se[6 * c:6 * c + 6, 6 * c:6 * c + 6] = np.maximum(db[c], db[c].T)
    for i, (a, b) in enumerate(sysm["keys"]):
        S[6 * a:6 * a + 6, 6 * b:6 * b + 6] = sysm["blk"][i]; S[6 * b:6 * b + 6, 6 * a:6 * a + 6] = sysm["blk"][i].T
        e = sysm["blk_bar"]["factor"][i]
        Se[6 * a:6 * a + 6, 6 * b:6 * b + 6] = e; Se[6 * b:6 * b + 6, 6 * a:6 * a + 6] = e.T
    return S, Se, np.asarray(sysm["b"], LD).reshape(-1), np.asarray(sysm["b_bar"]["factor"], LD).reshape(-1)


def _frob(M):
    return np.sqrt(np.sum(np.asarray(M, np.float64) ** 2, axis=(-2, -1)))


def solve_step(case, st, prep, sc, R):
    """One proposed step from the state st with the linearisation prep (scaled_system), the scales sc and the radius R (V).  Returns a
    dict: y, qc, tc, Pc, model, step_norm, xnorm (V), dcam / dpt (the scaled steps as V), cap, fragile (names)."""
    Nc, Np, ci, pi = prep["Nc"], prep["Np"], prep["ci"], prep["pi"]
    sysm = SY.system(prep, R)
    fragile = [f"{sysm['fragile']} damping clips"] if sysm["fragile"] else []
    S, Se, b, be = dense(sysm, Nc)
    n = 6 * Nc
    L = _chol(S)
    y = _llt_solve(L, b)
    Sinv = _llt_solve(L, np.eye(n, dtype=LD))
    ay, aL = np.abs(y), np.abs(L)
    ye = np.abs(Sinv) @ (Se @ ay + be + GAMMA(n) * (aL @ (aL.T @ ay)))
    yV = V(y.reshape(Nc, 6), ye.reshape(Nc, 6))
    # ---- cameras
    q, t, P = (np.asarray(st[k], np.float64) for k in ("q", "t", "P"))
    qvar, tvar, pvar = prep["qvar"], prep["tvar"], prep["pvar"]
    dcam = -(yV * sc[0])
    diff = Y._quat_plus_diff([V(q[:, k]) for k in range(4)], [dcam[:, k] for k in range(3)])
    qc = V.where(qvar[:, None], V(q) - diff, V(q))
    tc = V.where(tvar[:, None], V(t) + dcam[:, 3:6], V(t))
    # ---- points
    F, E, r = prep["F"], prep["E"], prep["r"]
    F64, E64 = np.asarray(F, np.float64), np.asarray(E, np.float64)
    yv, yev = yV.v, yV.e
    v = np.einsum("nki,ni->nk", F, yv[ci])
    gp = prep["gp"]
    a = gp.v - SY._seg(np.einsum("nki,nk->ni", E, v), pi, Np)
    A, dA = sysm["A"], sysm["dA"]
    u = BY._solve3(A, a)
    eye = np.eye(3, dtype=LD)
    nE, nF, eE, eF = BY._norm2(E64), BY._norm2(F64), _frob(prep["Ee"]), _frob(prep["Fe"])
    ny, ney, nu = BY._vnorm(yv), BY._vnorm(yev), BY._vnorm(u)
    Ltr = prep["track_len"]
    nAinv = BY._norm2(np.stack([BY._solve3(A, np.broadcast_to(eye[k], (Np, 3))) for k in range(3)], axis=2))
    res = (32 + 18 * Ltr) * EPS * (BY._norm2(A) * nu + BY._vnorm(gp.v) + SY._seg(nE * nF * ny[ci], pi, Np))
    da = BY._vnorm(gp.e) + SY._seg(eE * nF * ny[ci] + nE * eF * ny[ci], pi, Np)
    aYt = np.abs(np.einsum("nij,njk->nik", prep["W"], sysm["X"][pi]))   # |W_o X_j| [No][6][3]: du = -X W^T dy, entry by entry
    duc = nAinv[:, None] * (res + da + _frob(dA) * nu)[:, None] + SY._seg(np.einsum("nij,ni->nj", aYt, yev[ci]), pi, Np)
    du = BY._vnorm(duc)                                                # 2-norm bar of u, per point
    sp = sc[1]
    us = u * sp.v
    dpt = V(-us, np.abs(sp.v) * duc + np.abs(u) * sp.e)
    Pc = V(np.where(pvar[:, None], P.astype(LD) - us, P.astype(LD)),
           np.where(pvar[:, None], 8 * EPS * (np.abs(P) + np.abs(us)) + dpt.e, 0))
    dpt = V(np.where(pvar[:, None], dpt.v, 0), np.where(pvar[:, None], dpt.e, 0))
    # ---- model decrease
    m = v + np.einsum("nki,ni->nk", E, u[pi])
    model_v = np.sum(m * (r.v - m / 2))
    ao = nF * ny[ci] + nE * nu[pi]
    dm = eF * ny[ci] + nF * ney[ci] + eE * nu[pi] + nE * du[pi]
    model_e = (32 + ci.shape[0]) * EPS * np.sum(ao * (BY._vnorm(r.v) + ao)) + np.sum(BY._vnorm(r.v - m) * dm + BY._vnorm(m) * BY._vnorm(r.e))
    # ---- step norm and |x| over the variable blocks
    terms, xs = [], []
    for c, x, msk in ((qc, q, qvar), (tc, t, tvar), (Pc, P, pvar)):
        d = V((c.v - x)[msk], (c.e + EPS * np.abs(c.v))[msk])         # the candidate is rounded to float64 before the difference
        terms.append((d * d).v.reshape(-1)); terms.append((d * d).e.reshape(-1))
        xs.append(x[msk].reshape(-1))
    sq = V(np.concatenate(terms[0::2]), np.concatenate(terms[1::2]))
    zero = lambda k: np.zeros(k, np.int64)
    st2 = Y.seg_sum(sq, zero(sq.v.shape[0]), 1)[0] if sq.v.size else V(LD(0))
    xq = V(np.concatenate(xs[:2]))
    xn2 = (Y.seg_sum(xq * xq, zero(xq.v.shape[0]), 1)[0] if xq.v.size else V(LD(0))) + prep["xnorm2_pts"]
    cap = 0.0
    for d in (V(dcam.v[np.stack([qvar] * 3 + [tvar] * 3, axis=1)], dcam.e[np.stack([qvar] * 3 + [tvar] * 3, axis=1)]), dpt):
        if d.v.size and (np.abs(d.v).max() > 0 or d.e.max() > 0):
            dmax = np.abs(d.v).max()
            cap = max(cap, float(d.e.max() / dmax) if dmax > 0 else float("inf"))
    return dict(y=yV, qc=qc, tc=tc, Pc=Pc, model=V(model_v, model_e), step_norm=st2.sqrt(), xnorm=xn2.sqrt(), cap=cap, fragile=fragile,
                dcam=dcam, dpt=dpt)


def cost_sensitivity(case, cand, lin_c, qe, te, Pe):
    """|grad cost| . bar over the candidate's parameters (module docstring)."""
    out = (np.abs(lin_c["gp"].v) * Pe).sum() + (np.abs(lin_c["gc"].v[:, 3:6]) * te).sum()
    arr = _arr_at(case, cand)
    h = 2.0 ** -20
    for c in np.nonzero(qe.max(axis=1) > 0)[0]:
        sel = np.asarray(arr["obs_cam"]) == c
        sub = dict(arr, obs_cam=arr["obs_cam"][sel], obs_pt=arr["obs_pt"][sel], obs_uv=arr["obs_uv"][sel])
        for k in range(4):
            qp, qm = np.array(cand["q"], copy=True), np.array(cand["q"], copy=True)
            qp[c, k] += h; qm[c, k] -= h
            d = (Y.reference(dict(sub, cam_q=qp), False, case.opts["huber_a"])["cost"].v
                 - Y.reference(dict(sub, cam_q=qm), False, case.opts["huber_a"])["cost"].v) / LD(qp[c, k] - qm[c, k])
            out += np.abs(d) * qe[c, k]
    return out


# ------------------------------------------------------------------------------------------------ the checker
def _r64(x):
    return np.ascontiguousarray(np.asarray(x.v, np.float64))


def _same(a, b):
    return all(np.asarray(a[k], np.float64).tobytes() == np.asarray(b[k], np.float64).tobytes() for k in ("q", "t", "P"))


def _state(src):
    return {k: np.ascontiguousarray(src[k], dtype=np.float64) for k in ("q", "t", "P")}


def _step_bar(n_terms):
    return ((n_terms + Y.SUM_EXTRA + 4) / 2 + 1) * EPS


_LIN0 = {}


def _initial(case):
    if case.name not in _LIN0:
        st = _state(dict(q=case.arr["cam_q"], t=case.arr["cam_t"], P=case.arr["points"]))
        ref = linearise(case, st)
        sc = scales(ref)
        _LIN0[case.name] = (st, ref, sc, scaled_system(case, st, ref, sc))
    return _LIN0[case.name]


def check_case(case, run=None):
    """Walk the case's iterations.  run(k) is the code under test at max_iterations = k: a dict with q, t, P, initial_cost, final_cost,
    FIELDS and rows (a list of dicts over ROW_FIELDS + it, or None where the path has none).  run = None seats the yardstick on
    itself (its own candidates, rounded to float64): coverage()."""
    rep = Report()
    opts = case.opts
    st, ref, sc, prep = _initial(case)
    ref0 = ref
    if ref["fragile"].any():
        rep.fragile.append(f"{int(ref['fragile'].sum())} fragile observations at the start")
    cost, R, dec = ref["cost"], V(np.float64(opts["initial_radius"])), 2.0
    gtol = V(np.float64(opts["gradient_tolerance"]))
    ns = nu = att = 0
    done = None
    if PY._inside(prep["gmax"], gtol):
        rep.fragile.append("gradient test at the start")
    if prep["gmax"].v <= gtol.v:
        done = (CONVERGENCE, 1)
    decisions, radii, n_rows, prev_rows = [], [float(R.v)], 1, None
    gmaxes = [float(prep["gmax"].v)]
    clamped_new = 0
    for j in range(case.k + 1):
        got = run(j) if run is not None else None
        moved, row_want = None, None
        if j == 0:
            row_want = dict(cost=cost, gmax=prep["gmax"], radius=R, it=0)
        if j > 0 and done is None:
            s = solve_step(case, st, prep, sc, R)
            att += 1
            rep.fragile += [f"{x} (iteration {j})" for x in s["fragile"]]
            rep.cap = max(rep.cap, s["cap"])
            if not s["model"].v > s["model"].e:
                raise Unsupported(f"{case.name}: model decrease {s['model'].v} (bar {s['model'].e}) at iteration {j}")
            cand = dict(q=_r64(s["qc"]), t=_r64(s["tc"]), P=_r64(s["Pc"]))
            lin_c = linearise(case, cand)
            if lin_c["fragile"].any():
                rep.fragile.append(f"{int(lin_c['fragile'].sum())} fragile observations at the candidate of iteration {j}")
            what, rho, fr = PY.decide(s, cost, lin_c["cost"], opts)
            if what == "accept":
                rep.fragile += [f"{x} (iteration {j})" for x in fr]
                new = cand if got is None else _state(got)
                if _same(new, st):
                    rep.mismatch.append(f"iteration {j}: the yardstick accepts the step (rho {float(rho.v):.4g}), the code kept the point")
                    break
                moved = s
                lin_n = lin_c if _same(new, cand) else linearise(case, new)
                if lin_n["fragile"].any():
                    rep.fragile.append(f"{int(lin_n['fragile'].sum())} fragile observations at the returned state of iteration {j}")
                what2, rho, fr2 = PY.decide(s, cost, lin_n["cost"], opts)
                if what2 != "accept":
                    rep.fragile.append(f"the step of iteration {j} is accepted at the yardstick's candidate, '{what2}' at the returned state")
                    break
                rep.fragile += [f"{x} at the returned state (iteration {j})" for x in fr2]
                clamped_new += int((lin_n["clamped"] & ~ref["clamped"]).sum())
                change = cost - lin_n["cost"]
                R, fr3 = PY.grow(R, rho)
                if j < case.k:
                    rep.fragile += [f"{x} (iteration {j})" for x in fr3]
                dec, ns = 2.0, ns + 1
                prev, st, ref, cost = st, new, lin_n, lin_n["cost"]
                prep = scaled_system(case, st, ref, sc)
                nterm = 4 * int(prep["qvar"].sum()) + 3 * int(prep["tvar"].sum()) + 3 * int(prep["pvar"].sum())
                stepv = np.sqrt(sum(((st[k].astype(LD) - prev[k].astype(LD)) ** 2).sum() for k in ("q", "t", "P")))
                row_want = dict(cost=cost, change=change, gmax=prep["gmax"], step=V(stepv, _step_bar(nterm) * stepv), rho=rho, radius=R, it=j)
                n_rows += 1
                gmaxes.append(float(prep["gmax"].v))
                if PY._inside(prep["gmax"], gtol):
                    rep.fragile.append(f"gradient test after iteration {j}")
                if prep["gmax"].v <= gtol.v:
                    done = (CONVERGENCE, 1)
            else:
                wide = cost_sensitivity(case, cand, lin_c, np.asarray(s["qc"].e + EPS * np.abs(s["qc"].v), np.float64),
                                        np.asarray(s["tc"].e + EPS * np.abs(s["tc"].v), np.float64), np.asarray(s["Pc"].e + EPS * np.abs(s["Pc"].v), np.float64))
                cost_c = V(lin_c["cost"].v, lin_c["cost"].e + wide)
                what2, rho, fr = PY.decide(s, cost, cost_c, opts)
                rep.fragile += [f"{x} (iteration {j})" for x in fr]
                if what2 != what:
                    rep.fragile.append(f"the decision of iteration {j} depends on the candidate's rounding ({what} / {what2})")
                    break
                clamped_new += int((lin_c["clamped"] & ~ref["clamped"]).sum())
                if what == "ptol":
                    done = (CONVERGENCE, 2)
                elif what == "ftol":
                    done = (CONVERGENCE, 3)
                else:
                    R, dec, nu = R * (1.0 / dec), dec * 2, nu + 1
                    nterm = 4 * int(prep["qvar"].sum()) + 3 * int(prep["tvar"].sum()) + 3 * int(prep["pvar"].sum())
                    sn = s["step_norm"]
                    row_want = dict(cost=cost, change=cost - cost_c, gmax=prep["gmax"], step=V(sn.v, sn.e + _step_bar(nterm) * sn.v), rho=rho, radius=R, it=j)
                    n_rows += 1
                    if R.v < LD(PY.MIN_RADIUS):
                        done = (CONVERGENCE, 4)
            decisions.append((what,) if rho is None else (what, float(rho.v), float(rho.e)))
            radii.append(float(R.v))
        if got is None:
            continue
        # ---- the state after max_iterations = j
        term = done if done is not None else (NO_CONVERGENCE, 5)
        want = dict(zip(FIELDS, (ns, nu, att) + term))
        diff = {k: (int(got[k]), v) for k, v in want.items() if int(got[k]) != v}
        if diff:
            rep.mismatch.append(f"max_iterations = {j}: (reported, expected) {diff}")
        if moved is not None:
            for k, key in (("q", "qc"), ("t", "tc"), ("P", "Pc")):
                rep.note(k, Y.ratio(got[k], moved[key]))
        else:
            rep.note("kept", 0.0 if _same(_state(got), st) else np.inf)
        rep.note("initial_cost", Y.ratio(got["initial_cost"], ref0["cost"]))
        rep.note("final_cost", Y.ratio(got["final_cost"], cost))
        rows = got.get("rows")
        if rows is not None:
            if len(rows) != n_rows:
                rep.mismatch.append(f"max_iterations = {j}: {len(rows)} rows, expected {n_rows}")
            elif prev_rows is not None and rows[:len(prev_rows)] != prev_rows:
                rep.mismatch.append(f"max_iterations = {j}: the earlier rows differ from those of max_iterations = {j - 1}")
            elif row_want is not None:
                w = rows[-1]
                if w["it"] != row_want["it"]:
                    rep.mismatch.append(f"max_iterations = {j}: the last row is of iteration {w['it']}")
                for k in ROW_FIELDS:
                    if k in row_want:
                        rep.note("row_" + k, Y.ratio(w[k], row_want[k]))
                    else:
                        rep.note("row_" + k, 0.0 if w[k] == 0.0 else np.inf)          # iteration 0: change, step and rho are 0
            prev_rows = rows
        if diff and any(k in diff for k in ("n_successful", "n_unsuccessful")):
            break                          # the chain of radii is no longer the code's
    tsc = sc[0].v[ref0["active_cam"]][:, 3:6]
    rep.facts = dict(scale_spread=float(tsc.max() / tsc.min()) if tsc.size else 1.0, gmax=gmaxes, decisions=decisions, sequence=tuple(d[0] for d in decisions), exit=done, counts=(ns, nu, att), radii=radii,
                     huber_out=int((ref0["huber_out"] & ~ref0["clamped"]).sum()), clamped_start=int(ref0["clamped"].sum()),
                     clamped_new=clamped_new)
    return rep


# ------------------------------------------------------------------------------------------------ cases
@dataclasses.dataclass
class Case:
    name: str
    family: str
    arr: dict
    k: int = 2
    opts: dict = dataclasses.field(default_factory=lambda: dict(DEFAULTS))
    expect: dict = dataclasses.field(default_factory=dict)           # facts packing() / coverage() must report (test_lba_step_cpu.py)


def _opts(**kw):
    return dict(DEFAULTS, **kw)


def fixed_tracks(n_cams, n_tracks, length, seed):
    """n_tracks tracks of `length` consecutive cameras (cyclic), so that length divides 64 slots evenly into 64 / length tracks."""
    tracks = [np.sort((np.arange(length) + j) % n_cams) for j in range(n_tracks)]
    return H.make_tracks(n_cams, tracks, seed=seed)


def displaced(arr, sigma, rng_seed):
    """The quaternions displaced by sigma N(0, 1) and renormalised (test_gpu_lba_resident.py: the unsuccessful-step seed)."""
    arr = dict(arr)
    q = arr["cam_q"] + sigma * np.random.default_rng(rng_seed).standard_normal(arr["cam_q"].shape)
    arr["cam_q"] = q / np.linalg.norm(q, axis=1, keepdims=True)
    return arr


def ragged10():
    """Tracks of one observation next to tracks of 10 (test_kernel_corners["ragged"])."""
    rng = np.random.default_rng(3)
    return H.make_tracks(10, [list(range(10)) if i % 2 == 0 else [int(rng.integers(10))] for i in range(61)], seed=7)


def consts():
    """cam_const 3 / 1 / 2, a camera without observations, every third point constant (test_kernel_corners["consts"] plus the idle
    camera)."""
    arr = H.make(8, 300, 4, seed=101)
    arr["cam_const"][:] = 0; arr["cam_const"][2] = 3; arr["cam_const"][5] = 1; arr["cam_const"][6] = 2
    arr["point_const"][::3] = 1
    keep = arr["obs_cam"] != 4
    for k in ("obs_cam", "obs_pt", "obs_uv"):
        arr[k] = np.ascontiguousarray(arr[k][keep])
    return arr


def lba_pattern():
    arr = H.make(10, 400, 4, seed=103)
    seen = np.zeros(arr["points"].shape[0], bool); seen[arr["obs_pt"][arr["obs_cam"] == 9]] = True
    arr["point_const"][:] = (~seen).astype(np.uint8)
    return arr


def structure_only():
    arr = H.make(10, 400, 4, seed=103)
    arr["cam_const"][:] = 3
    return arr


def ring(n_cams, n_points, k_obs, seed):
    """Cameras on a ring around the scene (synth mode "unordered").  The forward-motion geometry of H.make's default misses DELTA_CAP
    on the point step at radius 1e4 already (measured: 8.6e-6 on H.make(10, 400, 4, seed=103), 3.3e-6 on H.make(7, 150, 4, seed=13) at
    the first iteration): the bar of y reaches the points through the lever arm |W X| of a low-parallax scene."""
    return H.make(n_cams, n_points, k_obs, seed=seed, mode="unordered", min_tri_angle_deg=2.0)


def gauge(arr):
    """Camera 0 constant, the translation of camera 1 constant: the seven gauge directions are gone, S stays well conditioned at any
    radius, and bar(delta) stays 1e-8 and below where the free problem has 1e-6."""
    arr["cam_const"][0] = 3; arr["cam_const"][1] = 2
    return arr


def shaken(arr, sigma_q, sigma_x, seed):
    """A start far from the optimum: quaternions displaced by sigma_q N(0, 1), points and translations by sigma_x N(0, 1)."""
    arr = displaced(arr, sigma_q, seed)
    rng = np.random.default_rng(seed + 100)
    arr["points"] = arr["points"] + sigma_x * rng.standard_normal(arr["points"].shape)
    arr["cam_t"] = arr["cam_t"] + sigma_x * rng.standard_normal(arr["cam_t"].shape)
    return arr


def behind():
    """Every seventh point five units behind the first camera that observes it (camera frame (0, 0, -5)): clamped residuals."""
    from oracle import ba_oracle as bo
    arr = ring(8, 300, 4, seed=101)
    M = bo.rotation_from_quat(arr["cam_q"])
    for j in range(0, 300, 7):
        c = int(arr["obs_cam"][np.nonzero(arr["obs_pt"] == j)[0][0]])
        arr["points"][j] = M[c].T @ (np.array([0.0, 0.0, -5.0]) - arr["cam_t"][c])
    return arr


def spread():
    """The scene of cameras 0..3 seen through focal lengths 30 times those of the others: unscaled column norms that differ by that
    factor across cameras (every camera its own intrinsics; the observations are re-synthesised by the same factor about the
    principal point)."""
    arr = H.with_models(ring(7, 150, 4, seed=13), seed=5)
    arr["intr_params"] = np.array(arr["intr_params"], copy=True); arr["obs_uv"] = np.array(arr["obs_uv"], copy=True)
    for c in range(4):
        i = int(arr["cam_intr"][c]); model = int(arr["intr_model"][i])
        nf = 1 if model in (0, 2) else 2
        pp = arr["intr_params"][i, nf:nf + 2].copy()
        arr["intr_params"][i, :nf] *= 30.0
        sel = arr["obs_cam"] == c
        arr["obs_uv"][sel] = pp + 30.0 * (arr["obs_uv"][sel] - pp)
    return arr


def _one_cam():
    arr = ring(1, 97, 1, seed=121)
    arr["point_const"][:] = 0
    return arr


NOTOL = dict(function_tolerance=0.0, parameter_tolerance=0.0)


def _build():
    cases = []
    add = lambda *a, **kw: cases.append(Case(*a, **kw))
    # gather geometry: n_items = 6 (nc (nc + 1) / 2 + nc), nslice = 512 / n_items
    add("cams1", "gather", _one_cam(), expect=dict(n_cams=1, nslice=42, head63=True, track_lens_has=(1,)))
    add("cams2", "gather", ring(2, 97, 2, seed=122), expect=dict(n_cams=2, nslice=17))
    add("cams6", "gather", ring(6, 97, 4, seed=126), expect=dict(n_cams=6, nslice=3))
    add("cams7", "gather", ring(7, 97, 4, seed=127), expect=dict(n_cams=7, nslice=2))
    add("cams8", "gather", ring(8, 97, 4, seed=128), expect=dict(n_cams=8, nslice=1, idle_threads=248))
    add("cams10", "gather", ring(10, 400, 4, seed=103), k=3, expect=dict(n_cams=10, n_items=390, nslice=1))
    # chunks of 8 tiles: every track sees the same four cameras, 16 tracks to a tile
    add("tiles_lt1", "chunks", fixed_tracks(4, 9, 4, seed=31), expect=dict(n_tiles=1, dead_lanes=True))
    add("tiles8", "chunks", fixed_tracks(4, 128, 4, seed=32), expect=dict(n_tiles=8, n_chunks=1, dead_lanes=False))
    add("tiles9", "chunks", fixed_tracks(4, 131, 4, seed=33), expect=dict(n_tiles=9, n_chunks=2, dead_lanes=True))
    add("tiles17", "chunks", fixed_tracks(4, 260, 4, seed=34), k=1, expect=dict(n_tiles=17, n_chunks=3))
    # tracks
    # k = 1: at the second iteration (radius 3e4) the rank-2 point blocks of the single-observation tracks bring bar(delta) to 1.1e-6
    add("track1", "tracks", gauge(H.make_tracks(3, [[c % 3] for c in range(40)] + [[0, 1, 2]] * 8, seed=41)), k=1,
        expect=dict(track_lens_has=(1, 3), head63=True))
    add("track2", "tracks", ring(5, 60, 2, seed=42), expect=dict(track_lens_has=(2,)))
    add("track_ncams", "tracks", fixed_tracks(6, 20, 6, seed=43), expect=dict(track_lens_has=(6,), n_cams=6))
    add("ragged", "tracks", ragged10(), expect=dict(track_lens_has=(1, 10), dead_lanes=True))
    # blocks
    add("models", "blocks", H.with_models(ring(10, 400, 4, seed=103), seed=4), expect=dict(models={0, 1, 2, 3, 4}))
    add("consts", "blocks", consts(), expect=dict(cam_const={0, 1, 2, 3}, inactive_cam=True, const_points_min=1))
    add("lba", "blocks", lba_pattern(), k=3, opts=_opts(**LBA_TOL), expect=dict(const_points_min=100))
    add("structure_only", "blocks", structure_only(), expect=dict(cam_const={3}))
    # arithmetic edges
    add("huber", "edges", H.make_tracks(6, [np.sort(np.random.default_rng(50 + j).choice(6, 3, replace=False)) for j in range(80)], seed=51,
                                         outlier_frac=0.2), expect=dict(huber_out_min=10))
    add("behind", "edges", behind(), expect=dict(clamped_start_min=10))
    add("spread", "edges", spread(), expect=dict(scale_spread_min=10.0))
    # decisions.  A rejected step needs a start far from the optimum; the seed of test_kernel_corners["unsuccessful"]
    # (H.make(7, 150, 4, seed=13), quaternions displaced by 0.04) rejects its step only at the fifth iteration, where the radius has
    # grown to 8e5 and bar(delta) to 3e-3 of the step: it misses DELTA_CAP and is replaced by gauge-fixed ring problems.
    add("rejected", "decisions", shaken(gauge(ring(7, 150, 4, seed=13)), 0.2, 2.0, 5), k=4, opts=_opts(**NOTOL), expect=dict(sequence=("accept", "accept", "reject", "reject")))
    add("reject_twice", "decisions", shaken(gauge(ring(4, 40, 2, seed=13)), 0.2, 2.0, 6), k=4, opts=_opts(**NOTOL),
        expect=dict(sequence=("accept", "reject", "reject", "accept")))
    add("reject_first", "decisions", shaken(gauge(ring(4, 40, 2, seed=13)), 0.1, 5.0, 5), k=3, opts=_opts(**NOTOL), expect=dict(sequence=("reject", "reject", "accept")))
    # a rejection, two accepted steps, two rejections: the decrease factor is back at 2 for the fourth step
    add("reject_accept_reject", "decisions", shaken(gauge(ring(4, 40, 2, seed=13)), 0.3, 3.0, 6), k=5, opts=_opts(**NOTOL),
        expect=dict(sequence=("reject", "accept", "accept", "reject", "reject")))
    add("ptol_exit", "decisions", ring(7, 150, 4, seed=12), opts=_opts(initial_radius=1e-9), expect=dict(exit=(CONVERGENCE, 2), counts=(0, 0, 1)))
    add("ftol_exit", "decisions", ring(7, 150, 4, seed=12), k=5, opts=_opts(function_tolerance=1e-2), expect=dict(exit=(CONVERGENCE, 3)))
    add("gtol_exit", "decisions", ring(7, 150, 4, seed=12), k=3, opts=_opts(gradient_tolerance=GTOL_EXIT), expect=dict(exit=(CONVERGENCE, 1), counts_min=1))
    add("gtol_start", "decisions", ring(7, 150, 4, seed=12), k=1, opts=_opts(gradient_tolerance=1e9), expect=dict(exit=(CONVERGENCE, 1), counts=(0, 0, 0)))
    add("max_it_0", "decisions", ring(7, 150, 4, seed=13), k=0, expect=dict(counts=(0, 0, 0)))
    add("radius_1e6", "decisions", gauge(ring(7, 150, 4, seed=13)), k=3, opts=_opts(initial_radius=1e6), expect=dict())
    # one constant point on the optical axis of one camera (pose_step_yardstick.on_axis): two diagonals of H_cc below 1e-6 at both
    # iterations, so the clamp's lower bound is taken where the damping, unlike everywhere else, depends on the scales
    add("on_axis_k2", "decisions", {k: PY.on_axis(0.01, -0.007)[k] for k in H.FIELDS}, k=2, opts=_opts(initial_radius=1.0, **NOTOL),
        expect=dict(sequence=("accept", "accept"), n_cams=1))
    add("radius_small", "decisions", ring(7, 150, 4, seed=13), k=1, opts=_opts(initial_radius=1e-3, **NOTOL), expect=dict(sequence=("accept",)))
    return {c.name: c for c in cases}


# a gradient tolerance between the gradient max-norms of H.make(7, 150, 4, seed=12) at the start and after its first step
GTOL_EXIT = 30.0
FAMILIES = ("gather", "chunks", "tracks", "blocks", "edges", "decisions")
_CASES = {}


def cases():
    if not _CASES:
        _CASES.update(_build())
    return _CASES


def case_names():
    return list(cases())


# ------------------------------------------------------------------------------------------------ coverage
def packing(arr):
    """What the host-side packing makes of a problem (capi.debug_pack, no GPU) and what lba_resident_solve derives from it."""
    from xrsfm_amd import capi
    pk = capi.debug_pack(H.to_product(arr))
    so = np.asarray(pk["slot_obs"]).reshape(-1, 64)
    n_tiles = so.shape[0]
    pt = np.where(so >= 0, np.asarray(arr["obs_pt"])[np.maximum(so, 0)], -1)
    nc = arr["cam_q"].shape[0]
    n_items = 6 * (nc * (nc + 1) // 2 + nc)
    nslice = 512 // n_items
    head63 = dead = False
    for row in pt:
        valid = row >= 0
        head63 |= bool(valid[63] and row[63] != row[62])
    last = pt[-1] >= 0
    dead = bool(last.sum() < 64 and last[:int(last.sum())].all())
    lens = np.bincount(arr["obs_pt"], minlength=arr["points"].shape[0])
    act = np.bincount(arr["obs_cam"], minlength=nc) > 0
    chunk_last = [int(pt[min(8 * c + 7, n_tiles - 1)][pt[min(8 * c + 7, n_tiles - 1)] >= 0][-1]) for c in range(-(-n_tiles // 8))]
    return dict(n_cams=nc, n_tiles=n_tiles, n_chunks=-(-n_tiles // 8), n_items=n_items, nslice=nslice, idle_threads=512 - n_items * nslice,
                head63=head63, dead_lanes=dead, track_lens=set(int(x) for x in lens if x > 0), inactive_cam=bool((~act).any()),
                cam_const=set(int(c) & 3 for c in arr["cam_const"]), const_points=int((np.asarray(arr["point_const"]) != 0).sum()),
                models=set(int(m) for m in np.asarray(arr["intr_model"])[np.asarray(arr["cam_intr"])[arr["obs_cam"]]]),
                tile_of_obs=_tile_of_obs(so, arr["obs_cam"].shape[0]), chunk_last_track=chunk_last)


def _tile_of_obs(so, n_obs):
    out = np.full(n_obs, -1, np.int64)
    t, l = np.nonzero(so >= 0)
    out[so[t, l]] = t
    return out


_COV = {}


def coverage(name):
    """The facts a case exists for: the packing's, and those of the yardstick seated on itself (decision sequence, exit, counters,
    radii, Huber and clamp counts) with its fragile decisions and the largest bar(delta) / max |delta|."""
    if name not in _COV:
        c = cases()[name]
        rep = check_case(c)
        _COV[name] = dict(packing(c.arr), **rep.facts, fragile=list(rep.fragile), cap=rep.cap)
    return _COV[name]


def assert_expected(name, facts):
    """The coverage facts of the case `name` hold in `facts`."""
    c = cases()[name]
    for k, v in c.expect.items():
        base = {"track_lens_has": "track_lens", "has": "sequence", "reject_run": "sequence", "accept_after_rejects": "sequence"}.get(
            k, k[:-4] if k.endswith("_min") else k)
        if base not in facts:
            continue                        # a packing fact asked of a chain report
        if k.endswith("_min"):
            x = facts[k[:-4]]
            assert (sum(x) if isinstance(x, tuple) else x) >= v, (name, k, x)
        elif k == "track_lens_has":
            assert set(v) <= facts["track_lens"], (name, facts["track_lens"])
        elif k == "has":
            assert set(v) <= set(facts["sequence"]), (name, facts["sequence"])
        elif k == "reject_run":
            seq = facts["sequence"]
            assert any(seq[i:i + v] == ("reject",) * v for i in range(len(seq))), (name, seq)
        elif k == "accept_after_rejects":
            seq = facts["sequence"]
            assert any(seq[i:i + 3] == ("reject", "reject", "accept") for i in range(len(seq))), (name, seq)
        elif k == "sequence":
            assert facts["sequence"][:len(v)] == v, (name, facts["sequence"])
        else:
            assert facts[k] == v, (name, k, facts[k], v)


def assert_sound(name, rep):
    """No fragile decision, the cap on bar(delta), and the case's facts, on the chain a code under test was seated on."""
    assert not rep.fragile, (name, rep.fragile)
    assert rep.cap <= DELTA_CAP, (name, rep.cap)
    assert_expected(name, rep.facts)
