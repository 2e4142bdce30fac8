"""The resident-solver step yardstick without a GPU (tests/lba_step_yardstick.py).

(i)   The conditions the yardstick has to meet by itself, from the self-seated chain and the packing (capi.debug_pack) alone: no
      FRAGILE decision in any case at any iteration, bar(delta) <= 1e-6 max |delta| over the camera step and over the point step, and
      every case still exercises what it exists for (the coverage table this module prints).
(ii)  A plain float64 numpy restatement of lba_resident_solve (restate(): the oracle's bo.evaluate and bo.quat_plus for the blocks,
      then the kernel's own order: point factor C, V = W C, z = C^T g_p, S and b from V, right-looking Cholesky with reciprocal
      pivots, the two triangular solves, back-substitution through C, candidate, model decrease, the controller and its rows) plays
      the code under test for max_iterations = 0..k and is inside every bar on every case.  It shares no code with the yardstick's
      long-double solve.
(iii) Hand-checkable systems: the yardstick's y and u against a direct dense solve of the un-reduced damped normal equations
      (J^T J + D) x = J^T r, written out from the same scaled blocks, on one camera with one constant point (S has no Schur term: it
      is F^T F + D, 6x6), two cameras with one track (S is 12x12, one off-diagonal block) and a four-camera tile.
(iv)  The checker FAILS on fifteen mutated restatements (MUTANTS: the defect, and the case that catches it).

Time of a full case check with the float64 restatement as the runner (its cost is the yardstick's), one CPU core, seconds
(test_float64_restatement_is_inside_every_bar prints each): 0.04 (max_it_0) to 1.1 (lba: 10 cameras, 1600 observations, k = 3) and
1.0 (rejected, k = 4: two kept points with the central differences of their widened cost); every other case under 0.9.  No depth had
to be cut for time; track1 (k = 1) and the absence of forward-motion scenes are cuts for DELTA_CAP (lba_step_yardstick.py).
"""
import math
import time

import numpy as np
import pytest

from oracle import ba_oracle as bo
from tests import helpers as H
from tests import lba_step_yardstick as LY
from tests import pose_step_yardstick as PY

_WORST = {}


def _point_factor(Hpp, d):
    """C (upper) with C C^T = (Hpp + diag d)^-1: point_factor() of ba_math.h with a plain 1 / sqrt."""
    h00, h11, h22 = Hpp[:, 0, 0] + d[:, 0], Hpp[:, 1, 1] + d[:, 1], Hpp[:, 2, 2] + d[:, 2]
    r0 = 1.0 / np.sqrt(h00)
    l10 = Hpp[:, 1, 0] * r0; l20 = Hpp[:, 2, 0] * r0
    r1 = 1.0 / np.sqrt(np.maximum(h11 - l10 * l10, 1e-300))
    l21 = (Hpp[:, 2, 1] - l20 * l10) * r1
    r2 = 1.0 / np.sqrt(np.maximum(h22 - l20 * l20 - l21 * l21, 1e-300))
    m10 = -l10 * r0 * r1
    m21 = -l21 * r1 * r2
    m20 = -(l20 * r0 + l21 * m10) * r2
    C = np.zeros(Hpp.shape)
    C[:, 0, 0], C[:, 0, 1], C[:, 0, 2], C[:, 1, 1], C[:, 1, 2], C[:, 2, 2] = r0, m10, m20, r1, m21, r2
    return C


def restate(case, max_it, mutate=None):
    """lba_resident_solve in float64 numpy; returns what a run reports plus the iteration rows.  mutate: one of MUTANTS."""
    arr, o = case.arr, case.opts
    pr = H.to_oracle(arr)
    if mutate == "move_const":           # the constant flag of one observed point is ignored
        j = int(np.nonzero((pr.point_const != 0) & (np.bincount(pr.obs_pt, minlength=pr.points.shape[0]) > 0))[0][0])
        pr.point_const[j] = 0
    ci, pi = pr.obs_cam.astype(np.int64), pr.obs_pt.astype(np.int64)
    Nc, Np, No = pr.cam_q.shape[0], pr.points.shape[0], ci.shape[0]
    a, ptol, ftol, gtol = o["huber_a"], o["parameter_tolerance"], o["function_tolerance"], o["gradient_tolerance"]
    act = np.bincount(ci, minlength=Nc) > 0
    qvar, tvar = act & ((pr.cam_const & 1) == 0), act & ((pr.cam_const & 2) == 0)
    pvar = (np.bincount(pi, minlength=Np) > 0) & (pr.point_const == 0)
    by_pt = [np.nonzero(pi == j)[0] for j in range(Np)]
    gathered = np.ones(No, bool)         # observations the gather of S, H_cc, g_c, b reaches
    hcc_skip = np.zeros(No, bool)
    if mutate in ("skip_chunk2", "hcc_skip_last"):
        pk = LY.packing(arr)
        if mutate == "skip_chunk2":
            gathered = ~((pk["tile_of_obs"] >= 8) & (pk["tile_of_obs"] < 16))
        else:
            hcc_skip = pi == pk["chunk_last_track"][0]
    q, t, P = pr.cam_q.copy(), pr.cam_t.copy(), pr.points.copy()

    def scales(Fc, Ep):
        return (1.0 / (1.0 + np.sqrt(bo._scatter_add(Nc, ci, np.sum(Fc * Fc, axis=1)))),
                1.0 / (1.0 + np.sqrt(bo._scatter_add(Np, pi, np.sum(Ep * Ep, axis=1)))))

    def linearise(q_, t_, P_, sc):
        cost, rt, Fc, Ep = bo.evaluate(pr, q_, t_, P_, a)
        if sc is None:
            sc = scales(Fc, Ep)
        Fs, Es = Fc * sc[0][ci][:, None, :], Ep * sc[1][pi][:, None, :]
        g = gathered[:, None, None]
        lin = dict(cost=cost, rt=rt, Fs=Fs, Es=Es,
                   Hpp=bo._scatter_add(Np, pi, np.einsum("nki,nkj->nij", Es, Es)), gp=bo._scatter_add(Np, pi, np.einsum("nki,nk->ni", Es, rt)),
                   Hcc=bo._scatter_add(Nc, ci, np.einsum("nki,nkj->nij", Fs, Fs) * (g & ~hcc_skip[:, None, None])),
                   gc=bo._scatter_add(Nc, ci, np.einsum("nki,nk->ni", Fs, rt) * gathered[:, None]), W=np.einsum("nki,nkj->nij", Fs, Es))
        gcu, gpu = lin["gc"] / sc[0], lin["gp"] / sc[1]
        m = float(np.abs(gpu[pvar]).max()) if pvar.any() else 0.0
        if qvar.any():
            m = max(m, float(np.abs(q_[qvar] - bo.quat_plus(q_[qvar], -gcu[qvar, 0:3])).max()))
        if tvar.any():
            m = max(m, float(np.abs(gcu[tvar, 3:6]).max()))
        lin["gmax"] = m
        lin["xn2_pts"] = float((P_[pvar] ** 2).sum())
        return lin, sc

    lin, sc = linearise(q, t, P, None)
    cost = initial_cost = lin["cost"]
    radius, decrease = float(o["initial_radius"]), 2.0
    it = n_succ = n_unsucc = attempted = invalid = 0
    term = reason = None
    rows = [dict(cost=cost, change=0.0, gmax=lin["gmax"], step=0.0, rho=0.0, radius=radius, it=0)]
    if lin["gmax"] <= gtol:
        term, reason = LY.CONVERGENCE, 1
    n = 6 * Nc
    while term is None:
        if it >= max_it:
            term, reason = LY.NO_CONVERGENCE, 5
            break
        it += 1; attempted += 1
        clip = (lambda x: x) if mutate == "no_clamp" else (lambda x: np.minimum(np.maximum(x, 1e-6), 1e32))
        Hpp, Hcc, gp, gc, W, Fs, Es, rt = (lin[k] for k in ("Hpp", "Hcc", "gp", "gc", "W", "Fs", "Es", "rt"))
        dp = clip(np.einsum("nii->ni", Hpp)) / radius
        if mutate == "no_point_damping":
            dp = np.maximum(dp * 0.0, 1e-300)
        C = _point_factor(Hpp, dp)
        Vo = np.matmul(W, C[pi])                                          # V = (F^T E) C
        z = np.einsum("nji,nj->ni", C, gp)                                # z = C^T g_p
        S = np.zeros((n, n)); b = np.zeros(n)
        for c in range(Nc):
            S[6 * c:6 * c + 6, 6 * c:6 * c + 6] = Hcc[c] + np.diag(clip(np.diag(Hcc[c])) / radius)
            b[6 * c:6 * c + 6] = gc[c]
        dropped = False
        for j in range(Np):
            obs = by_pt[j][gathered[by_pt[j]]]
            for x in obs:
                cx = 6 * ci[x]
                if mutate != "b_no_vz":
                    b[cx:cx + 6] -= Vo[x] @ z[j]
                for y_ in obs:
                    if mutate == "drop_shared" and not dropped and len(obs) > 1 and x == obs[0] and y_ == obs[1]:
                        continue
                    if mutate == "drop_shared" and not dropped and len(obs) > 1 and x == obs[1] and y_ == obs[0]:
                        dropped = True
                        continue
                    S[cx:cx + 6, 6 * ci[y_]:6 * ci[y_] + 6] -= Vo[x] @ Vo[y_].T
        if mutate == "transpose_block" and Nc > 1:
            blk = S[0:6, 6:12].copy()
            S[0:6, 6:12], S[6:12, 0:6] = blk.T, blk
        # right-looking Cholesky with reciprocal pivots, then the two triangular solves (lba_factor_solve)
        ok = True
        L = np.zeros((n, n)); dinv = np.zeros(n)
        for j in range(n):
            s = S[j, j]
            if not s > 0.0:
                ok = False
                break
            inv = 1.0 / math.sqrt(s)
            col = S[j + 1:, j] * inv
            S[j + 1:, j + 1:] -= np.tril(np.outer(col, col))
            L[j + 1:, j] = col
            dinv[j] = inv
        model = -1.0
        if ok:
            y = b.copy()
            for j in range(n):
                y[j] *= dinv[j]
                y[j + 1:] -= L[j + 1:, j] * y[j]
            for j in range(n - 1, -1, -1):
                y[j] *= dinv[j]
                y[:j] -= L[j, :j] * y[j]
            ok = bool(np.isfinite(y).all())
        if ok:
            y = y.reshape(Nc, 6)
            v = np.einsum("nki,ni->nk", Fs, y[ci])
            w = bo._scatter_add(Np, pi, np.einsum("nki,nk->ni", Es, v))
            u = np.einsum("nij,nj->ni", C, np.einsum("nji,nj->ni", C, gp - w))
            dq, dt = -y[:, 0:3] * sc[0][:, 0:3], -y[:, 3:6] * sc[0][:, 3:6]
            qc, tc, Pc = q.copy(), t.copy(), P.copy()
            if qvar.any():
                if mutate == "additive_quat":
                    qc[qvar, 0:3] = q[qvar, 0:3] + 0.5 * dq[qvar]
                else:
                    qc[qvar] = bo.quat_plus(q[qvar], dq[qvar])
            tc[tvar] = t[tvar] + dt[tvar]
            Pc[pvar] = P[pvar] + (-u[pvar] if mutate == "no_sp" else -u[pvar] * sc[1][pvar])
            m = v + np.einsum("nki,ni->nk", Es, u[pi])
            model = float(np.sum(m * (rt - 0.5 * m)))
        if not model > 0.0 or not math.isfinite(model):          # (no case proposes an invalid step; a mutant may)
            n_unsucc += 1; invalid += 1
            rows.append(dict(cost=cost, change=0.0, gmax=lin["gmax"], step=0.0, rho=0.0, radius=radius, it=it))
            if invalid >= 5:
                term, reason = 2, 6
            else:
                radius /= decrease; decrease *= 2.0
            continue
        invalid = 0
        cost_c = bo.evaluate(pr, q if mutate == "cost_old_cams" else qc, t if mutate == "cost_old_cams" else tc, Pc, a, want_jac=False)
        cost_c = cost_c[0] if isinstance(cost_c, tuple) else cost_c
        st2 = float(((qc - q)[qvar] ** 2).sum() + ((tc - t)[tvar] ** 2).sum()) + (0.0 if mutate == "step_no_points" else float(((Pc - P)[pvar] ** 2).sum()))
        xn2 = float((q[qvar] ** 2).sum() + (t[tvar] ** 2).sum()) + lin["xn2_pts"]
        step_norm, xnorm, change = math.sqrt(st2), math.sqrt(xn2), cost - cost_c
        if step_norm <= ptol * (xnorm + ptol):
            term, reason = LY.CONVERGENCE, 2
        elif abs(change) <= ftol * cost:
            term, reason = LY.CONVERGENCE, 3
        else:
            rel = change / model
            if rel > 1e-3:
                q, t, P = qc, tc, Pc
                lin, sc = linearise(q, t, P, None if mutate == "rescale" else sc)
                cost = lin["cost"]
                x = 2.0 * rel - 1.0
                radius = min(1e16, radius / max(1.0 / 3.0, 1.0 - (x * x if mutate == "grow_square" else x * x * x)))
                if mutate != "no_dec_reset":
                    decrease = 2.0
                n_succ += 1
                rows.append(dict(cost=cost, change=change, gmax=lin["gmax"], step=step_norm, rho=rel, radius=radius, it=it))
                if lin["gmax"] <= gtol:
                    term, reason = LY.CONVERGENCE, 1
            else:
                radius /= decrease; decrease *= 2.0
                n_unsucc += 1
                rows.append(dict(cost=cost, change=change, gmax=lin["gmax"], step=step_norm, rho=rel, radius=radius, it=it))
                if radius < 1e-32:
                    term, reason = LY.CONVERGENCE, 4
    return dict(q=q, t=t, P=P, initial_cost=initial_cost, final_cost=cost, n_successful=n_succ, n_unsuccessful=n_unsucc,
                lm_steps_attempted=attempted, termination=term, termination_reason=reason, rows=rows)


# ------------------------------------------------------------------------------------------------ (i) the yardstick by itself
@pytest.mark.parametrize("name", LY.case_names())
def test_case_is_sound_and_exercises_what_it_exists_for(name):
    """coverage(): the packing and the yardstick seated on itself, independent of any code under test."""
    cov = LY.coverage(name)
    keys = ("n_cams", "n_tiles", "n_chunks", "n_items", "nslice", "idle_threads", "head63", "dead_lanes", "track_lens", "inactive_cam", "cam_const",
            "const_points", "models", "huber_out", "clamped_start", "clamped_new", "sequence", "exit", "counts")
    print(f"LBASTEP coverage case={name} cap={cov['cap']:.2g} radii={[f'{r:.3g}' for r in cov['radii']]} " + " ".join(f"{k}={cov[k]}" for k in keys))
    assert not cov["fragile"], (name, cov["fragile"])
    assert cov["cap"] <= LY.DELTA_CAP, (name, cov["cap"])
    LY.assert_expected(name, cov)


def test_catalogue():
    cov = {n: LY.coverage(n) for n in LY.case_names()}
    cs = LY.cases()
    assert {c["n_cams"] for c in cov.values()} >= {1, 2, 6, 7, 8, 10}
    assert {c["nslice"] for c in cov.values()} >= {42, 17, 3, 2, 1}
    assert any(c["n_cams"] == 10 and c["n_items"] == 390 for c in cov.values())
    assert {c["n_tiles"] for c in cov.values()} >= {1, 8, 9, 17} and {c["n_chunks"] for c in cov.values()} >= {1, 2, 3}
    lens = set().union(*(c["track_lens"] for c in cov.values()))
    assert lens >= {1, 2, 10} and any(c["n_cams"] in c["track_lens"] for c in cov.values())
    assert any(c["track_lens"] >= {1, 10} for c in cov.values())
    assert any(c["head63"] for c in cov.values()) and any(c["dead_lanes"] for c in cov.values())
    assert set().union(*(c["models"] for c in cov.values())) >= {0, 1, 2, 3, 4}
    assert set().union(*(c["cam_const"] for c in cov.values())) >= {0, 1, 2, 3}
    assert any(c["inactive_cam"] for c in cov.values()) and any(c["cam_const"] == {3} for c in cov.values())
    assert any(c["const_points"] > 0 for c in cov.values())
    assert any(c["huber_out"] >= 10 for c in cov.values()) and any(c["clamped_start"] >= 10 for c in cov.values())
    seqs = [c["sequence"] for c in cov.values()]
    assert any("reject" in s for s in seqs) and any(s[i:i + 3] == ("reject", "reject", "accept") for s in seqs for i in range(len(s)))
    assert {c["exit"] for c in cov.values()} >= {None, (0, 1), (0, 2), (0, 3)}
    assert any(c.k == 0 for c in cs.values()) and max(c.k for c in cs.values()) <= 5
    assert {c.opts["initial_radius"] for c in cs.values()} >= {1e4, 1e6, 1e-3}
    assert set(c.family for c in cs.values()) == set(LY.FAMILIES)


# ------------------------------------------------------------------------------------------------ (ii) the float64 restatement
@pytest.mark.parametrize("name", LY.case_names())
def test_float64_restatement_is_inside_every_bar(name):
    case = LY.cases()[name]
    t0 = time.perf_counter()
    rep = LY.check_case(case, lambda k: restate(case, k))
    dt = time.perf_counter() - t0
    print(f"LBASTEP64 case={name} family={case.family} time={dt:.2f}s worst={rep.worst:.3g} cap={rep.cap:.2g} "
          + " ".join(f"{k}={v:.3g}" for k, v in rep.ratios.items()) + f" sequence={rep.facts['sequence']}")
    LY.assert_sound(name, rep)
    assert rep.ok, (name, rep.mismatch, rep.ratios)
    fam = _WORST.setdefault(case.family, {})
    for k, v in rep.ratios.items():
        fam[k] = max(fam.get(k, 0.0), v)
    print(f"LBASTEP64 family {case.family} so far: " + " ".join(f"{k}={v:.3g}" for k, v in fam.items()))


# ------------------------------------------------------------------------------------------------ (iii) hand-checkable systems
def _direct(case):
    """(y, u) of the yardstick's first step and of a dense solve of (J^T J + D) x = J^T r, J = [F | E] from the same scaled blocks."""
    st, ref, sc, prep = LY._initial(case)
    R = float(case.opts["initial_radius"])
    s = LY.solve_step(case, st, prep, sc, LY.V(np.float64(R)))
    Nc, Np, ci, pi = prep["Nc"], prep["Np"], prep["ci"], prep["pi"]
    F, E, r = (np.asarray(x, np.float64) for x in (prep["F"], prep["E"], prep["r"].v))
    J = np.zeros((2 * ci.shape[0], 6 * Nc + 3 * Np))
    for o in range(ci.shape[0]):
        J[2 * o:2 * o + 2, 6 * ci[o]:6 * ci[o] + 6] = F[o]
        J[2 * o:2 * o + 2, 6 * Nc + 3 * pi[o]:6 * Nc + 3 * pi[o] + 3] = E[o]
    Hf = J.T @ J
    Hf += np.diag(np.clip(np.diag(Hf), 1e-6, 1e32) / R)
    x = np.linalg.solve(Hf, J.T @ r.reshape(-1))
    pvar = prep["pvar"]
    u_y = np.asarray(-s["dpt"].v / sc[1].v, np.float64)
    return np.asarray(s["y"].v, np.float64), x[:6 * Nc].reshape(Nc, 6), u_y[pvar], x[6 * Nc:].reshape(Np, 3)[pvar]


def _one_track(n_cams):
    arr = H.make_tracks(max(n_cams, 2), [list(range(n_cams))], seed=3, outlier_frac=0.0)
    if n_cams == 1:
        for k in ("cam_q", "cam_t", "cam_const", "cam_intr"):
            arr[k] = np.ascontiguousarray(arr[k][:1])
    return arr


def test_one_camera_one_constant_point_has_no_schur_term():
    """S = F^T F + clip(diag F^T F) / R and b = F^T r: the 6x6 system written out."""
    arr = _one_track(1)
    arr["point_const"][:] = 1
    case = LY.Case("hand_1x1", "hand", arr, k=1)
    st, ref, sc, prep = LY._initial(case)
    F, r = np.asarray(prep["F"], np.float64)[0], np.asarray(prep["r"].v, np.float64)[0]
    from tests import schur_yardstick as SY
    S, Se, b, be = LY.dense(SY.system(prep, 1e4), 1)
    want = F.T @ F
    want += np.diag(np.clip(np.diag(want), 1e-6, 1e32) / 1e4)
    assert np.allclose(np.asarray(S, np.float64), want, rtol=1e-13, atol=0) and np.allclose(np.asarray(b, np.float64), F.T @ r, rtol=1e-13, atol=0)
    assert (np.asarray(prep["E"], np.float64) == 0).all()
    y, y_direct, _, _ = _direct(case)
    assert np.allclose(y, y_direct, rtol=1e-7, atol=0), (y, y_direct)


@pytest.mark.parametrize("n_cams,n_tracks", [(2, 1), (4, 9)])
def test_step_equals_the_unreduced_normal_equations(n_cams, n_tracks):
    """Two cameras and one track (12x12 S, one off-diagonal block), and a four-camera tile: y and u of the yardstick against the
    dense solve of the whole damped system, cameras and points together."""
    arr = _one_track(2) if n_tracks == 1 else LY.fixed_tracks(4, 9, 4, seed=31)
    case = LY.Case(f"hand_{n_cams}x{n_tracks}", "hand", LY.gauge(arr), k=1)
    y, y_direct, u, u_direct = _direct(case)
    assert np.abs(y - y_direct).max() <= 1e-7 * np.abs(y_direct).max(), (y, y_direct)
    assert np.abs(u - u_direct).max() <= 1e-7 * np.abs(u_direct).max(), (u, u_direct)


def test_gamma_is_the_stated_operation_count():
    assert float(LY.GAMMA(60) / LY.EPS) == 3 * 60 + 1 + 60 * 5 == 481 and float(LY.GAMMA(6) / LY.EPS) == 49


# ------------------------------------------------------------------------------------------------ (iv) mutations
# (defect, the case that catches it)
MUTANTS = (("rescale", "on_axis_k2"),             # 1  scales recomputed at every accepted point
           ("no_clamp", "structure_only"),        # 2  the damping clamp skipped
           ("no_point_damping", "track1"),        # 3  point damping omitted
           ("drop_shared", "cams2"),              # 4  one shared track dropped from one off-diagonal block
           ("hcc_skip_last", "tiles9"),           # 5  the last track of a chunk left out of H_cc
           ("skip_chunk2", "tiles9"),             # 6  tiles of the second chunk not accumulated
           ("transpose_block", "cams2"),          # 7  an off-diagonal block transposed
           ("b_no_vz", "cams6"),                  # 8  b without the V z term
           ("no_sp", "cams6"),                    # 9  candidate points without s_p
           ("additive_quat", "cams6"),            # 10 the quaternion updated additively instead of by Plus
           ("step_no_points", "reject_first"),    # 11 the step norm without its point part
           ("grow_square", "rejected"),             # 12 the radius grown with a square instead of the cube
           ("no_dec_reset", "reject_accept_reject"),     # 13 the decrease factor not reset after a success
           ("cost_old_cams", "cams6"),            # 14 cost_c evaluated with the old cameras
           ("move_const", "consts"))              # 15 a constant block moved


@pytest.mark.parametrize("mutate,name", MUTANTS)
def test_checker_fails_on_a_mutated_restatement(mutate, name):
    case = LY.cases()[name]
    good = LY.check_case(case, lambda k: restate(case, k))
    assert good.ok and not good.fragile, (name, good.mismatch, good.ratios, good.fragile)
    bad = LY.check_case(case, lambda k: restate(case, k, mutate))
    over = {k: v for k, v in bad.ratios.items() if not v <= 1.0}
    print(f"LBASTEP64 mutant={mutate} caught by case={name}: worst={bad.worst:.3g} over={over} mismatch={bad.mismatch}")
    assert not bad.ok, (mutate, name, bad.ratios)
