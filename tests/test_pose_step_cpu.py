"""The pose-refinement step yardstick without a GPU (tests/pose_step_yardstick.py).

(i) A plain float64 numpy restatement of k_refine_pose's loop (the order of operations of ba_refine.h on lane 0, the oracle's
bo.evaluate and bo.quat_plus for the blocks) plays the code under test for max_iterations = 0..k and is inside every bar on every
case: the bars, derived from operation counts and the Cholesky backward-error bound, are wide enough for a correct float64 loop.
(ii) No case holds a fragile decision, bar(delta) <= 1e-6 max |delta| on every case and iteration, and every case exercises what
it exists for (coverage()).
(iii) The checker FAILS on mutated restatements, each on the smallest case that can show it: a dropped correspondence, two swapped
entries of H, S recomputed at the second iteration, no damping clamp, R instead of R / 2 after a rejection, a back-substitution that
reads the upper triangle."""
import math

import numpy as np
import pytest

from oracle import ba_oracle as bo
from tests import helpers as H
from tests import pose_step_yardstick as PY

_WORST = {}


def restate(case, max_it, mutate=None):
    """k_refine_pose in float64 numpy; returns what xrsfm_ba_refine_pose reports.  mutate: one of the defects of (iii)."""
    arr, o = case.arr, case.opts
    sel = PY.selected(case).copy()
    if mutate == "drop_last":
        sel[np.nonzero(sel)[0][-1]] = False
    m = int(sel.sum())
    pr = H.to_oracle(dict(arr, points=arr["points"][sel], point_const=arr["point_const"][sel], obs_cam=np.zeros(m, np.int32),
                          obs_pt=np.arange(m, dtype=np.int32), obs_uv=arr["obs_uv"][sel]))

    def ev(q, t):
        cost, rt, Fc, _ = bo.evaluate(pr, q[None], t[None], pr.points, o["huber_a"])
        Hu = np.array([(Fc[:, 0, a] * Fc[:, 0, b] + Fc[:, 1, a] * Fc[:, 1, b]).sum() for a, b in PY.PAIRS])
        g = (Fc[:, 0] * rt[:, 0:1] + Fc[:, 1] * rt[:, 1:2]).sum(axis=0)
        if mutate == "swap_offdiag":
            Hu[[1, 2]] = Hu[[2, 1]]
        return cost, Hu, g

    def gradmax(q, g):
        return max(float(np.abs(q - bo.quat_plus(q[None], -g[None, :3])[0]).max()), float(np.abs(g[3:]).max()))

    def scales(Hu):
        return np.array([1.0 / (1.0 + math.sqrt(Hu[PY.IDX[k, k]])) for k in range(6)])

    q, t = np.array(arr["cam_q"][0], np.float64), np.array(arr["cam_t"][0], np.float64)
    cost, Hu, g = ev(q, t)
    initial_cost = cost
    S = scales(Hu)
    radius, decrease = float(o["initial_radius"]), 2.0
    it = n_succ = n_unsucc = attempted = invalid = 0
    term, reason = None, None
    if gradmax(q, g) <= PY.GTOL:
        term, reason = PY.CONVERGENCE, 1
    while term is None:
        if it >= max_it:
            term, reason = PY.NO_CONVERGENCE, 5
            break
        it += 1; attempted += 1
        if mutate == "recompute_scale" and it == 2:
            S = scales(Hu)
        A = np.zeros((6, 6)); b = np.zeros(6)
        for a in range(6):
            for c in range(a, 6):
                A[a, c] = A[c, a] = Hu[PY.IDX[a, c]] * S[a] * S[c]
            b[a] = -S[a] * g[a]
        for a in range(6):
            A[a, a] += (A[a, a] if mutate == "no_clamp" else min(max(A[a, a], 1e-6), 1e32)) / radius
        ok = True
        for j in range(6):
            d = A[j, j]
            for k in range(j):
                d -= A[j, k] * A[j, k]
            if not d > 0.0:
                ok = False
                break
            d = math.sqrt(d)
            A[j, j] = d
            for i in range(j + 1, 6):
                v = A[i, j]
                for k in range(j):
                    v -= A[i, k] * A[j, k]
                A[i, j] = v / d
        model = -1.0
        if ok:
            for i in range(6):
                v = b[i]
                for k in range(i):
                    v -= A[i, k] * b[k]
                b[i] = v / A[i, i]
            for i in range(5, -1, -1):
                v = b[i]
                for k in range(i + 1, 6):
                    v -= (A[i, k] if mutate == "upper_triangle" else A[k, i]) * b[k]
                b[i] = v / A[i, i]
            delta = S * b
            gd = dHd = 0.0
            for a in range(6):
                gd += g[a] * delta[a]
                hv = 0.0
                for c in range(6):
                    hv += Hu[PY.IDX[a, c]] * delta[c]
                dHd += delta[a] * hv
            model = -(gd + 0.5 * dHd)
        if not model > 0.0 or not math.isfinite(model):          # (no case proposes an invalid step; a mutant may)
            n_unsucc += 1; invalid += 1
            if invalid >= 5:
                term, reason = 2, 6
            else:
                radius /= decrease; decrease *= 2.0
            continue
        invalid = 0
        qc = bo.quat_plus(q[None], delta[None, :3])[0]
        tc = t + delta[3:]
        cost_c, Hc, gc = ev(qc, tc)
        xn2 = st2 = 0.0
        for k in range(4):
            xn2 += q[k] * q[k]; st2 += (qc[k] - q[k]) ** 2
        for k in range(3):
            xn2 += t[k] * t[k]; st2 += (tc[k] - t[k]) ** 2
        step_norm, xnorm, change = math.sqrt(st2), math.sqrt(xn2), cost - cost_c
        ptol, ftol = o["parameter_tolerance"], o["function_tolerance"]
        if step_norm <= ptol * (xnorm + ptol):
            term, reason = PY.CONVERGENCE, 2
        elif abs(change) <= ftol * cost:
            term, reason = PY.CONVERGENCE, 3
        else:
            rel = change / model
            if rel > 1e-3:
                q, t, cost, Hu, g = qc, tc, cost_c, Hc, gc
                radius = min(1e16, radius / max(1.0 / 3.0, 1.0 - (2.0 * rel - 1.0) ** 3))
                decrease = 2.0
                n_succ += 1
                if gradmax(q, g) <= PY.GTOL:
                    term, reason = PY.CONVERGENCE, 1
            else:
                radius /= 1.0 if mutate == "no_shrink" else decrease
                decrease *= 2.0
                n_unsucc += 1
                if radius < 1e-32:
                    term, reason = PY.CONVERGENCE, 4
    return dict(q=q, t=t, initial_cost=initial_cost, final_cost=cost, n_successful=n_succ, n_unsuccessful=n_unsucc,
                lm_steps_attempted=attempted, termination=term, termination_reason=reason)


@pytest.mark.parametrize("name", PY.case_names())
def test_float64_restatement_is_inside_every_bar(name):
    case = PY.cases()[name]
    rep = PY.check_case(case, lambda k: restate(case, k))
    print(f"POSESTEP64 case={name} worst={rep.worst:.3g} cap={rep.cap:.2g} " + " ".join(f"{k}={v:.3g}" for k, v in rep.ratios.items())
          + f" facts={rep.facts}")
    PY.assert_sound(name, rep)
    assert rep.ok, (name, rep.mismatch, rep.ratios)
    fam = _WORST.setdefault(case.family, {})
    for k, v in rep.ratios.items():
        fam[k] = max(fam.get(k, 0.0), v)
    print(f"POSESTEP64 family {case.family} so far: " + " ".join(f"{k}={v:.3g}" for k, v in fam.items()))


@pytest.mark.parametrize("name", [n for n in PY.case_names() if PY.cases()[n].expect])
def test_case_exercises_what_it_exists_for(name):
    """coverage(): the yardstick seated on itself, independent of any code under test."""
    cov = PY.coverage(name)
    assert not cov["fragile"] and cov["cap"] <= PY.DELTA_CAP, (name, cov)
    PY.assert_expected(name, cov)


def test_catalogue():
    cs = PY.cases()
    sizes = [c for c in cs.values() if c.family == "sizes"]
    assert {(c.arr["points"].shape[0], c.model, c.opts["initial_radius"]) for c in sizes} >= {(n, m, R) for n in PY.SIZES for m in range(5) for R in PY.RADII}
    assert any(c.mask is not None for c in sizes)
    assert any(c.expect.get("clamp_taken") and c.arr["points"].shape[0] <= 2 for c in sizes)
    assert {c.opts["initial_radius"] for c in cs.values() if c.family == "radius"} == set(PY.SPECTRUM)
    assert sum(c.family == "rejected" and c.arr["points"].shape[0] >= 65 for c in cs.values()) >= 1
    assert sum(c.family == "clamped" for c in cs.values()) >= 2
    assert {c.k for c in cs.values() if c.family in ("huber", "rejected", "plain") and c.name != "huber_inner_n65"} == {3}
    assert set(c.family for c in cs.values()) == set(PY.FAMILIES)


def test_parameter_tolerance_exit_keeps_the_point():
    case = PY.cases()["radius_1e-12"]
    got = restate(case, 1)
    assert got["termination_reason"] == 2 and got["final_cost"] == got["initial_cost"]
    assert np.array_equal(got["q"], case.arr["cam_q"][0]) and np.array_equal(got["t"], case.arr["cam_t"][0])


def test_all_clamped_cost():
    """Every residual is (12, 12): s = 288 on Huber's outer branch, cost = n rho(288) / 2, inside the cost bar."""
    case = PY.cases()["all_clamped"]
    a = np.longdouble(np.float64(case.opts["huber_a"]))
    want = 65 * (2 * a * np.sqrt(np.longdouble(288)) - np.longdouble(np.float64(case.opts["huber_a"]) ** 2)) / 2
    lin = PY._initial(case)[0]
    assert abs(lin["cost"].v - want) <= lin["cost"].e and float((np.abs(lin["g"].v)).max()) == 0.0


MUTANTS = (("drop_last", "n65_m2_R10000"), ("drop_last", "n257_m2_R10000"), ("swap_offdiag", "n3_m2_R10000"), ("recompute_scale", "on_axis_near_k2"),
           ("no_clamp", "on_axis_R10000"), ("no_shrink", "rejected_n3_R2e4"), ("upper_triangle", "n3_m2_R10000"))


@pytest.mark.parametrize("mutate,name", MUTANTS)
def test_checker_fails_on_a_mutated_restatement(mutate, name):
    case = PY.cases()[name]
    good = PY.check_case(case, lambda k: restate(case, k))
    assert good.ok and not good.fragile, (name, good.mismatch, good.ratios, good.fragile)
    bad = PY.check_case(case, lambda k: restate(case, k, mutate))
    print(f"POSESTEP64 mutant={mutate} case={name} worst={bad.worst:.3g} mismatch={bad.mismatch}")
    assert not bad.ok, (mutate, name, bad.ratios)
