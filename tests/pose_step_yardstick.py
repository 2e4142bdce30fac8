"""Yardstick, cases and checker of the pose-refinement step tests (tests/test_pose_step_cpu.py, tests/test_gpu_pose_step.py).

k_refine_pose (xrsfm_amd/csrc/ba_refine.h) runs a whole Levenberg-Marquardt loop in one workgroup.  xrsfm_ba_refine_pose with
max_iterations = k returns the state after exactly k attempted steps, so every step is visible through the public call.  The
yardstick restates one step in np.longdouble on the (value, bar) arithmetic of tests/lin_yardstick.py (its V, reference, seg_sum,
_quat_plus_diff and ratio are used, not copied); it never calls the library.

One step from the float64 pose (q, t), the scales S, the radius R and the options:

  normal equations   F (unscaled 2x6 camera block) and the robustified residual r of lin_yardstick.reference at (q, t), restricted
                     to the selected correspondences: H = sum F^T F (21 entries), g = sum F^T r through seg_sum (the bar of a sum
                     over L terms), cost = 1/2 sum rho.
  scaling, damping   S_k = 1 / (1 + sqrt(H_kk)) from the FIRST linearisation only;  A = S H S + diag(clamp(diag(S H S), 1e-6, 1e32)) / R,
                     b = -S g.  The clamp is decided on the long-double value; a diagonal within its own bar of a bound is FRAGILE.
  solve              long-double Cholesky A = L L^T and y = A^-1 b.  Forward bar |dy| <= |A^-1| (bar(A) |y| + bar(b) + gamma |L| |L^T| |y|),
                     gamma = (3 * 6 + 1) eps: the backward error of a Cholesky solve of order 6 (Higham, Accuracy and Stability of
                     Numerical Algorithms, Thm 10.4), so it holds for any float64 Cholesky solve (the kernel's on lane 0, the
                     engine's tile factorisation).  It is derived, not tuned.
  step, model        delta = S y;  model = -(g . delta + 1/2 delta^T H delta);  candidate q_c = Plus(q, delta[0:3]), t_c = t + delta[3:6],
                     each with its propagated bar.
  decisions          in the order of ba_refine.h / ba_trust_region.h: model > 0; the parameter- and function-tolerance exits (both
                     keep the point: reasons 2 and 3); rho = (cost - cost_c) / model > 1e-3; on success the radius grows by
                     1 / max(1/3, 1 - (2 rho - 1)^3), capped at 1e16, and the gradient test |x - Plus(x, -g)|_inf <= 1e-10 follows; on
                     failure the radius shrinks by the decrease factor, which doubles.  A decision whose margin lies inside its
                     bar is FRAGILE (the two switches of the radius update only when a later step of the case uses the radius).

Seating.  The expected state after k iterations is built iteration by iteration: iteration j starts from the float64 pose the code
under test returned for max_iterations = j - 1, which is an exact input, so no bar accumulates across iterations.  S comes from
the yardstick's linearisation at the initial pose; the radius and the decrease factor from the yardstick's own chain of rho values
(carried as V).  The step is first judged with the cost at the yardstick's own candidate (rounded to float64).  If that accepts,
the code under test must have moved; its pose is compared with the candidate bars, and cost_c, rho and the new radius are then
taken at the pose it returned (the decision must come out the same).  If the point is kept (rejection, tolerance exit) the
candidate of the code under test is not visible: the decision must then hold with cost_c widened by |grad cost| . bar(candidate),
the gradient over the seven pose parameters taken by central differences of the yardstick's cost.  The chain is valid only while
the code under test reports the yardstick's (n_successful, n_unsuccessful); that equality is checked at every j and the chain stops
at the first difference.

Every bar follows the rules at the top of lin_yardstick.py plus the solve bound above; none is fitted to a result.  So that the
check cannot go vacuous, bar(delta) <= 1e-6 max |delta| is required of every case and iteration (DELTA_CAP, test_pose_step_cpu.py).
"""
import dataclasses

import numpy as np

from tests import helpers as H
from tests import lin_yardstick as Y

V, LD, EPS = Y.V, Y.LD, Y.EPS
GAMMA = (3 * 6 + 1) * EPS
DELTA_CAP = 1e-6
GTOL = 1e-10                         # xrsfm_ba_refine_pose_options
MIN_DIAG, MAX_DIAG = 1e-6, 1e32
MAX_RADIUS, MIN_RADIUS, MIN_REL_DECREASE = 1e16, 1e-32, 1e-3
CONVERGENCE, NO_CONVERGENCE = 0, 1
PAIRS = [(a, b) for a in range(6) for b in range(a, 6)]          # row-major upper triangle, the kernel's order
IDX = np.array([[PAIRS.index((min(a, b), max(a, b))) for b in range(6)] for a in range(6)])
DEFAULTS = dict(initial_radius=1e4, huber_a=5.99, function_tolerance=1e-6, parameter_tolerance=1e-8)
FIELDS = ("n_successful", "n_unsuccessful", "lm_steps_attempted", "termination", "termination_reason")


class Unsupported(Exception):
    """The chain met something no case may contain (a step without a positive model decrease, an indefinite A)."""


# ------------------------------------------------------------------------------------------------ the linearisation
def selected(case):
    n = case.arr["points"].shape[0]
    return np.ones(n, bool) if case.mask is None else np.asarray(case.mask, bool)


def linearise(case, q, t):
    """H (21 upper entries), g (6), cost as V at the float64 pose (q, t), over the selected correspondences, and the facts."""
    arr = dict(case.arr, cam_q=np.asarray(q, np.float64).reshape(1, 4), cam_t=np.asarray(t, np.float64).reshape(1, 3))
    ref = Y.reference(arr, False, case.opts["huber_a"], case.mask)
    sel = selected(case)
    F, r = ref["Jc"][sel], ref["r"][sel]
    idx = np.zeros(F.shape[0], np.int64)
    Hu = Y.seg_sum(V.stack([F[:, 0, a] * F[:, 0, b] + F[:, 1, a] * F[:, 1, b] for a, b in PAIRS]), idx, 1)[0]
    g = Y.seg_sum(F[:, 0] * r[:, 0:1] + F[:, 1] * r[:, 1:2], idx, 1)[0]
    return dict(H=Hu, g=g, cost=ref["cost"], clamped=ref["clamped"][sel], huber_out=(ref["huber_out"] & ~ref["clamped"])[sel],
                fragile=int(ref["fragile"][sel].sum()))


def cost_only(case, q, t):
    arr = dict(case.arr, cam_q=np.asarray(q, np.float64).reshape(1, 4), cam_t=np.asarray(t, np.float64).reshape(1, 3))
    return Y.reference(arr, False, case.opts["huber_a"], case.mask)["cost"]


def _v1(x):
    return V(x.v.reshape(1), x.e.reshape(1))


def quat_plus(q, d):
    """Plus(q, d) as V [4] from the float64 quaternion q and the tangent step d (V [3])."""
    diff = Y._quat_plus_diff([V(np.array([q[k]])) for k in range(4)], [_v1(d[k]) for k in range(3)])
    return V(np.asarray(q, np.float64)) - diff[0]


def gradmax(q, g):
    """|x - Plus(x, -g)|_inf of the pose block (refine_gradmax)."""
    diff = Y._quat_plus_diff([V(np.array([q[k]])) for k in range(4)], [_v1(-g[k]) for k in range(3)])
    return Y._max_norm([diff, g[3:6]])


def scales(lin):
    return 1.0 / (1.0 + lin["H"][IDX[np.arange(6), np.arange(6)]].sqrt())


# ------------------------------------------------------------------------------------------------ the solve
def _chol(A):
    L = np.zeros((6, 6), LD)
    for j in range(6):
        d = A[j, j] - (L[j, :j] * L[j, :j]).sum()
        if not d > 0:
            raise Unsupported("A is not positive definite")
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, 6):
            L[i, j] = (A[i, j] - (L[i, :j] * L[j, :j]).sum()) / L[j, j]
    return L


def _llt_solve(L, b):
    y = np.array(b, LD)
    for i in range(6):
        y[i] = (y[i] - (L[i, :i] * y[:i]).sum()) / L[i, i]
    for i in range(5, -1, -1):
        y[i] = (y[i] - (L[i + 1:, i] * y[i + 1:]).sum()) / L[i, i]
    return y


def solve_step(lin, S, R, q, t):
    """One proposed step.  Returns dict(delta, model, qc, tc, step_norm, xnorm: V; clamp_lo, clamp_hi: taken per diagonal;
    fragile: list of names)."""
    H6, g = lin["H"][IDX], lin["g"]
    SHS = H6 * V(S.v[:, None], S.e[:, None]) * V(S.v[None, :], S.e[None, :])
    k6 = np.arange(6)
    d = SHS[k6, k6]
    lo, hi = d.v < LD(MIN_DIAG), d.v > LD(MAX_DIAG)
    fragile = []
    if ((np.abs(d.v - LD(MIN_DIAG)) <= d.e) | (np.abs(d.v - LD(MAX_DIAG)) <= d.e)).any():
        fragile.append("damping clamp")
    dd = V.where(lo, MIN_DIAG, V.where(hi, MAX_DIAG, d))
    Ad = d + dd / R
    Av, Ae = SHS.v.copy(), SHS.e.copy()
    Av[k6, k6], Ae[k6, k6] = Ad.v, Ad.e
    b = -(S * g)
    L = _chol(Av)
    y = _llt_solve(L, b.v)
    Ainv = np.stack([_llt_solve(L, np.eye(6, dtype=LD)[k]) for k in range(6)], axis=1)
    ay = np.abs(y)
    ye = np.abs(Ainv) @ (Ae @ ay + b.e + GAMMA * ((np.abs(L) @ np.abs(L.T)) @ ay))
    delta = S * V(y, ye)
    dl = [delta[k] for k in range(6)]
    gd = Y._dot([g[k] for k in range(6)], dl)
    hv = [Y._dot([H6[a, c] for c in range(6)], dl) for a in range(6)]
    model = -(gd + 0.5 * Y._dot(dl, hv))
    qc = quat_plus(q, delta[0:3])
    tc = V(np.asarray(t, np.float64)) + delta[3:6]
    dq, dt = qc - V(np.asarray(q, np.float64)), tc - V(np.asarray(t, np.float64))
    st2 = Y._dot([dq[k] for k in range(4)] + [dt[k] for k in range(3)], [dq[k] for k in range(4)] + [dt[k] for k in range(3)])
    x = [V(np.float64(v)) for v in list(q) + list(t)]
    return dict(delta=delta, model=model, qc=qc, tc=tc, step_norm=st2.sqrt(), xnorm=Y._dot(x, x).sqrt(), clamp_lo=lo, clamp_hi=hi,
                fragile=fragile)


def _inside(a, b):
    """Is the comparison of the V a with the V b undecided in float64?"""
    return bool(np.abs(a.v - b.v) <= a.e + b.e)


def decide(st, cost, cost_c, opts):
    """The tolerance exits and the rho test.  Returns (decision, rho or None, fragile names)."""
    fragile = []
    ptol, ftol = opts["parameter_tolerance"], opts["function_tolerance"]
    lhs, rhs = st["step_norm"], (st["xnorm"] + ptol) * ptol
    if _inside(lhs, rhs):
        fragile.append("parameter tolerance")
    if lhs.v <= rhs.v:
        return "ptol", None, fragile
    change = cost - cost_c
    lhs, rhs = change.abs(), cost * ftol
    if _inside(lhs, rhs):
        fragile.append("function tolerance")
    if lhs.v <= rhs.v:
        return "ftol", None, fragile
    rho = change / st["model"]
    if _inside(rho, V(MIN_REL_DECREASE)):
        fragile.append("rho")
    return ("accept" if rho.v > LD(MIN_REL_DECREASE) else "reject"), rho, fragile


def grow(R, rho):
    """TrustRegion::grow; (2 rho - 1)^3 as two products (pow() is within an ulp of them)."""
    x = 2.0 * rho - 1.0
    f = 1.0 - x * x * x
    third = V(np.float64(1.0 / 3.0))
    fragile = ["grow max(1/3, .)"] if _inside(f, third) else []
    Rn = R / V.where(f.v > third.v, f, third)
    if _inside(Rn, V(MAX_RADIUS)):
        fragile.append("grow min(1e16, .)")
    return V.where(Rn.v < LD(MAX_RADIUS), Rn, MAX_RADIUS), fragile


def cost_sensitivity(case, q, t, eq, et):
    """|grad cost| . (eq, et) over the seven pose parameters, the gradient by central differences (h = 2^-20, exact in float64)."""
    h = 2.0 ** -20
    x0 = np.concatenate([np.asarray(q, np.float64), np.asarray(t, np.float64)])
    e = np.concatenate([eq, et])
    out = LD(0)
    for k in range(7):
        xp, xm = x0.copy(), x0.copy()
        xp[k] += h; xm[k] -= h
        d = (cost_only(case, xp[:4], xp[4:]).v - cost_only(case, xm[:4], xm[4:]).v) / LD(xp[k] - xm[k])
        out += np.abs(d) * e[k]
    return out


# ------------------------------------------------------------------------------------------------ the checker
@dataclasses.dataclass
class Report:
    ratios: dict = dataclasses.field(default_factory=dict)            # check -> largest ratio to its bar (exact checks: 0 / inf)
    mismatch: list = dataclasses.field(default_factory=list)          # discrete differences (counters, exits, kept points)
    fragile: list = dataclasses.field(default_factory=list)
    cap: float = 0.0                                                   # largest bar(delta) / max |delta|
    facts: dict = dataclasses.field(default_factory=dict)

    def note(self, key, r):
        r = float(np.max(r))
        self.ratios[key] = max(self.ratios.get(key, 0.0), r) if r == r else float("inf")

    @property
    def worst(self):
        return max(self.ratios.values(), default=0.0)

    @property
    def ok(self):
        return not self.mismatch and self.worst <= 1.0


def _r64(x):
    return np.asarray(x.v, np.float64)


def _same_bits(a, b):
    return np.asarray(a, np.float64).tobytes() == np.asarray(b, np.float64).tobytes()


_LIN0 = {}


def _initial(case):
    if case.name not in _LIN0:
        lin = linearise(case, case.arr["cam_q"][0], case.arr["cam_t"][0])
        _LIN0[case.name] = (lin, scales(lin))
    return _LIN0[case.name]


def check_case(case, run=None):
    """Walk the case's iterations.  run(k) is the code under test at max_iterations = k: a dict with q, t, initial_cost, final_cost
    and FIELDS.  run = None seats the yardstick on itself (its own candidates, rounded to float64): coverage()."""
    rep = Report()
    opts = case.opts
    q, t = np.array(case.arr["cam_q"][0], np.float64), np.array(case.arr["cam_t"][0], np.float64)
    lin, S = _initial(case)
    lin0 = lin
    if lin["fragile"]:
        rep.fragile.append(f"{lin['fragile']} fragile observations at the start")
    cost, R, dec = lin["cost"], V(np.float64(opts["initial_radius"])), LD(2)
    ns = nu = att = 0
    done = None
    gm = gradmax(q, lin["g"])
    if _inside(gm, V(GTOL)):
        rep.fragile.append("gradient test at the start")
    if gm.v <= LD(GTOL):
        done = (CONVERGENCE, 1)
    decisions, clamp_taken, clamp_second, clamped_cand_only = [], False, False, 0
    for j in range(case.k + 1):
        got = run(j) if run is not None else None
        moved = None                      # the candidate bars when the yardstick accepts this step
        if j > 0 and done is None:
            st = solve_step(lin, S, R, q, t)
            att += 1
            rep.fragile += [f"{x} (iteration {j})" for x in st["fragile"]]
            dmax = np.abs(st["delta"].v).max()
            rep.cap = max(rep.cap, float(st["delta"].e.max() / dmax) if dmax > 0 else float("inf"))
            clamp_taken |= bool(st["clamp_lo"].any())
            clamp_second |= j == 2 and bool(st["clamp_lo"].any())
            if not st["model"].v > st["model"].e:
                raise Unsupported(f"{case.name}: model decrease {st['model'].v} (bar {st['model'].e}) at iteration {j}")
            qc64, tc64 = _r64(st["qc"]), _r64(st["tc"])
            lin_c = linearise(case, qc64, tc64)
            if lin_c["fragile"]:
                rep.fragile.append(f"{lin_c['fragile']} fragile observations at the candidate of iteration {j}")
            what, rho, fr = decide(st, cost, lin_c["cost"], opts)
            if what == "accept":
                rep.fragile += [f"{x} (iteration {j})" for x in fr]
                pq, pt = (qc64, tc64) if got is None else (np.asarray(got["q"], np.float64), np.asarray(got["t"], np.float64))
                if _same_bits(pq, q) and _same_bits(pt, t):
                    rep.mismatch.append(f"iteration {j}: the yardstick accepts the step (rho {float(rho.v):.4g}), the code kept the point")
                    break
                moved = (st["qc"], st["tc"])
                lin_n = lin_c if _same_bits(pq, qc64) and _same_bits(pt, tc64) else linearise(case, pq, pt)
                if lin_n["fragile"]:
                    rep.fragile.append(f"{lin_n['fragile']} fragile observations at the returned pose of iteration {j}")
                what2, rho, fr2 = decide(st, cost, lin_n["cost"], opts)
                if what2 != "accept":
                    rep.fragile.append(f"the step of iteration {j} is accepted at the yardstick's candidate, '{what2}' at the returned pose")
                    break
                rep.fragile += [f"{x} at the returned pose (iteration {j})" for x in fr2]
                clamped_cand_only += int((lin_n["clamped"] & ~lin["clamped"]).sum())
                R, fr3 = grow(R, rho)
                if j < case.k:
                    rep.fragile += [f"{x} (iteration {j})" for x in fr3]
                dec, ns = LD(2), ns + 1
                q, t, lin, cost = pq, pt, lin_n, lin_n["cost"]
                gm = gradmax(q, lin["g"])
                if _inside(gm, V(GTOL)):
                    rep.fragile.append(f"gradient test after iteration {j}")
                if gm.v <= LD(GTOL):
                    done = (CONVERGENCE, 1)
            else:
                # the candidate of the code under test is not visible: the decision must hold over the candidate's bar
                wide = cost_sensitivity(case, qc64, tc64, st["qc"].e + EPS * np.abs(st["qc"].v), st["tc"].e + EPS * np.abs(st["tc"].v))
                what2, rho, fr = decide(st, cost, V(lin_c["cost"].v, lin_c["cost"].e + wide), opts)
                rep.fragile += [f"{x} (iteration {j})" for x in fr]
                if what2 != what:
                    rep.fragile.append(f"the decision of iteration {j} depends on the candidate's rounding ({what} / {what2})")
                    break
                clamped_cand_only += int((lin_c["clamped"] & ~lin["clamped"]).sum())
                if what == "ptol":
                    done = (CONVERGENCE, 2)
                elif what == "ftol":
                    done = (CONVERGENCE, 3)
                else:
                    R, dec, nu = R / V(dec), dec * 2, nu + 1
                    if R.v < LD(MIN_RADIUS):
                        done = (CONVERGENCE, 4)
            decisions.append((what,) if rho is None else (what, float(rho.v), float(rho.e)))
        if got is None:
            continue
        # ---- the state after max_iterations = j
        term = done if done is not None else (NO_CONVERGENCE, 5)
        want = dict(zip(FIELDS, (ns, nu, att) + term))
        diff = {k: (int(got[k]), v) for k, v in want.items() if int(got[k]) != v}
        if diff:
            rep.mismatch.append(f"max_iterations = {j}: (reported, expected) {diff}")
        if moved is not None:
            rep.note("q", Y.ratio(got["q"], moved[0]))
            rep.note("t", Y.ratio(got["t"], moved[1]))
        else:
            rep.note("kept", 0.0 if _same_bits(got["q"], q) and _same_bits(got["t"], t) else np.inf)
        rep.note("initial_cost", Y.ratio(got["initial_cost"], lin0["cost"]))
        rep.note("final_cost", Y.ratio(got["final_cost"], cost))
        if diff and any(k in diff for k in ("n_successful", "n_unsuccessful")):
            break                          # the chain of radii is no longer the code's
    rep.facts = dict(n=int(selected(case).sum()), huber_in=int((~lin0["huber_out"] & ~lin0["clamped"]).sum()), huber_out=int(lin0["huber_out"].sum()),
                     clamped_start=int(lin0["clamped"].sum()), clamped_candidate_only=clamped_cand_only, clamp_taken=clamp_taken, clamp_second=clamp_second,
                     decisions=decisions, exit=done, counts=(ns, nu, att))
    return rep


# ------------------------------------------------------------------------------------------------ cases
@dataclasses.dataclass
class Case:
    name: str
    family: str
    arr: dict
    k: int = 1
    mask: object = None
    opts: dict = dataclasses.field(default_factory=lambda: dict(DEFAULTS))
    expect: dict = dataclasses.field(default_factory=dict)           # facts coverage() must report (test_pose_step_cpu.py)

    @property
    def model(self):
        return int(self.arr["intr_model"][0])


SIZES = (1, 2, 3, 5, 63, 64, 65, 255, 256, 257, 513)
RADII = (1.0, 1e4)
SPECTRUM = (1e-12, 1e-4, 1.0, 1e4, 1e12, 1e16)
MASKED_N = 257


def _opts(**kw):
    return dict(DEFAULTS, **kw)


def _with_pose(arr, q, t):
    return dict(arr, cam_q=np.asarray(q, np.float64).reshape(1, 4).copy(), cam_t=np.asarray(t, np.float64).reshape(1, 3).copy())


def after_one_step(arr, **opts):
    """The problem with the yardstick's own first candidate (rounded to float64) as the initial pose."""
    c = Case("tmp", "tmp", arr, opts=_opts(**opts))
    lin = linearise(c, arr["cam_q"][0], arr["cam_t"][0])
    st = solve_step(lin, scales(lin), V(np.float64(c.opts["initial_radius"])), arr["cam_q"][0], arr["cam_t"][0])
    return _with_pose(arr, _r64(st["qc"]), _r64(st["tc"]))


def t_perturbed(arr, seed, sigma=1.0):
    """The initial translation moved by N(0, sigma) per axis."""
    return _with_pose(arr, arr["cam_q"][0], arr["cam_t"][0] + np.random.default_rng(seed).normal(0, sigma, 3))


def on_axis(du=3.0, dv=-2.0):
    """One point on the optical axis of an identity pose, observed (du, dv) px off the principal point: the columns of the rotation
    about and the translation along the axis are exactly zero, so two diagonals of S H S are 0 and the clamp's lower bound is taken.
    With an offset of 0.01 px the point stays so close to the axis after a step that those diagonals stay below 1e-6: the clamp is
    taken at the second iteration too, where the damping, unlike everywhere else, depends on the scales S (elsewhere
    S (H + diag(H) / R) S y = -S g gives the same delta = S y for any S)."""
    arr = H.make_pose_problem(1, seed=0, model=2)
    prm = arr["intr_params"][0]
    return dict(arr, cam_q=np.array([[0.0, 0.0, 0.0, 1.0]]), cam_t=np.zeros((1, 3)), points=np.array([[0.0, 0.0, 10.0]]),
                obs_uv=np.array([[prm[1] + du, prm[2] + dv]]))


def far(arr, shift):
    """Points and t moved by `shift` along (1, 1, 1) / sqrt(3) consistently: t - M(q) d (rounded to float64), so that M P + t
    cancels log10(shift) digits."""
    d = np.full(3, shift / np.sqrt(3.0), LD)
    M = np.array([[float(x.v[0]) for x in row] for row in Y._quat_mat(arr["cam_q"])], LD)
    return dict(_with_pose(arr, arr["cam_q"][0], (arr["cam_t"][0].astype(LD) - M @ d).astype(np.float64)),
                points=(arr["points"].astype(LD) + d).astype(np.float64))


def all_clamped(arr):
    """Every point behind the camera."""
    return _with_pose(arr, arr["cam_q"][0], arr["cam_t"][0] - np.array([0.0, 0.0, 100.0]))


def _build():
    cases = []
    add = lambda *a, **kw: cases.append(Case(*a, **kw))
    P = H.make_pose_problem
    for n in SIZES:
        for model in range(5):
            for R in RADII:
                add(f"n{n}_m{model}_R{R:g}", "sizes", P(n=n, seed=40 + model, model=model), opts=_opts(initial_radius=R))
    for model in range(5):
        add(f"masked_m{model}", "sizes", P(n=MASKED_N, seed=60 + model, model=model), mask=(np.arange(MASKED_N) % 3 != 1).astype(np.uint8),
            expect=dict(n=int((np.arange(MASKED_N) % 3 != 1).sum())))
    for R in RADII:
        add(f"on_axis_R{R:g}", "sizes", on_axis(), opts=_opts(initial_radius=R), expect=dict(clamp_taken=True))
    add("on_axis_near_k2", "sizes", on_axis(0.01, -0.007), k=2, opts=_opts(initial_radius=1.0, function_tolerance=0.0, parameter_tolerance=0.0),
        expect=dict(clamp_second=True, sequence=("accept", "accept")))
    spec = P(n=65, seed=44, model=4)
    for R in SPECTRUM:
        add(f"radius_{R:g}", "radius", spec, opts=_opts(initial_radius=R), expect=dict(exit=(CONVERGENCE, 2)) if R == 1e-12 else {})
        add(f"radius_{R:g}_notol", "radius", spec, opts=_opts(initial_radius=R, function_tolerance=0.0, parameter_tolerance=0.0),
            expect=dict(exit=None))
    add("huber_mixed_n65", "huber", after_one_step(P(n=65, seed=51, model=4)), k=3, expect=dict(huber_min_frac=0.1, exit=(CONVERGENCE, 3)))
    add("huber_mixed_n257", "huber", after_one_step(P(n=257, seed=45, model=2)), k=3, opts=_opts(function_tolerance=0.0, parameter_tolerance=0.0),
        expect=dict(huber_min_frac=0.1, sequence=("accept", "accept", "accept")))
    add("huber_inner_n65", "huber", P(n=65, seed=43, model=3), opts=_opts(huber_a=1e3), expect=dict(huber_out=0))
    for name, n, seed, model, dz, tseed, seq in CLAMPED:
        arr = P(n=n, seed=seed, model=model)
        add(name, "clamped", t_perturbed(_with_pose(arr, arr["cam_q"][0], arr["cam_t"][0] + np.array([0.0, 0.0, dz])), tseed),
            expect=dict(clamped_start_min=1, clamped_candidate_only_min=1, sequence=seq))
    add("all_clamped", "clamped", all_clamped(P(n=65, seed=41, model=1)), expect=dict(exit=(CONVERGENCE, 1), counts=(0, 0, 0), clamped_start=65))
    rej = P(n=3, seed=44, model=4)
    add("rejected_n3_R2e4", "rejected", rej, k=3, opts=_opts(initial_radius=2e4), expect=dict(sequence=("reject", "accept")))
    add("rejected_n3_R1e12", "rejected", rej, k=3, opts=_opts(initial_radius=1e12), expect=dict(sequence=("reject", "reject", "reject")))
    for name, n, seed, model, tseed, sigma, seq in REJECTED:
        add(name, "rejected", t_perturbed(P(n=n, seed=seed, model=model), tseed, sigma), k=3, opts=_opts(huber_a=1e3),
            expect=dict(sequence=seq, rho_margin=1e3))
    add("plain_n257", "plain", P(n=257, seed=42, model=2), k=3, expect=dict(sequence=("accept", "accept")))
    add(f"far_{FAR_SHIFT:g}", "far", far(P(n=65, seed=42, model=2), FAR_SHIFT))
    return {c.name: c for c in cases}


# Found by searching make_pose_problem and pinned by their seeds.
# CLAMPED: (name, n, seed, model, shift of t along the optical axis, seed of the N(0, 1) perturbation of t, decisions): points behind
# the camera at the start and more of them at the candidate.
CLAMPED = (("clamped_n65_accept", 65, 41, 2, -20.0, 1, ("accept",)), ("clamped_n65_reject", 65, 42, 2, -20.0, 3, ("reject",)),
           ("clamped_n257_accept", 257, 41, 3, -14.0, 0, ("accept",)))
# REJECTED: (name, n, seed, model, seed and sigma of the perturbation of t, decisions), quadratic loss (huber_a = 1e3), radius 1e4
REJECTED = (("rejected_n65", 65, 43, 2, 6, 3.0, ("reject", "reject", "accept")),)
# the bar of delta exceeds DELTA_CAP at a shift of 1e4 (4.8e-6 of max |delta|: M P + t cancels four digits and the solve amplifies
# the bars of H and g); 1e3 is the largest power of ten at which the cap holds
FAR_SHIFT = 1e3
_CASES = {}


def cases():
    if not _CASES:
        _CASES.update(_build())
    return _CASES


def case_names():
    return list(cases())


FAMILIES = ("sizes", "radius", "huber", "clamped", "rejected", "plain", "far")
_COV = {}


def coverage(name):
    """The facts a case exists for, from the yardstick seated on itself: counts on each Huber branch and clamped at the start, newly
    clamped at a candidate, whether the clamp's lower bound was taken, the decision sequence, the exit and (n_successful,
    n_unsuccessful, attempted); with them the fragile decisions and the largest bar(delta) / max |delta| of the self-seated chain."""
    if name not in _COV:
        rep = check_case(cases()[name])
        _COV[name] = dict(rep.facts, fragile=list(rep.fragile), cap=rep.cap)
    return _COV[name]


def assert_expected(name, facts):
    """The coverage facts of the case `name` hold in `facts` (Report.facts)."""
    c = cases()[name]
    for k, v in c.expect.items():
        if k == "huber_min_frac":
            assert min(facts["huber_in"], facts["huber_out"]) >= v * facts["n"], (name, facts)
        elif k.endswith("_min") and k != "rho_margin":
            assert facts[k[:-4]] >= v, (name, k, facts)
        elif k == "sequence":
            assert tuple(d[0] for d in facts["decisions"][:len(v)]) == v, (name, facts["decisions"])
        elif k == "rho_margin":
            for d in facts["decisions"]:
                assert abs(d[1] - MIN_REL_DECREASE) >= v * d[2], (name, d)
        else:
            assert facts[k] == v, (name, k, facts[k], v)


def assert_sound(name, rep):
    """No fragile decision, the cap on bar(delta), and the case's facts, on the chain a code under test was seated on."""
    assert not rep.fragile, (name, rep.fragile)
    assert rep.cap <= DELTA_CAP, (name, rep.cap)
    assert_expected(name, rep.facts)
