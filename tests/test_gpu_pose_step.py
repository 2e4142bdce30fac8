"""k_refine_pose's Levenberg-Marquardt steps (ba_refine.h: the 28-value reduction, Jacobi scaling, damping clamp, 6x6 Cholesky and
triangular solves, model decrease, quat_plus update and trust-region book-keeping) against the extended-precision yardstick of
tests/pose_step_yardstick.py, through the public call alone: xrsfm_ba_refine_pose with max_iterations = 0..k returns the state
after exactly that many attempted steps.  Every case runs on two paths: the persistent kernel (default) and the same one-camera
problem through the general engine (XRSFM_BA_REFINE_ENGINE=1, set and removed around each call).

Per case and k: q and t elementwise against the candidate bars of the yardstick's step from the pose returned for k - 1; bit-for-bit
equality with that pose where the yardstick rejects the step or a tolerance exit keeps the point; initial_cost and final_cost
against the cost bars (final_cost at the returned pose); (n_successful, n_unsuccessful, lm_steps_attempted, termination,
termination_reason) equal to the yardstick's; two identical calls return identical bits.  On the chain the library was seated on, no
decision is fragile, bar(delta) <= 1e-6 max |delta| and the case still exercises what it exists for.  The engine reports every
field the kernel does at a truncated max_iterations (xrsfm_ba.hip, ba_run_impl: the same iteration-limit exit, counters and
xtr::TrustRegion calls), so no field is treated separately.

Largest measured ratio of each check to its bar, per case family: kernel / engine on an MI355X / float64 restatement
(test_pose_step_cpu.py).  Nothing in the assertions depends on these numbers; the bar is 1.0.

  check         sizes               radius              huber               clamped             rejected            plain               far
  q             2e-2 / 2e-2 / 2e-2  0.11 / 0.11 / 0.11  2e-2 / 2e-2 / 2e-2  2e-5 / 8e-5 / 3e-5  3e-4 / 1e-4 / 1e-4  1e-2 / 1e-2 / 9e-3  2e-6 / 1e-5 / 4e-6
  t             1e-2 / 1e-2 / 1e-2  0.62 / 0.62 / 0.62  2e-2 / 3e-2 / 3e-2  8e-5 / 4e-4 / 9e-5  1e-3 / 4e-4 / 4e-4  3e-2 / 4e-3 / 2e-2  6e-6 / 2e-5 / 2e-5
  initial_cost  0.15 / 0.15 / 0.15  1e-2 / 1e-2 / 7e-3  2e-2 / 2e-2 / 1e-2  3e-2 / 3e-2 / 3e-2  3e-2 / 3e-2 / 4e-2  5e-3 / 5e-3 / 5e-3  5e-2 / 5e-2 / 5e-2
  final_cost    0.22 / 0.22 / 0.22  2e-2 / 2e-2 / 2e-2  2e-2 / 2e-2 / 1e-2  3e-2 / 3e-2 / 3e-2  5e-2 / 4e-2 / 7e-2  7e-3 / 5e-3 / 7e-3  5e-2 / 5e-2 / 5e-2
  Every exact check (kept points, counters, exits, two identical calls): exact on all three.
  The pose sits far inside its bars because the forward bound of the solve charges every entry of A and b its whole bar through
  |A^-1| at once; the largest ratios (radius family) are the steps at radii 1e-12 and 1e-4, so short that the one rounding of
  t + delta and of the quaternion product is most of the bar.  A discrete defect (a dropped term, swapped entries of H, a recomputed S, a skipped clamp, an unshrunk radius,
  the wrong triangle) moves the pose by 1e6 to 1e11 bars or changes a counter (test_pose_step_cpu.py).
"""
import os

import numpy as np
import pytest

from tests import pose_step_yardstick as PY

pytestmark = pytest.mark.gpu

PATHS = ("kernel", "engine")


def _call(capi, case, k, engine):
    o = case.opts
    opt = capi.refine_pose_options(max_iterations=k, initial_radius=o["initial_radius"], huber_a=o["huber_a"],
                                   function_tolerance=o["function_tolerance"], parameter_tolerance=o["parameter_tolerance"])
    arr = case.arr
    if engine:
        os.environ["XRSFM_BA_REFINE_ENGINE"] = "1"
    try:
        q, t, s = capi.refine_pose(case.model, arr["intr_params"][0], arr["points"], arr["obs_uv"], arr["cam_q"][0], arr["cam_t"][0],
                                   inlier_mask=case.mask, options=opt)
    finally:
        if engine:
            del os.environ["XRSFM_BA_REFINE_ENGINE"]
    return dict(q=q, t=t, initial_cost=float(s.initial_cost), final_cost=float(s.final_cost), **{f: int(getattr(s, f)) for f in PY.FIELDS})


def _bits(r):
    return (r["q"].tobytes(), r["t"].tobytes(), np.float64(r["initial_cost"]).tobytes(), np.float64(r["final_cost"]).tobytes(),
            tuple(r[f] for f in PY.FIELDS))


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", PY.case_names())
def test_pose_step_matches_yardstick(lib, name, path):
    from xrsfm_amd import capi
    case = PY.cases()[name]
    assert "XRSFM_BA_REFINE_ENGINE" not in os.environ

    def run(k):
        a, b = _call(capi, case, k, path == "engine"), _call(capi, case, k, path == "engine")
        assert _bits(a) == _bits(b), (name, path, k, "two identical calls differ")
        return a

    rep = PY.check_case(case, run)
    print(f"POSESTEP case={name} family={case.family} path={path} worst={rep.worst:.4g} cap={rep.cap:.2g} "
          + " ".join(f"{k}={v:.4g}" for k, v in rep.ratios.items()) + f" decisions={[d[0] for d in rep.facts['decisions']]}")
    PY.assert_sound(name, rep)
    assert not rep.mismatch, (name, path, rep.mismatch)
    bad = {k: v for k, v in rep.ratios.items() if not v <= 1.0}
    assert not bad, f"{(name, path)}: outside the bar: {bad}"


def test_parameter_tolerance_exit_keeps_the_point(lib):
    """initial_radius = 1e-12: the first step is shorter than the parameter tolerance; reason 2, the pose unchanged bit for bit and
    final_cost == initial_cost, on both paths."""
    from xrsfm_amd import capi
    case = PY.cases()["radius_1e-12"]
    for path in PATHS:
        got = _call(capi, case, 1, path == "engine")
        assert got["termination"] == PY.CONVERGENCE and got["termination_reason"] == 2 and got["lm_steps_attempted"] == 1, (path, got)
        assert got["final_cost"] == got["initial_cost"], (path, got)
        assert np.array_equal(got["q"], case.arr["cam_q"][0]) and np.array_equal(got["t"], case.arr["cam_t"][0]), path


def test_all_clamped_converges_without_a_step(lib):
    """Every point behind the camera: zero gradient, CONVERGENCE by the gradient test (reason 1), no step attempted, the pose
    untouched, cost = n rho(288) / 2 within the cost bar, on both paths and for every iteration limit."""
    from xrsfm_amd import capi
    case = PY.cases()["all_clamped"]
    a = np.longdouble(np.float64(case.opts["huber_a"]))
    want = 65 * (2 * a * np.sqrt(np.longdouble(288)) - np.longdouble(np.float64(case.opts["huber_a"]) ** 2)) / 2
    bar = PY._initial(case)[0]["cost"].e
    for path in PATHS:
        for k in (0, 1, 10):
            got = _call(capi, case, k, path == "engine")
            assert (got["termination"], got["termination_reason"], got["lm_steps_attempted"]) == (PY.CONVERGENCE, 1, 0), (path, k, got)
            assert np.array_equal(got["q"], case.arr["cam_q"][0]) and np.array_equal(got["t"], case.arr["cam_t"][0]), (path, k)
            assert abs(np.longdouble(got["initial_cost"]) - want) <= bar and got["final_cost"] == got["initial_cost"], (path, k, got)
