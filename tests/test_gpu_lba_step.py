"""Every Levenberg-Marquardt step of lba_resident_solve (xrsfm_amd/csrc/ba_lba.h: its own per-observation blocks, point factor and
V = (F^T E) C staging, track-by-camera lane table and sliced gather of S and b, 60x60 right-looking Cholesky in LDS with wave-0
triangular solves, camera update, gradient max-norm, back-substitution, candidate cost and trust-region book-keeping) against the
extended-precision yardstick of tests/lba_step_yardstick.py.  A run with max_iterations = 0..k returns the state after exactly that
many attempted steps; the chain is re-seated on the returned state at every k.  Every case of the catalogue runs on two paths:
"resident" = XRSFM_BA_SOLVER_RESIDENT through xrsfm_ba_debug_resident_rows (the same launch plus the iteration rows), and
"engine" = XRSFM_BA_SOLVER_CHOLESKY on the same problems (ctx.reset() and run(max_iterations = k) on one context per case), whose
steps at this size had no end-to-end check either.  The engine reports the same summary fields at a truncated iteration limit and
has no rows.

Per case and k: every camera and point elementwise against the candidate bars of the yardstick's step from the state returned for
k - 1, or bit-for-bit equality with that state where the yardstick keeps the point; initial_cost and final_cost against the cost
bars; (n_successful, n_unsuccessful, lm_steps_attempted, termination, termination_reason) equal to the yardstick's; the rows
(cost, change, gmax, step, rho, radius: lba_step_yardstick's docstring); two identical calls return identical bits; the rows entry
leaves the state and the summary of a plain run, bit for bit.  On the chain the library was seated on, no decision is fragile,
bar(delta) <= 1e-6 max |delta| and the case still exercises what it exists for.  One batch test sends the catalogue, grouped by
options, through xrsfm_ba_run_batch in one launch per group and asserts state and summary bit-equal to the single resident runs (the
existing batch tests hold no 1-camera, 9-tile or 17-tile problem).

Largest measured ratio of each check to its bar, per case family: resident kernel / engine on an MI355X / float64 restatement
(test_lba_step_cpu.py).  Nothing in the assertions depends on these numbers; the bar is 1.0.

  check        gather                  chunks                  tracks                  blocks                  edges                   decisions
  q            6e-5 / 6e-5 / 3e-5      2e-5 / 1e-5 / 5e-5      4e-5 / 4e-5 / 5e-5      2e-3 / 2e-3 / 5e-3      1e-5 / 1e-5 / 3e-5      0.12 / 0.12 / 0.15
  t            2e-3 / 1e-3 / 7e-4      1e-3 / 2e-3 / 1e-3      5e-4 / 6e-4 / 9e-4      5e-3 / 5e-3 / 5e-3      2e-4 / 4e-4 / 3e-4      0.69 / 0.69 / 0.69
  P            7e-4 / 5e-4 / 1e-3      4e-5 / 2e-5 / 9e-5      5e-4 / 6e-4 / 6e-4      1e-2 / 1e-2 / 2e-2      3e-5 / 1e-5 / 3e-5      0.12 / 0.12 / 0.12
  initial_cost 7e-3 / 7e-3 / 2e-2      3e-3 / 2e-3 / 1e-2      1e-2 / 1e-2 / 1e-2      7e-3 / 7e-3 / 8e-3      2e-3 / 2e-3 / 2e-3      3e-3 / 3e-3 / 1e-2
  final_cost   1e-2 / 7e-2 / 7e-2      3e-2 / 8e-3 / 2e-2      2e-2 / 1e-2 / 2e-2      9e-3 / 8e-3 / 9e-3      8e-3 / 7e-3 / 7e-3      0.16 / 0.16 / 0.16
  row_cost     1e-2 / - / 7e-2         3e-2 / - / 2e-2         2e-2 / - / 2e-2         9e-3 / - / 9e-3         8e-3 / - / 7e-3         0.16 / - / 0.16
  row_change   7e-3 / - / 7e-2         2e-2 / - / 1e-2         1e-2 / - / 1e-2         2e-3 / - / 4e-3         3e-3 / - / 3e-3         0.16 / - / 0.16
  row_gmax     6e-3 / - / 5e-3         3e-3 / - / 4e-3         7e-4 / - / 2e-3         2e-2 / - / 1e-2         9e-4 / - / 7e-4         0.12 / - / 0.12
  row_step     6e-3 / - / 4e-3         2e-2 / - / 1e-2         1e-2 / - / 1e-2         4e-3 / - / 4e-3         4e-3 / - / 4e-3         4e-2 / - / 4e-2
  row_rho      2e-4 / - / 1e-4         5e-8 / - / 2e-7         3e-6 / - / 6e-7         7e-7 / - / 3e-7         1e-8 / - / 1e-8         2e-2 / - / 2e-2
  row_radius   0.50 / - / 0.50         0.50 / - / 0.50         0.50 / - / 0.50         0.50 / - / 0.50         0.50 / - / 0.50         0.50 / - / 0.50
  Every exact check (kept points, counters, exits, row counts and earlier rows, two identical calls, rows entry against a plain run,
  batch against single launch): exact on all paths.
  The states sit far inside their bars because the forward bound of the solve charges every entry of S and b its whole bar through
  |S^-1| at once and the bars of the linearisation enter S with the worst sign.  The largest ratios (decisions family) are the step at
  radius 1e-3 and the on-axis case at radius 1, so short that the one rounding of t + delta and of the quaternion product is most of
  the bar.  row_radius = 0.50: after a step with rho near 1 the radius is R / (1/3), one rounding where the bar counts two.  A discrete
  defect (a dropped track, a skipped chunk, a transposed block, b without V z, scales recomputed, no clamp, a wrong radius rule) moves
  the state by 1e5 to 1e10 bars, keeps a point the yardstick moves, or changes a row (test_lba_step_cpu.py).
"""
import numpy as np
import pytest

from tests import helpers as H
from tests import lba_step_yardstick as LY

pytestmark = pytest.mark.gpu

PATHS = ("resident", "engine")
SUMMARY = ("initial_cost", "final_cost", "num_residuals", "num_effective_params", "n_successful", "n_unsuccessful", "termination",
           "termination_reason", "pcg_iterations", "lm_steps_attempted", "linear_solver_used")          # every field except the times / profile


def _options(capi, case, k, solver):
    o = case.opts
    return capi.default_options(linear_solver=solver, max_iterations=k, initial_radius=o["initial_radius"], huber_a=o["huber_a"],
                                function_tolerance=o["function_tolerance"], parameter_tolerance=o["parameter_tolerance"],
                                gradient_tolerance=o["gradient_tolerance"])


def _result(ctx, s, rows):
    q, t, P = ctx.download()
    return dict(q=q, t=t, P=P, initial_cost=float(s.initial_cost), final_cost=float(s.final_cost), rows=rows,
                summary=tuple(getattr(s, f) for f in SUMMARY), **{f: int(getattr(s, f)) for f in LY.FIELDS})


def _bits(r):
    return (r["q"].tobytes(), r["t"].tobytes(), r["P"].tobytes(), np.float64(r["initial_cost"]).tobytes(), np.float64(r["final_cost"]).tobytes(),
            r["summary"], None if r["rows"] is None else tuple(tuple(np.float64(w[k]).tobytes() for k in LY.ROW_FIELDS) + (w["it"],) for w in r["rows"]))


def _call(capi, ctx, case, k, path):
    ctx.reset()
    if path == "resident":
        s, rows = ctx.debug_resident_rows(_options(capi, case, k, capi.SOLVER_RESIDENT))
        return _result(ctx, s, rows)
    return _result(ctx, ctx.run(_options(capi, case, k, capi.SOLVER_CHOLESKY)), None)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", LY.case_names())
def test_lba_step_matches_yardstick(lib, name, path):
    from xrsfm_amd import capi
    case = LY.cases()[name]
    ctx = capi.Context(H.to_product(case.arr))
    try:
        def run(k):
            a, b = _call(capi, ctx, case, k, path), _call(capi, ctx, case, k, path)
            assert _bits(a) == _bits(b), (name, path, k, "two identical calls differ")
            return a

        rep = LY.check_case(case, run)
        if path == "resident":                 # the rows entry leaves what a plain run leaves
            got = _call(capi, ctx, case, case.k, path)
            ctx.reset()
            plain = _result(ctx, ctx.run(_options(capi, case, case.k, capi.SOLVER_RESIDENT)), got["rows"])
            assert _bits(got) == _bits(plain), (name, "the rows entry and a plain run differ")
            assert got["summary"][-1] == capi.SOLVER_RESIDENT
    finally:
        ctx.close()
    print(f"LBASTEP case={name} family={case.family} path={path} worst={rep.worst:.4g} cap={rep.cap:.2g} "
          + " ".join(f"{k}={v:.4g}" for k, v in rep.ratios.items()) + f" sequence={rep.facts['sequence']}")
    LY.assert_sound(name, rep)
    assert not rep.mismatch, (name, path, rep.mismatch)
    bad = {k: v for k, v in rep.ratios.items() if not v <= 1.0}
    assert not bad, f"{(name, path)}: outside the bar: {bad}"


def test_batch_is_bit_equal_to_the_single_launches(lib):
    """The catalogue grouped by (options, K), each group one xrsfm_ba_run_batch launch."""
    from xrsfm_amd import capi
    groups = {}
    for name in LY.case_names():
        c = LY.cases()[name]
        groups.setdefault((tuple(sorted(c.opts.items())), c.k), []).append(c)
    assert {"cams1", "tiles9", "tiles17"} <= {c.name for g in groups.values() for c in g}
    for (_, k), group in groups.items():
        opt = _options(capi, group[0], k, capi.SOLVER_RESIDENT)
        ctxs = [capi.Context(H.to_product(c.arr)) for c in group]
        try:
            code, sums, codes = capi.run_batch(ctxs, opt)
            assert code == 0 and not codes.any(), ([c.name for c in group], code, codes)
            for c, ctx, s in zip(group, ctxs, sums):
                got = _result(ctx, s, None)
                one = capi.Context(H.to_product(c.arr))
                try:
                    want = _result(one, one.run(opt), None)
                finally:
                    one.close()
                assert _bits(got) == _bits(want), (c.name, "batch and single launch differ")
        finally:
            for ctx in ctxs:
                ctx.close()
