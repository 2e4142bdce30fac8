"""Run-only and one-shot times of XRSFM_BA_SOLVER_CHOLESKY and XRSFM_BA_SOLVER_RESIDENT on the LBA-sized shapes of
tools/lba_timing.py that are eligible for the resident solver (at most 10 cameras, 32768 observations), in one process.
Each time is the minimum of 5 after a warm-up; the largest differences between the two results are printed with them."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch  # noqa: F401  (first, so that both share one HIP runtime)

from xrsfm_amd import capi
from tests import helpers as H

SHAPES = [(7, 1500, 4), (7, 6000, 5)]


def timed(arr, solver):
    opt = capi.default_options(max_iterations=5, function_tolerance=1e-4, parameter_tolerance=1e-5, linear_solver=solver)
    capi.solve(H.to_product(arr), opt)          # warm-up
    one_shot = []
    for _ in range(5):
        p = H.to_product(arr); t0 = time.perf_counter(); capi.solve(p, opt); one_shot.append(time.perf_counter() - t0)
    ctx = capi.Context(H.to_product(arr)); ctx.run(opt)
    run_only = []
    for _ in range(5):
        ctx.reset(); t0 = time.perf_counter(); s = ctx.run(opt); run_only.append(time.perf_counter() - t0)
    state = ctx.download()
    ctx.close()
    return min(run_only) * 1e3, min(one_shot) * 1e3, s, state


for nc, npts, k in SHAPES:
    arr = H.make(nc, npts, k, seed=5)
    n_obs = arr["obs_cam"].shape[0]
    out = {name: timed(arr, solver) for name, solver in (("cholesky", capi.SOLVER_CHOLESKY), ("resident", capi.SOLVER_RESIDENT))}
    for name, (run_ms, shot_ms, s, _) in out.items():
        print(f"{nc} cams {npts} pts {n_obs} obs  {name:8s}: run only {run_ms:.3f} ms, one-shot solve {shot_ms:.3f} ms, "
              f"{s.n_successful}+{s.n_unsuccessful} steps, termination {s.termination}/{s.termination_reason}")
    (_, _, se, de), (_, _, sr, dr) = out["cholesky"], out["resident"]
    n_res = 2 * n_obs
    print(f"    resident vs cholesky: |d rmse| {abs(np.sqrt(sr.final_cost / n_res) - np.sqrt(se.final_cost / n_res)):.3e} px, "
          f"|d cam| {max(np.abs(dr[0] - de[0]).max(), np.abs(dr[1] - de[1]).max()):.3e}, |d points| {np.abs(dr[2] - de[2]).max():.3e}, "
          f"run-only ratio {out['resident'][0] / out['cholesky'][0]:.2f}")
