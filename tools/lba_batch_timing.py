"""xrsfm_ba_run_batch against N sequential xrsfm_ba_run calls with XRSFM_BA_SOLVER_CHOLESKY, on the same N contexts after a reset.

Shapes: the 7-camera / 6000-observation shape of tools/lba_timing.py and a 5-camera / 600-observation one; N = 1, 16, 64, 256, 512,
1024.  Per shape the contexts are created once (8 seeds, cycled) and the first N of them are used.  Per (shape, N): one warm-up of
each path, then REPEATS rounds that alternate the two paths (reset of every context outside the timed window, host clock around calls
that end in a stream synchronise); median, minimum and maximum are reported, and the median per problem.  A further batch call with
profile = 1 gives the HIP-event time of the one launch.  The LBA options of the reference (5 iterations, 1e-4 / 1e-5).

    python tools/lba_batch_timing.py [--out FILE.md] [--repeats 7] [--sizes 1,16,64,256,512,1024]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: F401  (first, so that both share one HIP runtime)

from xrsfm_amd import capi
from tests import helpers as H

SHAPES = [("7 cameras / 1500 points / k=4", 7, 1500, 4), ("5 cameras / 200 points / k=3", 5, 200, 3)]
LBA = dict(max_iterations=5, function_tolerance=1e-4, parameter_tolerance=1e-5)


def ms(ts):
    return statistics.median(ts) * 1e3, min(ts) * 1e3, max(ts) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--sizes", default="1,16,64,256,512,1024")
    a = ap.parse_args()
    sizes = [int(x) for x in a.sizes.split(",")]
    if capi.device_count() < 1:
        raise SystemExit("no HIP device: nothing to measure")
    o_batch = capi.default_options(linear_solver=capi.SOLVER_RESIDENT, **LBA)
    o_prof = capi.default_options(linear_solver=capi.SOLVER_RESIDENT, profile=1, **LBA)
    o_seq = capi.default_options(linear_solver=capi.SOLVER_CHOLESKY, **LBA)
    lines = []

    def emit(s=""):
        print(s, flush=True)
        lines.append(s)

    for label, nc, npts, k in SHAPES:
        arrs = [H.make(nc, npts, k, seed=5 + i) for i in range(8)]
        n_obs = arrs[0]["obs_cam"].shape[0]
        tiles = capi.debug_pack(H.to_product(arrs[0]))["tiles"]
        ctxs = [capi.Context(H.to_product(arrs[i % len(arrs)])) for i in range(max(sizes))]
        emit(f"### {label} ({n_obs} observations, {tiles} tiles)")
        emit()
        emit("| N | batch call: median (min .. max) ms | of it the one launch (HIP events) ms | N sequential `_CHOLESKY` runs: median (min .. max) ms "
             "| per problem, batch ms | per problem, sequential ms | sequential / batch |")
        emit("|---|---|---|---|---|---|---|")
        for n in sizes:
            use = ctxs[:n]

            def reset():
                for c in use:
                    c.reset()

            def batch(opt=o_batch):
                t0 = time.perf_counter()
                code, sums, _ = capi.run_batch(use, opt)
                dt = time.perf_counter() - t0
                assert code == 0, code
                return dt, sums

            def sequential():
                t0 = time.perf_counter()
                for c in use:
                    s = c.run(o_seq)
                return time.perf_counter() - t0, s

            reset(); batch(); reset(); sequential()          # warm-up of both paths at this size
            tb, ts = [], []
            for _ in range(a.repeats):
                reset(); dt, sb = batch(); tb.append(dt)
                reset(); dt, ss = sequential(); ts.append(dt)
            reset(); _, sp = batch(o_prof)
            (bm, b0, b1), (sm, s0, s1) = ms(tb), ms(ts)
            emit(f"| {n} | {bm:.3f} ({b0:.3f} .. {b1:.3f}) | {sp[0].dom_kernel_ms:.3f} | {sm:.3f} ({s0:.3f} .. {s1:.3f}) | {bm / n:.4f} | {sm / n:.4f} | {sm / bm:.2f} |")
        emit()
        emit(f"Steps of the last problem: batch {sb[-1].n_successful}+{sb[-1].n_unsuccessful} (reason {sb[-1].termination_reason}), "
             f"sequential {ss.n_successful}+{ss.n_unsuccessful} (reason {ss.termination_reason}).")
        emit()
        for c in ctxs:
            c.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
