"""Time xrsfm_ba_two_view_init and write profiles/two_view_init.md: wall time per call for 1 / 64 / 256 pairs of 300 and 2000
matches at outlier shares 0.2 and 0.6, and beside it the sequential host build of the same two headers (ba_init_scan.h,
ba_init_geom.h: the driver of tests/init_host_driver.py, g++ -O2, one core) on the same box.

Wall time: host clock around the blocking C call through the ctypes wrapper (checks, bound rows and sample quintuples on the host,
staging, one upload, one launch, one read-back), the median of --repeat calls (at least 20) after --warmup calls.  Host column: the
time the driver spends in its solves (its own steady clock, parsing and printing excluded), one run.  Pairs: tests/init_yardstick.py's
make_pair, wide baseline, 0.5 px of noise at fx = 800; every pair of a call is different.

    python tools/two_view_timing.py [--repeat 20] [--warmup 3] [--out profiles/two_view_init.md] [--no-host]
"""
import argparse
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "two_view_init.md"))
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    import torch  # noqa: F401  (first, so that both share one HIP runtime)
    from xrsfm_amd import capi
    from tests import init_host_driver as H
    from tests import init_yardstick as Y
    if capi.device_count() < 1:
        raise SystemExit("no HIP device visible")
    repeat = max(args.repeat, 20)
    tmp = tempfile.mkdtemp()
    exe = None if args.no_host else H.build(tmp, "pairs_o2", H.PAIR_DRIVER, flags=["-O2"])
    rows = []
    for n in (300, 2000):
        for share in (0.2, 0.6):
            pairs = [Y.make_pair(n, share, 0.5, 2.2, seed=100000 + 1000 * int(10 * share) + n + j)[:2] for j in range(256)]
            for npair in (1, 64, 256):
                ptr = (n * np.arange(npair + 1)).astype(np.int32)
                xa = np.ascontiguousarray(np.concatenate([p[0] for p in pairs[:npair]]))
                xb = np.ascontiguousarray(np.concatenate([p[1] for p in pairs[:npair]]))
                th = np.full(npair, Y.TH)
                for _ in range(args.warmup):
                    r = capi.two_view_init(ptr, xa, xb, th)
                wall = []
                for _ in range(repeat):
                    t0 = time.perf_counter()
                    r = capi.two_view_init(ptr, xa, xb, th)
                    wall.append(1e3 * (time.perf_counter() - t0))
                host_ms = float("nan")
                if exe:
                    text = "\n".join(H.pair_input(a, b, Y.TH, Y.Options()) for a, b in pairs[:npair]) + "\n"
                    p = subprocess.run([exe, "time"], input=text, capture_output=True, text=True, check=True)
                    host_ms = float(p.stderr.split()[-1])
                rows.append((npair, n, share, int((r.status == 1).sum()), int((r.accepted & 1).astype(bool).sum()), float(np.median(wall)), float(np.min(wall)),
                             float(np.max(wall)), float(r.num_trials.mean()), host_ms))
                print(rows[-1], flush=True)
    lines = ["# Batched two-view initialisation (`xrsfm_ba_two_view_init`): time per call", "",
             "Measured on one MI355X with the library of the commit that added the call, one session, `python tools/two_view_timing.py "
             "--repeat %d` (%d warm-up calls, then the median of %d calls; smallest and largest call beside it).  Wall time: host clock" % (repeat, args.warmup, repeat),
             "around the blocking call through the ctypes wrapper: argument checks, the rows of the trial bound and the sample quintuples",
             "on the host, staging, one upload, one launch of `k_init_pairs` (one 256-thread workgroup per pair), one read-back.  Host column:",
             "the sequential build of the same two headers (`g++ -O2`, one core of the same box), the time spent in its solves, one run.",
             "No kernel-only time was taken (no HIP events around the launch, no rocprofv3 pass).", "",
             "| pairs | matches per pair | outlier share | geometry found | accepted at 16 deg | wall ms (median) | min | max | mean trials | sequential host ms |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for npair, n, share, found, acc, med, lo, hi, tr, host in rows:
        lines.append(f"| {npair} | {n} | {share} | {found} | {acc} | {med:.3f} | {lo:.3f} | {hi:.3f} | {tr:.1f} | {host:.3f} |")
    lines += ["", "No speed bar is set on these times; the parent commit has no such call to compare with.  The kernel computes every trial of a",
              "sub-block of 32 before the scan sees it, so a pair whose trial bound drops to 6 still pays for 32 sample models.",
              "Not measured: kernel time apart from the call, the share of the steps (a)-(d), other sub-block sizes, hardware counters.", ""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
