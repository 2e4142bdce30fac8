"""Time xrsfm_ba_verify_pairs and write profiles/pair_verify.md: wall time per call for 1 / 16 / 256 / 4096 pairs of 100 and 1000
matches at outlier shares 0.3 and 0.7, beside the sequential host driver (tests/fund_host_driver.py: the same headers, g++ -O2, one
core) on the same inputs, and the two measured deviations of F over the test catalogue (the float64 restatement of
tests/fund_yardstick.py and the library, each against the extended-precision run).

Wall time: host clock around the blocking C call through the ctypes wrapper (checks, dyn rows, staging, one upload, one launch,
one read-back), the median of --repeat calls (at least 20) after --warmup calls.  Pairs: the generator of the test catalogue
(1280 x 720 pixels, 0.5 px of noise on the inliers, outliers uniform over the image); every pair of a call is different.  The host
driver is run once per row, on at most --host-pairs pairs (its time grows linearly with the pairs).

    python tools/pair_verify_timing.py [--repeat 20] [--warmup 3] [--out profiles/pair_verify.md] [--no-deviations] [--host-pairs 256]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pair_verify.md"))
    ap.add_argument("--no-deviations", action="store_true")
    ap.add_argument("--host-pairs", type=int, default=256)
    args = ap.parse_args()
    import torch  # noqa: F401  (first, so that both share one HIP runtime)
    from xrsfm_amd import capi
    from tests import fund_host_driver as H
    from tests import fund_yardstick as Y
    if capi.device_count() < 1:
        raise SystemExit("no HIP device visible")
    repeat = max(args.repeat, 20)
    tmp = tempfile.mkdtemp(prefix="pair_verify_")
    exe = H.build(tmp, "pairs", H.PAIR_DRIVER, flags=["-O2"])
    opt = Y.Options()
    rows = []
    for n in (100, 1000):
        for share in (0.3, 0.7):
            pairs = [Y.make_pair(n, share, 0.5, seed=100000 * n + 10000 * int(10 * share) + j)[:2] for j in range(256)]
            text = [H.pair_input(a, b, opt) for a, b in pairs]
            for npair in (1, 16, 256, 4096):
                sel = [pairs[j % 256] for j in range(npair)]
                if npair > 256:                                    # 4096 different pairs: the 256 with their matches rotated by 1 .. 15 places
                    sel = [(np.roll(a, j // 256, 0), np.roll(b, j // 256, 0)) for j, (a, b) in enumerate(sel)]
                ptr = (n * np.arange(npair + 1)).astype(np.int32)
                xa = np.ascontiguousarray(np.concatenate([a for a, _ in sel]))
                xb = np.ascontiguousarray(np.concatenate([b for _, b in sel]))
                for _ in range(args.warmup):
                    r = capi.verify_pairs(ptr, xa, xb)
                wall = []
                for _ in range(repeat):
                    t0 = time.perf_counter()
                    r = capi.verify_pairs(ptr, xa, xb)
                    wall.append(1e3 * (time.perf_counter() - t0))
                host_ms = None
                if npair <= min(args.host_pairs, 256):
                    p = subprocess.run([exe, "time"], input="\n".join(text[:npair]) + "\n", capture_output=True, text=True, check=True)
                    host_ms = float(p.stderr.split()[-1])
                    same = all(H.parse_pair(ln, n)["num_trials"] == int(r["num_trials"][j]) for j, ln in enumerate(p.stdout.strip().split("\n")))
                else:
                    same = None
                rows.append((npair, n, share, int((r["status"] == 1).sum()), int(r["accepted"].sum()), float(np.median(wall)), float(np.min(wall)),
                             float(np.max(wall)), float(r["num_trials"].mean()), float(r["num_inliers"].mean()), host_ms, same))
                print(rows[-1], flush=True)
    lines = ["# Batched pair verification (`xrsfm_ba_verify_pairs`): time per call and measured deviations", "",
             "Measured on one MI355X with the library of the commit that added the call, one session, `python tools/pair_verify_timing.py "
             "--repeat %d` (%d warm-up calls, then the median of %d calls; smallest and largest call beside it).  Wall time: host clock" % (repeat, args.warmup, repeat),
             "around the blocking call through the ctypes wrapper: argument checks, the rows of the adaptive trial bound, staging, one upload,",
             "one launch of `k_verify_pairs` (one 256-thread workgroup per pair; the septuples are drawn on the device), one read-back.",
             "Host column: the sequential driver of `tests/fund_host_driver.py` (the same `ba_fund_scan.h` / `ba_fund_geom.h`, `g++ -O2`, one core),",
             "run once on the same pairs, time of the solves only; it is not run for 4096 pairs (its time grows linearly with the pairs).", "",
             "| pairs | matches per pair | outlier share | models found | accepted | wall ms (median) | min | max | mean trials | mean inliers | host driver ms (one core) | host / GPU | same trial counts |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    slower = []
    for npair, n, share, found, acc, med, lo, hi, tr, inl, host, same in rows:
        hs = "-" if host is None else f"{host:.1f}"
        ratio = "-" if host is None else f"{host / med:.1f}"
        lines.append(f"| {npair} | {n} | {share} | {found} | {acc} | {med:.3f} | {lo:.3f} | {hi:.3f} | {tr:.0f} | {inl:.0f} | {hs} | {ratio} | {'-' if same is None else same} |")
        if npair == 256 and host is not None and med > host:
            slower.append((n, share))
    lines += ["", "The only condition set for this step: the 256-pair batches must not be slower than the host run.  " +
              ("It holds in every row." if not slower else "It does NOT hold for (matches, outlier share) = %s." % slower),
              "Nobody had measured this step here before; no speed bar is set, and the parent commit has no such call to compare with.",
              "Not measured: kernel time apart from the call (no HIP events around the launch, no rocprofv3 pass), the share of the blocks",
              "(a)-(d) and of the sampler, other workgroup sizes, hardware counters.", ""]
    if not args.no_deviations:
        from tests.test_fund_cpu import run_pair_driver
        ext, fr, E = Y.reference("longdouble"), Y.fragile(), Y.entries()
        worst, worst_host = 0.0, 0.0
        hostres = run_pair_driver(exe, list(range(len(E))))
        for o, idx in Y.option_groups().items():
            ptr, xa, xb = Y.arrays(idx)
            r = capi.verify_pairs(ptr, xa, xb, capi.verify_pairs_options(**dict(o)))
            for j, k in enumerate(idx):
                if k < Y.n_main() and ext[k]["status"] == 1 and not fr[k] and r["status"][j] == 1:
                    worst = max(worst, Y.deviation(r["F"][j], ext[k]))
                    worst_host = max(worst_host, Y.deviation(hostres[k]["F"], ext[k]))
        lines += ["## Deviation from the extended-precision yardstick", "",
                  "Over the non-fragile status-1 pairs of the main test catalogue (tests/fund_yardstick.py, every option set; deviation = max |F - F_ext|,",
                  "both of unit Frobenius norm with the largest entry positive):", "",
                  "| | largest deviation |", "|---|---|",
                  f"| float64 restatement of the yardstick | {Y.restatement_deviation():.3e} |",
                  f"| sequential host driver (the library's headers, g++ -O2) | {worst_host:.3e} |",
                  f"| library (GPU) | {worst:.3e} |",
                  f"| tight bar of the tests: {Y.TIGHT_FACTOR} x RESTATEMENT_DEVIATION ({Y.RESTATEMENT_DEVIATION:.1e}) | {Y.TIGHT_BAR:.1e} |", "",
                  f"Fragile pairs of the main catalogue: {Y.fragile_share():.1%} (cap {Y.FRAGILE_CAP:.0%}).", ""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
