"""Time xrsfm_ba_absolute_pose and write profiles/absolute_pose.md: wall time per call for 1 / 16 / 256 frames of 100 and 1000
correspondences at outlier shares 0.2 and 0.7, and the two measured pose deviations of the test catalogue (the float64 restatement
of tests/pose_yardstick.py and the library, each against the extended-precision run).

Wall time: host clock around the blocking C call through the ctypes wrapper (checks, dyn rows and sample triples on the host,
staging, one upload, one launch, one read-back), the median of --repeat calls (at least 20) after --warmup calls.  Frames: random
pose, points 3-9 in front of the camera, 0.1 x max_error of noise on the inliers, outliers uniform over the image; every frame of a
call is different.

    python tools/absolute_pose_timing.py [--repeat 20] [--warmup 3] [--out profiles/absolute_pose.md] [--no-deviations]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "absolute_pose.md"))
    ap.add_argument("--no-deviations", action="store_true")
    args = ap.parse_args()
    import torch  # noqa: F401  (first, so that both share one HIP runtime)
    from xrsfm_amd import capi
    from tests import pose_yardstick as Y
    if capi.device_count() < 1:
        raise SystemExit("no HIP device visible")
    repeat = max(args.repeat, 20)
    rows = []
    for n in (100, 1000):
        for share in (0.2, 0.7):
            rng = np.random.default_rng(1000 * n + int(10 * share))
            frames = [Y._frame(rng, n, share, "timing") for _ in range(256)]
            for nf in (1, 16, 256):
                ptr = (n * np.arange(nf + 1)).astype(np.int32)
                xy = np.ascontiguousarray(np.concatenate([f["xy"] for f in frames[:nf]]))
                X = np.ascontiguousarray(np.concatenate([f["X"] for f in frames[:nf]]))
                for _ in range(args.warmup):
                    r = capi.absolute_pose(ptr, xy, X)
                wall = []
                for _ in range(repeat):
                    t0 = time.perf_counter()
                    r = capi.absolute_pose(ptr, xy, X)
                    wall.append(1e3 * (time.perf_counter() - t0))
                err = max((float(np.abs(np.asarray(Y.quat_to_mat(r["q"][j]), np.float64) - frames[j]["R"]).max()) for j in range(nf) if r["status"][j] == 1), default=0.0)
                rows.append((nf, n, share, int((r["status"] == 1).sum()), float(np.median(wall)), float(np.min(wall)), float(np.max(wall)),
                             float(r["num_trials"].mean()), float(r["num_inliers"].mean()), err))
                print(rows[-1], flush=True)
    lines = ["# Batched absolute pose (`xrsfm_ba_absolute_pose`): time per call and measured deviations", "",
             "Measured on one MI355X with the library of the commit that added the call, one session, `python tools/absolute_pose_timing.py "
             "--repeat %d` (%d warm-up calls, then the median of %d calls; smallest and largest call beside it).  Wall time: host clock" % (repeat, args.warmup, repeat),
             "around the blocking call through the ctypes wrapper: argument checks, the rows of the adaptive trial bound and the sample",
             "triples on the host (585 triples per frame at the default options), staging, one upload, one launch of `k_pnp_frames` (one",
             "256-thread workgroup per frame), one read-back.  No kernel-only time was taken (no HIP events around the launch, no rocprofv3 pass).", "",
             "| frames | correspondences per frame | outlier share | poses found | wall ms (median) | min | max | mean trials | mean inliers | largest rotation error against the generating pose |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for nf, n, share, found, med, lo, hi, tr, inl, err in rows:
        lines.append(f"| {nf} | {n} | {share} | {found} | {med:.3f} | {lo:.3f} | {hi:.3f} | {tr:.0f} | {inl:.0f} | {err:.1e} |")
    lines += ["", "For scale: one `xrsfm_ba_refine_pose` call, the step that follows in `RegisterImage`, takes 0.11 ms (README, the row of the",
              "pose refinement).  Nobody had measured a pose RANSAC here before; no speed bar is set, and the parent commit has no such call to compare with.",
              "Not measured: kernel time apart from the call, the share of the blocks (a)-(d), other workgroup sizes, hardware counters.", ""]
    if not args.no_deviations:
        worst = 0.0
        for name in Y.OPTION_SETS:
            ext, fr, idx = Y.reference("longdouble", name), Y.fragile(name), Y.frames_of(name)
            ptr, xy, X = Y.arrays(idx)
            r = capi.absolute_pose(ptr, xy, X, capi.absolute_pose_options(**dict(Y.OPTION_SETS[name])))
            for j, k in enumerate(idx):
                if ext[k]["status"] == 1 and not fr[k] and r["status"][j] == 1:
                    worst = max(worst, Y.deviation(np.asarray(Y.quat_to_mat(r["q"][j]), np.float64), r["t"][j], ext[k]))
        lines += ["## Deviation from the extended-precision yardstick", "",
                  "Over the non-fragile status-1 frames of the test catalogue (tests/pose_yardstick.py, every option set; deviation = the larger of",
                  "max |R - R_ext| and max |t - t_ext| / max(1, |t_ext|)):", "",
                  "| | largest deviation |", "|---|---|",
                  f"| float64 restatement of the yardstick | {Y.restatement_deviation():.3e} |",
                  f"| library (GPU) | {worst:.3e} |",
                  f"| tight bar of the tests: {Y.TIGHT_FACTOR} x RESTATEMENT_DEVIATION ({Y.RESTATEMENT_DEVIATION:.1e}) | {Y.TIGHT_BAR:.1e} |", "",
                  f"Fragile frames of the catalogue: {Y.fragile_share():.1%} (cap {Y.FRAGILE_CAP:.0%}).  Both largest deviations belong to the exactly planar frame,",
                  "whose returned model is a P3P sample model (EPnP has no model there): its quartic root is the ill-conditioned quantity.", ""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
