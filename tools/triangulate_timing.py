"""Time xrsfm_ba_triangulate_tracks on two shapes: a frame's worth (2 000 tracks of 2-8 observations) and a map's worth (500 000
tracks of 2-30 observations, 20 % outlier observations: config 4's point count).

Per shape: the wall time of the call (host clock around the blocking C call through the ctypes wrapper) and the HIP-event time of
k_tri_tracks (the library's own events around the launch, XRSFM_BA_TRI_TIMING), each the median of --repeat calls (at least 20) after
--warmup calls, and the trials per second of the kernel (sum of the reported num_trials over the kernel time).  With --phases the
"tri_phases" build of the library is used (XBA_TRI_PHASES: every wave counts the clock ticks of its blocks) and the shares of the
blocks (a) sample models, (b) supports, (c) scan, (d) refits are printed; that build's times are not the product's.

    python tools/triangulate_timing.py [--repeat 20] [--warmup 3] [--phases] [--shape frame|map|both]
"""
import argparse
import os
import re
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _stderr_of(f):
    """Run f() and return (result, what the process wrote to file descriptor 2 meanwhile): the library prints from C."""
    sys.stderr.flush()
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        saved = os.dup(2)
        os.dup2(tmp.fileno(), 2)
        try:
            r = f()
        finally:
            os.dup2(saved, 2); os.close(saved)
        tmp.seek(0)
        return r, tmp.read().decode(errors="replace")


def make_shape(n_tracks, lo, hi, outlier_frac, n_cams, spacing, seed):
    """Cameras on a line along x looking down +z with small rotations; every track sees a random window of consecutive cameras;
    1e-3 noise on the normalised coordinates, outliers displaced by up to +-0.2."""
    rng = np.random.default_rng(seed)
    w = rng.uniform(-0.05, 0.05, (n_cams, 3))
    ang = np.linalg.norm(w, axis=1)
    q = np.concatenate([w * (np.sin(ang / 2) / ang)[:, None], np.cos(ang / 2)[:, None]], axis=1)
    x, y, z, s = q.T
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - s * z), 2 * (x * z + s * y), 2 * (x * y + s * z), 1 - 2 * (x * x + z * z), 2 * (y * z - s * x),
                  2 * (x * z - s * y), 2 * (y * z + s * x), 1 - 2 * (x * x + y * y)], axis=1).reshape(-1, 3, 3)
    c = np.stack([spacing * np.arange(n_cams), rng.uniform(-0.1, 0.1, n_cams), rng.uniform(-0.1, 0.1, n_cams)], axis=1)
    t = -np.einsum("nrc,nc->nr", R, c)
    length = rng.integers(lo, hi + 1, n_tracks)
    ptr = np.zeros(n_tracks + 1, np.int32)
    ptr[1:] = np.cumsum(length)
    trk = np.repeat(np.arange(n_tracks), length)
    start = rng.integers(0, n_cams - hi, n_tracks)
    cam = (start[trk] + (np.arange(ptr[-1]) - ptr[:-1][trk])).astype(np.int32)
    X = np.stack([c[start + length // 2, 0] + rng.uniform(-1, 1, n_tracks), rng.uniform(-1, 1, n_tracks), rng.uniform(4, 12, n_tracks)], axis=1)
    pc = np.einsum("nrc,nc->nr", R[cam], X[trk]) + t[cam]
    xy = pc[:, :2] / pc[:, 2:3] + rng.normal(0, 1e-3, (len(cam), 2))
    out = rng.random(len(cam)) < outlier_frac
    xy[out] += rng.uniform(-0.2, 0.2, (int(out.sum()), 2))
    return np.ascontiguousarray(q), np.ascontiguousarray(t), ptr, cam, np.ascontiguousarray(xy)


SHAPES = {"frame": dict(n_tracks=2000, lo=2, hi=8, outlier_frac=0.0, n_cams=40, spacing=0.5, seed=1),
          "map": dict(n_tracks=500000, lo=2, hi=30, outlier_frac=0.2, n_cams=1000, spacing=0.25, seed=2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shape", default="both", choices=["frame", "map", "both"])
    ap.add_argument("--phases", action="store_true", help="use the tri_phases build and print the share of each block of the kernel")
    args = ap.parse_args()
    import torch  # noqa: F401  (first, so that both share one HIP runtime)
    from xrsfm_amd import _build, capi
    if args.phases:
        os.environ["XRSFM_BA_LIB"] = _build.build_lib(variant="tri_phases")
    if capi.device_count() < 1:
        raise SystemExit("no HIP device visible")
    os.environ["XRSFM_BA_TRI_TIMING"] = "1"
    print("| shape | tracks | observations | created | wall ms (median of %d) | kernel ms (HIP events, median) | trials | trials / s |" % max(args.repeat, 20))
    print("|---|---|---|---|---|---|---|---|")
    for name in (("frame", "map") if args.shape == "both" else (args.shape,)):
        q, t, ptr, cam, xy = make_shape(**SHAPES[name])
        for _ in range(args.warmup):
            _stderr_of(lambda: capi.triangulate_tracks(q, t, ptr, cam, xy))
        wall, kern, ticks = [], [], None
        for _ in range(max(args.repeat, 20)):
            t0 = time.perf_counter()
            r, err = _stderr_of(lambda: capi.triangulate_tracks(q, t, ptr, cam, xy))
            wall.append(1e3 * (time.perf_counter() - t0))
            m = re.search(r"kernel_ms ([0-9.]+) ticks_a (\d+) ticks_b (\d+) ticks_c (\d+) ticks_d (\d+)", err)
            kern.append(float(m.group(1)))
            ticks = [int(m.group(k)) for k in range(2, 6)]
        trials = int(r["num_trials"].sum())
        k_med = float(np.median(kern))
        print(f"| {name} | {len(ptr) - 1} | {len(cam)} | {int((r['status'] == 1).sum())} | {np.median(wall):.3f} | {k_med:.3f} | {trials} | "
              f"{trials / (k_med * 1e-3):.3e} |", flush=True)
        if args.phases and sum(ticks) > 0:
            tot = float(sum(ticks))
            print(f"|   {name}: share of wave ticks | (a) sample models {ticks[0] / tot:.1%} | (b) supports {ticks[1] / tot:.1%} | (c) scan {ticks[2] / tot:.1%} | "
                  f"(d) refits {ticks[3] / tot:.1%} | | | |", flush=True)


if __name__ == "__main__":
    main()
