"""Time xrsfm_ba_detect_keypoints and write profiles/keypoint_detect.md: one call of 1, 16 and 64 images of 1024 x 768 and one of
3200 x 2400, first_octave -1, each row with

  wall     host clock around the blocking C call on host buffers (checks, staging, upload, launches, the read-back of the counts,
           budget and prefix sum, the emit pass, the read-back and ordering of the keypoints), the median of --repeat calls after
           --warmup calls;
  kernels  XRSFM_BA_SIFT_TIMING makes the library print the time of every kernel from events on its stream (summed over octaves
           and chunks), from one further call;
  floor    the bytes that must move per level, read + write of the planes actually touched, at 8 TB/s: a level filter reads G[i]
           and writes G[i+1] and D[i] (12 bytes per pixel), the initial smoothing 8, the base plane 0.25 or 1 read and 4 written,
           the down-sample 4 written per pixel of the new octave (its reads are every second pixel of every second row: whole
           lines move, counted as the source rows touched), the key pass the five DoG planes once (each of the three launches'
           levels reads three);
  CPU      the -O2 one-core build of the host driver (tests/sift_host_driver.py: ba_sift_rule.h, sequential, whole images), on the
           same images, for the rows up to 16 images of 1024 x 768 (per image beyond that).

Images: the alternating blob lattices of the test catalogue (tests/sift_yardstick.py) at the row's size, pitches 4 to 40 px.

    python tools/keypoint_timing.py [--repeat 5] [--warmup 1] [--out profiles/keypoint_detect.md]
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = ("base", "init", "filter0", "filter1", "filter2", "filter3", "filter4", "down", "count", "emit")


def make_images(Y, n, w, h, seed=100):
    rows = [(1, [4, 5, 6.5, 8]), (1, [10, 13, 17, 22]), (1.5, [28, 34, 40])]
    distinct = [Y.blobs(w, h, seed + k, Y._bands(w, h, rows)) for k in range(min(n, 4))]          # (four contents in turn)
    return [distinct[k % len(distinct)] for k in range(n)]


def floor_ms(Y, w, h, n, first_octave=-1, num_octaves=4, tbs=8e12):
    """kernel -> milliseconds at tbs bytes per second"""
    geo = Y.geometry(w, h, first_octave, num_octaves)
    px = [gw * gh for gw, gh in geo]
    b = dict.fromkeys(KERNELS, 0.0)
    b["base"] = (w & ~3) * h + 4 * px[0]
    b["init"] = 8 * px[0]
    for i in range(5):
        b["filter%d" % i] = 12 * sum(px)
    b["down"] = sum(4 * px[o] + 4 * geo[o - 1][0] * geo[o][1] for o in range(1, len(geo)))
    b["count"] = 3 * 3 * 4 * sum(px)
    b["emit"] = b["count"]
    return {k: 1e3 * n * v / tbs for k, v in b.items()}


def kernel_times(text):
    m = re.search(r"sift timing: base ([\d.]+) ms, init ([\d.]+) ms, filter ([\d.]+) ([\d.]+) ([\d.]+) ([\d.]+) ([\d.]+) ms, down ([\d.]+) ms, count ([\d.]+) ms, "
                  r"emit ([\d.]+) ms, chunks (\d+)", text)
    return dict(zip(KERNELS, (float(x) for x in m.groups()[:10]))), int(m.group(11))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "keypoint_detect.md"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    import torch  # noqa: F401
    from tests import sift_host_driver as H
    from tests import sift_yardstick as Y
    from xrsfm_amd import capi
    if args.child:                      # one call with the kernel timing on, in a fresh process (the variable is read per call)
        n, w, h = (int(x) for x in args.child.split(","))
        imgs = make_images(Y, n, w, h)
        os.environ.pop("XRSFM_BA_SIFT_TIMING", None)
        capi.detect_keypoints([Y.image("c64x48")], capi.sift_options())         # (loads the code object: 17 ms on the first launch)
        cap = sum(len(r["loc"]) for r in capi.detect_keypoints(imgs, capi.sift_options()))
        os.environ["XRSFM_BA_SIFT_TIMING"] = "1"
        capi.detect_keypoints(imgs, capi.sift_options(), capacity=cap)
        return
    tmp = tempfile.mkdtemp()
    exe = H.build(tmp, flags=["-O2"])
    rows, lines = ((1, 1024, 768), (16, 1024, 768), (64, 1024, 768), (1, 3200, 2400)), []
    cpu_per_image = {}
    for n, w, h in rows:
        imgs = make_images(Y, n, w, h)
        opt = capi.sift_options()
        cap = sum(len(r["loc"]) for r in capi.detect_keypoints(imgs, opt))      # (so that every timed call is ONE C call)
        for _ in range(args.warmup):
            capi.detect_keypoints(imgs, opt, capacity=cap)
        wall = []
        for _ in range(args.repeat):
            t0 = time.perf_counter()
            res = capi.detect_keypoints(imgs, opt, capacity=cap)
            wall.append(1e3 * (time.perf_counter() - t0))
        env = dict(os.environ, XRSFM_BA_SIFT_TIMING="1")
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "%d,%d,%d" % (n, w, h)], env=env, capture_output=True, text=True, check=True)
        kt, chunks = kernel_times(out.stderr)
        fl = floor_ms(Y, w, h, n)
        if (w, h) not in cpu_per_image or n == 16:
            m = min(n, 16)
            _, ms = H.run(exe, tmp, imgs[:m], [Y.options()] * m, timing=True)
            cpu_per_image[(w, h)] = ms / m
            cpu, measured = ms * n / m, m == n
        else:
            cpu, measured = cpu_per_image[(w, h)] * n, False
        keys = sum(len(r["loc"]) for r in res)
        lines.append(dict(n=n, w=w, h=h, wall=float(np.median(wall)), kt=kt, fl=fl, chunks=chunks, cpu=cpu, measured=measured, keys=keys))
        print(lines[-1], flush=True)
    dev = Y.measured_deviation()
    with open(args.out, "w") as f:
        f.write("# xrsfm_ba_detect_keypoints: measured times and deviations\n\n")
        f.write("Written by `tools/keypoint_timing.py` (what every column is: its docstring).  first_octave -1, four octaves, the defaults of\n"
                "`xrsfm_ba_sift_options_default`; one MI355X; median of %d calls after %d.\n\n" % (args.repeat, args.warmup))
        f.write("| images | size | keypoints | wall ms | kernels ms | floor ms (8 TB/s) | chunks | CPU one core ms | CPU / wall |\n|---|---|---|---|---|---|---|---|---|\n")
        for r in lines:
            f.write("| %d | %d x %d | %d | %.2f | %.3f | %.3f | %d | %.0f%s | %.1f |\n" % (
                r["n"], r["w"], r["h"], r["keys"], r["wall"], sum(r["kt"].values()), sum(r["fl"].values()), r["chunks"], r["cpu"],
                "" if r["measured"] else " (scaled from %d)" % min(r["n"], 16), r["cpu"] / r["wall"]))
        f.write("\nPer kernel, measured ms / floor ms (summed over the octaves and chunks of the call):\n\n| images | size | " + " | ".join(KERNELS) + " |\n|---|---|" + "---|" * len(KERNELS) + "\n")
        for r in lines:
            f.write("| %d | %d x %d | " % (r["n"], r["w"], r["h"]) + " | ".join("%.3f / %.3f" % (r["kt"][k], r["fl"][k]) for k in KERNELS) + " |\n")
        ok = [r for r in lines if (r["n"], r["w"]) == (16, 1024)][0]
        f.write("\nThe condition of DESIGN.md 5m (the call on 16 images of 1024 x 768 is not slower than the one-core host build): wall %.2f ms against %.0f ms: %s.\n" % (
            ok["wall"], ok["cpu"], "holds" if ok["wall"] <= ok["cpu"] else "DOES NOT HOLD"))
        f.write("\nThe wall time includes the wrapper's packing of the images into one buffer and its slicing of the result.  Where the time goes and what is\n"
                "known about it: the filter kernels run at several times their bandwidth floor.  Per output pixel a level of W taps reads 2 W floats from LDS and\n"
                "issues 2 W FMAs beside its 12 bytes of HBM traffic, and the horizontal pass also filters the halo rows, (32 + W - 1) / 32 of the tile; with W = 25 that\n"
                "is 44 + 25 = 69 FMAs and as many LDS reads per pixel.  NOT measured: LDS bandwidth or bank-conflict counters, VALU utilisation, occupancy achieved, the share of\n"
                "the scalar tap loads.  Nothing was tuned on a guess; a register-blocked vertical pass (several rows per thread, each LDS value used for several\n"
                "outputs) is the obvious candidate once counters say LDS reads bind.  The key passes read three DoG planes per level (nine plane reads per octave\n"
                "where five distinct planes exist) and decide every candidate twice (count, emit).\n")
        f.write("\n## The measured deviations behind the 16x bars\n\nThe float32 restatement of `tests/sift_yardstick.py` against its longdouble rule over the catalogue (CPU, no GPU involved):\n"
                "Gaussian levels %.3e, DoG levels %.3e, offsets (dx, dy, ds) %.3e, X and Y %.3e px, S %.3e.  A tested implementation must stay within 16 times the last\n"
                "three on the keypoints found by both.\n" % (dev["gauss"], dev["dog"], dev["off"], dev["xy"], dev["s"]))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
