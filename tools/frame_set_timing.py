"""Time the device-resident frame sets against the chain of entry points they replace and write profiles/frame_set.md.

Rows: 16 and 64 images of 1024 x 768 (the images of tools/keypoint_timing.py), default options, all pairs (120 / 2016), cut into two
halves: the first call and the call that follows it on the same frames, as ExpansionAndMatching makes them.

  A  extract_features on host buffers (floats=False: the set holds no float descriptors either)  |  frames_from_images, no download
  B  match_descriptors + matched_points + verify_pairs on the first half of the pairs            |  frames_match on a new set
  C  the same three calls on the other half                                                      |  frames_match on the same set

Host clocks around blocking calls (each ends in a synchronise inside the library), through the Python wrappers on both sides.  The
two sides alternate within one process; per side the median of --repeat rounds after --warmup rounds and the spread (min / max).
The comparator is this library's own existing entry points: this change does not touch what they compute.  The condition per row:
the new path's median is not above the comparator's median by more than the comparator's own spread (max - min).

One further round in a child process with XRSFM_BA_SIFT_TIMING and XRSFM_BA_MATCH_TIMING set gives the event times of the two new
kernels beside k_siftd_desc and the matching kernels.

    python tools/frame_set_timing.py [--repeat 5] [--warmup 1] [--out profiles/frame_set.md]
"""
import argparse
import importlib.util
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _keypoint_timing():
    spec = importlib.util.spec_from_file_location("keypoint_timing", os.path.join(ROOT, "tools", "keypoint_timing.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def all_pairs(n):
    pa, pb = np.triu_indices(n, 1)
    return pa.astype(np.int32), pb.astype(np.int32)


def halves(n):
    pa, pb = all_pairs(n)
    return (pa[0::2].copy(), pb[0::2].copy()), (pa[1::2].copy(), pb[1::2].copy())


def chain(capi, dptr, desc, xy, pa, pb, mo, vo):
    r = capi.match_descriptors(dptr, desc, pa, pb, mo)
    xa, xb = capi.matched_points(r, dptr, xy, pa, pb)
    r.update(capi.verify_pairs(r["match_ptr"].astype(np.int32), xa, xb, vo))
    return r


def clock(f):
    t0 = time.perf_counter()
    out = f()
    return 1e3 * (time.perf_counter() - t0), out


def stats(v):
    return dict(median=float(np.median(v)), lo=float(min(v)), hi=float(max(v)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frame_set.md"))
    ap.add_argument("--sizes", default="16,64")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    import torch  # noqa: F401
    from tests import sift_yardstick as Y
    from xrsfm_amd import capi
    if capi.device_count() <= 0:
        raise SystemExit("no GPU: nothing here can be measured without one")
    K = _keypoint_timing()
    so, do, mo, vo = capi.sift_options(), capi.sift_desc_options(), capi.match_options(), capi.verify_pairs_options()
    if args.child:                      # one round of the new path with the kernel timing on (the variables are read per call)
        n = int(args.child)
        imgs = K.make_images(Y, n, 1024, 768)
        (pa1, pb1), (pa2, pb2) = halves(n)
        with capi.frames_from_images(imgs, so, do) as fs:          # (loads the code objects)
            capi.frames_match(fs, pa1, pb1, mo, vo)
        os.environ["XRSFM_BA_SIFT_TIMING"] = "1"
        os.environ["XRSFM_BA_MATCH_TIMING"] = "1"
        with capi.frames_from_images(imgs, so, do) as fs:
            capi.frames_match(fs, pa1, pb1, mo, vo)
            capi.frames_match(fs, pa2, pb2, mo, vo)
        return
    rows = []
    for n in (int(x) for x in args.sizes.split(",")):
        imgs = K.make_images(Y, n, 1024, 768)
        (pa1, pb1), (pa2, pb2) = halves(n)
        res = capi.extract_features(imgs, so, do, floats=False)
        cap = sum(len(r["loc"]) for r in res)                       # (so that every timed extract_features is ONE C call)
        desc, dptr, xy = capi.feature_frames(res)
        t = {k: [] for k in ("A_old", "A_new", "B_old", "B_new", "C_old", "C_new")}
        same = True
        for rnd in range(args.warmup + args.repeat):
            a_old, _ = clock(lambda: capi.extract_features(imgs, so, do, capacity=cap, floats=False))
            a_new, fs = clock(lambda: capi.frames_from_images(imgs, so, do))
            b_old, w1 = clock(lambda: chain(capi, dptr, desc, xy, pa1, pb1, mo, vo))
            b_new, g1 = clock(lambda: capi.frames_match(fs, pa1, pb1, mo, vo))
            c_old, w2 = clock(lambda: chain(capi, dptr, desc, xy, pa2, pb2, mo, vo))
            c_new, g2 = clock(lambda: capi.frames_match(fs, pa2, pb2, mo, vo))
            info = capi.frames_info(fs)
            fs.close()
            for g, w in ((g1, w1), (g2, w2)):                       # (faster and different is not faster)
                same = same and all(np.array_equal(np.ascontiguousarray(g[k]).view(np.uint8), np.ascontiguousarray(w[k]).view(np.uint8)) for k in w)
            if rnd >= args.warmup:
                for k, v in zip(t, (a_old, a_new, b_old, b_new, c_old, c_new)):
                    t[k].append(v)
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(n)], capture_output=True, text=True, check=True)
        ev = dict(order=float(re.search(r"frames timing: order ([\d.]+) ms", out.stderr).group(1)),
                  desc=float(re.search(r"sift descriptor timing: .* desc ([\d.]+) ms", out.stderr).group(1)))
        mt = re.findall(r"frames match timing: dots ([\d.]+) ms, select ([\d.]+) ms, gather ([\d.]+) ms, verify ([\d.]+) ms", out.stderr)
        ev.update(match=[tuple(float(x) for x in m) for m in mt])
        rows.append(dict(n=n, keys=int(info["key_ptr"][-1]), bytes=info["device_bytes"], matches=(len(w1["matches"]), len(w2["matches"])),
                         pairs=(len(pa1), len(pa2)), same=same, ev=ev, **{k: stats(v) for k, v in t.items()}))
        print(rows[-1], flush=True)
    with open(args.out, "w") as f:
        f.write("# Device-resident frame sets against the chain of entry points: measured times\n\n")
        f.write("Written by `tools/frame_set_timing.py` (what every row is: its docstring).  Images of 1024 x 768, default options, one MI355X; host clocks around\n"
                "blocking calls, the two sides alternating in one process, median (min .. max) of %d rounds after %d.  \"within\": the new median is not above the\n"
                "comparator's median by more than the comparator's spread (max - min).\n\n" % (args.repeat, args.warmup))
        f.write("| images | row | what | comparator ms | frame set ms | ratio | within |\n|---|---|---|---|---|---|---|\n")
        what = dict(A="extract_features (host buffers) / frames_from_images", B="chain / frames_match, first half of the pairs, new set",
                    C="chain / frames_match, other half, same set")
        for r in rows:
            for row in "ABC":
                o, nw = r[row + "_old"], r[row + "_new"]
                ok = nw["median"] <= o["median"] + (o["hi"] - o["lo"])
                f.write("| %d | %s | %s | %.2f (%.2f .. %.2f) | %.2f (%.2f .. %.2f) | %.2f | %s |\n" % (
                    r["n"], row, what[row], o["median"], o["lo"], o["hi"], nw["median"], nw["lo"], nw["hi"], o["median"] / nw["median"], "yes" if ok else "NO"))
        f.write("\n| images | key points | device bytes | bytes per key point | pairs (B, C) | matches (B, C) | outputs bit-equal in every round |\n|---|---|---|---|---|---|---|\n")
        for r in rows:
            f.write("| %d | %d | %d | %.1f | %d, %d | %d, %d | %s |\n" % (r["n"], r["keys"], r["bytes"], r["bytes"] / max(r["keys"], 1), r["pairs"][0], r["pairs"][1],
                                                                   r["matches"][0], r["matches"][1], "yes" if r["same"] else "NO"))
        f.write("\nEvent times of one further round (a child process with `XRSFM_BA_SIFT_TIMING` and `XRSFM_BA_MATCH_TIMING`), ms:\n\n"
                "| images | k_frames_order | k_siftd_desc | call | k_match_dots | k_match_select | k_frames_gather | k_verify_pairs |\n|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            for call, m in zip(("B", "C"), r["ev"]["match"]):
                f.write("| %d | %.4f | %.4f | %s | %.4f | %.4f | %.4f | %.4f |\n" % ((r["n"], r["ev"]["order"], r["ev"]["desc"], call) + m))
        f.write("\nThe bytes per key point are those of the block held from the allocation cache (its size class), above the 169 the arrays need\n"
                "(16 key + 128 descriptor + 4 term + 16 loc + 1 sign + 4 orientation).\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
