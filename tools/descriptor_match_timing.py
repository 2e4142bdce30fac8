"""Time xrsfm_ba_match_descriptors and write profiles/descriptor_match.md: wall time per call for 1 / 16 / 256 / 1024 pairs of
2048 x 2048, 4096 x 4096 and 8192 x 8192 descriptors, beside the PyTorch formulation of the same matcher on the same device (the
comparator) and, at the smallest size, the sequential host driver (tests/match_host_driver.py: ba_match_rule.h, g++ -O2, one core).

Wall time: host clock around the blocking call through the ctypes wrapper (checks, staging, upload, launches, read-back, packing),
the median of --repeat calls (at least 20) after --warmup calls.  Frames: the synthetic SIFT-like generator of the test catalogue;
frame f + 1 holds perturbed copies of two thirds of frame f, the pairs of a call are (f, f + 1 + k) over a ring of frames, so a frame
takes part in many pairs and is prepared once per call.

Comparator: fp32 matmul of the descriptors (exact: every partial sum is an integer below 2^24), topk(2) along both axes, the same
table, test and mutual check, in chunks of 16 pairs (bmm), from descriptors in host memory to matches in host memory like the
library call.  Its matches are asserted equal to the library's.  It runs where the condition of DESIGN.md 5l needs it and wherever
it is cheap: every single pair, and 16 and 256 pairs of 2048 and 4096 (median of --comparator-repeat calls from 256 pairs on).

Kernel time: XRSFM_BA_MATCH_TIMING makes the library print the times of its kernels from events on its stream; beside it the time
the int8 matrix instructions alone would take: 2 (n_a / 16) (n_b / 16) instructions of 16 cycles per pair over 4 SIMDs of every CU.

    python tools/descriptor_match_timing.py [--repeat 20] [--warmup 2] [--comparator-repeat 5] [--out profiles/descriptor_match.md]
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


def make_frames(Y, n_frames, n, seed):
    rng = np.random.default_rng(seed)
    frames = [Y.sift_like(rng, n)]
    for _ in range(n_frames - 1):
        frames.append(Y.related(rng, frames[-1], n)[0])
    return frames


def make_pairs(n_frames, n_pairs):
    pa = np.arange(n_pairs, dtype=np.int32) % n_frames
    pb = (pa + 1 + np.arange(n_pairs, dtype=np.int32) // n_frames) % n_frames
    return pa, pb


def comparator(torch, desc_host, n, pa, pb, tab, opt, chunk=16):
    """the PyTorch-ROCm formulation: list of matches [k][2] per pair (numpy, on the host)"""
    dev = torch.device("cuda")
    D = torch.from_numpy(desc_host).to(dev).float().reshape(-1, n, 128)           # every frame converted once
    ar = torch.arange(n, device=dev)
    maxd, ratio = float(np.float32(opt.max_distance)), float(np.float32(opt.max_ratio))
    out = []

    def side(S, dim):
        v, i = S.topk(2, dim=dim)
        v0, v1, i0 = v.select(dim, 0), v.select(dim, 1), i.select(dim, 0)
        d0, d1 = tab[v0.long().clamp(max=1 << 18)], tab[v1.long().clamp(max=1 << 18)]
        keep = (d0 < maxd) & (d0 < d1 * ratio) & (v0 > 0)
        return torch.where(keep, i0, torch.full_like(i0, -1))
    for c0 in range(0, len(pa), chunk):
        A, B = D[torch.from_numpy(pa[c0:c0 + chunk]).long().to(dev)], D[torch.from_numpy(pb[c0:c0 + chunk]).long().to(dev)]
        S = torch.bmm(A, B.transpose(1, 2))
        rm, cm = side(S, 2), side(S, 1)
        ok = rm >= 0
        if opt.mutual_best:
            ok &= torch.gather(cm, 1, rm.clamp(min=0)) == ar
        rm_h, ok_h = rm.cpu().numpy(), ok.cpu().numpy()
        for q in range(len(rm_h)):
            i = np.flatnonzero(ok_h[q])
            out.append(np.stack([i, rm_h[q][i]], 1).astype(np.int32))
    return out


def timed(fn, warmup, repeat):
    for _ in range(warmup):
        r = fn()
    wall = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        r = fn()
        wall.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(wall)), r


def kernel_times(fn):
    """one call with XRSFM_BA_MATCH_TIMING set; the library's stderr line -> (prep, dots, select) in ms, launches"""
    with tempfile.TemporaryFile(mode="w+") as f:
        sys.stderr.flush()
        saved = os.dup(2)
        os.environ["XRSFM_BA_MATCH_TIMING"] = "1"
        try:
            os.dup2(f.fileno(), 2)
            fn()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
            del os.environ["XRSFM_BA_MATCH_TIMING"]
        f.seek(0)
        m = re.search(r"prep ([\d.]+) ms, dots ([\d.]+) ms, select ([\d.]+) ms, launches (\d+)", f.read())
    return (float(m.group(1)), float(m.group(2)), float(m.group(3)), int(m.group(4))) if m else (float("nan"),) * 3 + (0,)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--comparator-repeat", type=int, default=5)
    ap.add_argument("--sizes", default="2048,4096,8192")
    ap.add_argument("--pairs", default="1,16,256,1024")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "descriptor_match.md"))
    args = ap.parse_args()
    import torch
    from xrsfm_amd import capi
    from tests import match_host_driver as H
    from tests import match_yardstick as Y
    if capi.device_count() < 1:
        raise SystemExit("no HIP device visible")
    torch.backends.cuda.matmul.allow_tf32 = False
    repeat = max(args.repeat, 20)
    sizes, counts = [int(x) for x in args.sizes.split(",")], [int(x) for x in args.pairs.split(",")]
    opt = capi.match_options()
    tab = torch.from_numpy(capi.debug_match_table()).cuda()
    props = torch.cuda.get_device_properties(0)
    cus, ghz = props.multi_processor_count, 2.4
    rows, ratios = [], {}
    n_frames = 33
    for n in sizes:
        frames = make_frames(Y, n_frames, n, seed=n)
        desc = np.ascontiguousarray(np.concatenate(frames))
        ptr = (n * np.arange(n_frames + 1)).astype(np.int64)
        host_ms = None
        if n == min(sizes):
            exe = H.build(tempfile.mkdtemp(prefix="match_host_"), flags=["-O2"])
            p = subprocess.run([exe, "time"], input=H.pair_input(frames[0], frames[1], Y.options()) + "\n", capture_output=True, text=True, check=True)
            host_ms = float(re.search(r"ms ([\d.]+)", p.stderr).group(1))
        for npair in counts:
            pa, pb = make_pairs(n_frames, npair)
            call = lambda: capi.match_descriptors(ptr, desc, pa, pb, opt)
            lib_ms, r = timed(call, args.warmup, repeat)
            prep, dots, select, launches = kernel_times(call)
            mfma_ms = 1e3 * npair * 2 * (n / 16) ** 2 * 16 / (4 * cus * ghz * 1e9)
            cmp_ms = None
            if npair == 1 or (npair <= 256 and n <= 4096):
                cmp_fn = lambda: (comparator(torch, desc, n, pa, pb, tab, opt), torch.cuda.synchronize())[0]
                cmp_ms, got = timed(cmp_fn, 1, repeat if npair < 256 else max(args.comparator_repeat, 1))
                mp = r["match_ptr"]
                for q in range(npair):
                    assert np.array_equal(got[q], r["matches"][mp[q]:mp[q + 1]]), ("comparator and library differ", n, npair, q)
                ratios[(n, npair)] = cmp_ms / lib_ms
            rows.append((n, npair, lib_ms, cmp_ms, prep, dots, select, launches, mfma_ms, int(r["match_ptr"][-1]), host_ms if npair == 1 else None))
            print(rows[-1], flush=True)
    f = lambda x, p="%.3f": "-" if x is None else p % x
    lines = ["# Descriptor matching: wall time per call", "",
             "Written by tools/descriptor_match_timing.py on %s (%d CUs).  Library and comparator: median wall time of a call in ms" % (props.name, cus),
             "(library: %d calls; comparator: %d calls, %d from 256 pairs on).  Kernel times: events on the library's stream, one call." % (
                 repeat, repeat, max(args.comparator_repeat, 1)),
             "MFMA: the time the int8 matrix instructions alone would take at 16 cycles each, 4 SIMDs per CU, %.1f GHz.  Host: the" % ghz,
             "sequential build of ba_match_rule.h (g++ -O2, one core), one pair.", "",
             "| size | pairs | library ms | comparator ms | comparator / library | k_match_prep ms | k_match_dots ms | k_match_select ms | launches | MFMA ms | matches | host ms |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for n, npair, lib_ms, cmp_ms, prep, dots, select, launches, mfma_ms, nm, host_ms in rows:
        lines.append("| %d x %d | %d | %s | %s | %s | %s | %s | %s | %d | %s | %d | %s |" % (
            n, n, npair, f(lib_ms), f(cmp_ms), f(None if cmp_ms is None else cmp_ms / lib_ms, "%.2f"), f(prep, "%.4f"), f(dots, "%.4f"), f(select, "%.4f"),
            launches, f(mfma_ms, "%.4f"), nm, f(host_ms, "%.1f")))
    lines.append("")
    for n in (2048, 4096):
        if (n, 256) in ratios:
            ok = ratios[(n, 256)] >= 1.0
            lines.append("Condition at 256 pairs of %d x %d: comparator / library = %.2f: %s." % (
                n, n, ratios[(n, 256)], "the library call is not slower than the comparator" if ok else "FAILS, the library call is slower than the comparator"))
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
