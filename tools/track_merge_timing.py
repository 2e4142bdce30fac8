"""Time track completion and merging (xrsfm_ba_merge_tracks) and write profiles/track_merge.md.

Input: a synthetic ring of n pinhole cameras on a circle, looking outward.  Points outside the circle are seen by runs of 6 consecutive
frames, about `keys` of them per frame, projected with 0.5 px of noise; every frame is paired with its next two neighbours and matched
on the points both see (capi.correspondence_graph), and one match in a hundred is made wrong.  Tracks have the triangulation's shape:
of the six views of a point the first two carry one track and the fourth and fifth another, both near the point; the third and the
sixth are free.  So every point offers two continues and one merge, and the wrong matches offer merges that fail.

Per size, median (min .. max) of --repeat calls after --warmup, ms:
  map mode 3    host clock around capi.merge_tracks (ContinueTrack then MergeTrack over every track), XRSFM_BA_MERGE_TIMING unset
  phases        one line per call with XRSFM_BA_MERGE_TIMING set: host clocks of the checks and components, the upload, k_merge_components,
                k_merge_counts and the read-back.  The stream is drained at the phase boundaries in this mode.
  frame mode    MergeTracks on the middle frame through capi.merge_closure: the closure (numpy) and the call on the sub-map
  host program  the stand-alone program of tests/merge_host_driver.py, built from ba_merge_rule.h at -O2, on the same input in map
                mode 3: its own clocks around the components and plan, and around the driver loops and counts (no parsing).
                Information only: nothing computed this before, so there is no ratio to hold.

    python tools/track_merge_timing.py [--repeat 5] [--warmup 1] [--sizes 64x2000,256x4000] [--out profiles/track_merge.md]
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
SPAN, STEPS = 6, 2
FX, CX, CY, R0 = 400.0, 640.0, 480.0, 10.0            # (the pinhole models double the focal length: 800 px)


def ring(n, keys, seed=1):
    from xrsfm_amd import capi
    rng = np.random.default_rng(seed)
    pts = n * keys // SPAN
    start = rng.integers(0, n, pts)
    mid = 2 * np.pi * (start + 2.5 + rng.uniform(-0.5, 0.5, pts)) / n
    rad = R0 + rng.uniform(4.0, 9.0, pts)
    P = np.stack([rad * np.sin(mid), rng.uniform(-1.5, 1.5, pts), rad * np.cos(mid)], 1)
    a = 2 * np.pi * np.arange(n) / n
    cam_q = np.stack([np.zeros(n), np.sin(-a / 2), np.zeros(n), np.cos(-a / 2)], 1)
    rows = lambda f: np.array([[np.cos(a[f]), 0, -np.sin(a[f])], [0, 1, 0], [np.sin(a[f]), 0, np.cos(a[f])]])
    cam_t = np.stack([-rows(f) @ (R0 * np.array([np.sin(a[f]), 0, np.cos(a[f])])) for f in range(n)])
    seen = [np.flatnonzero(((f - start) % n) < SPAN) for f in range(n)]          # ascending point ids: the key points of frame f
    key_ptr = np.concatenate([[0], np.cumsum([len(s) for s in seen])]).astype(np.int64)
    xy = []
    for f in range(n):
        pc = P[seen[f]] @ rows(f).T + cam_t[f]
        xy.append(np.stack([2 * FX * pc[:, 0] / pc[:, 2] + CX, 2 * FX * pc[:, 1] / pc[:, 2] + CY], 1) + rng.normal(0, 0.5, (len(pc), 2)))
    pa, pb, ms = [], [], []
    for f in range(n):
        for d in range(1, STEPS + 1):
            g = (f + d) % n
            both = np.intersect1d(seen[f], seen[g])
            m = np.stack([np.searchsorted(seen[f], both), np.searchsorted(seen[g], both)], 1)
            wrong = rng.random(len(m)) < 0.01
            m[wrong, 1] = rng.integers(0, len(seen[g]), int(wrong.sum()))
            pa.append(f); pb.append(g); ms.append(m)
    match_ptr = np.concatenate([[0], np.cumsum([len(m) for m in ms])]).astype(np.int64)
    corr_ptr, corr_key = capi.correspondence_graph(key_ptr, pa, pb, match_ptr, np.concatenate(ms))
    tok = np.full(int(key_ptr[-1]), -1, np.int32)
    for f in range(n):                                  # view 0, 1 of a point: track 2 p; view 3, 4: track 2 p + 1
        view = (f - start[seen[f]]) % n
        k = key_ptr[f] + np.arange(len(seen[f]))
        tok[k[view < 2]] = 2 * seen[f][view < 2]
        tok[k[(view == 3) | (view == 4)]] = 2 * seen[f][(view == 3) | (view == 4)] + 1
    points = np.repeat(P, 2, axis=0) + rng.normal(0, 0.01, (2 * pts, 3))
    return dict(key_ptr=key_ptr, key_xy=np.concatenate(xy), registered=np.ones(n, np.uint8), cam_q=cam_q, cam_t=cam_t, cam_intr=np.zeros(n, np.int32),
                intr_model=np.array([1], np.int32), intr_params=np.array([[FX, FX, CX, CY, 0, 0, 0, 0]], np.float64), corr_ptr=corr_ptr, corr_key=corr_key, points=points,
                track_outlier=np.zeros(2 * pts, np.uint8), track_of_key=tok, max_re=8.0, frame=n // 2)


ARGS = ("key_ptr", "key_xy", "registered", "cam_q", "cam_t", "cam_intr", "intr_model", "intr_params", "corr_ptr", "corr_key", "points", "track_outlier", "track_of_key")
PHASES = ("host", "upload", "components", "counts", "back")
LINE = re.compile(r"merge timing: host ([\d.]+) ms, upload ([\d.]+) ms, components ([\d.]+) ms, counts ([\d.]+) ms, back ([\d.]+) ms")


def stat(v):
    return "%.3f (%.3f .. %.3f)" % (float(np.median(v)), min(v), max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sizes", default="64x2000,256x4000")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_merge.md"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    import torch  # noqa: F401
    from tests import merge_host_driver as HD
    from xrsfm_amd import capi
    if capi.device_count() <= 0:
        raise SystemExit("no GPU: nothing here can be measured without one")
    call = lambda c, **kw: capi.merge_tracks(*[c[k] for k in ARGS], options=capi.merge_options(max_reproj_error=c["max_re"], **kw))
    if args.child:                                   # the calls with the phase clocks on: their lines go to stderr
        n, keys = (int(x) for x in args.child.split("x"))
        c = ring(n, keys)
        call(c)
        os.environ["XRSFM_BA_MERGE_TIMING"] = "1"
        for _ in range(args.warmup + args.repeat):
            call(c)
        return
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        exe = HD.build(tmp, flags=["-O2", "-ffp-contract=off"])
        for size in args.sizes.split(","):
            n, keys = (int(x) for x in size.split("x"))
            c = ring(n, keys)
            e2e, closure, framecall = [], [], []
            for k in range(args.warmup + args.repeat):
                t0 = time.perf_counter()
                r = call(c)
                if k >= args.warmup:
                    e2e.append(1e3 * (time.perf_counter() - t0))
            for k in range(args.warmup + args.repeat):
                t0 = time.perf_counter()
                s = capi.merge_closure(c["frame"], c["key_ptr"], c["corr_ptr"], c["corr_key"], c["track_of_key"])
                sub = dict(c, key_ptr=s["key_ptr"], key_xy=c["key_xy"][s["keys"]], corr_ptr=s["corr_ptr"], corr_key=s["corr_key"], points=c["points"][s["tracks"]],
                           track_outlier=c["track_outlier"][s["tracks"]], track_of_key=s["track_of_key"])
                t1 = time.perf_counter()
                rf = call(sub, mode=4, frame=c["frame"])
                if k >= args.warmup:
                    closure.append(1e3 * (t1 - t0)); framecall.append(1e3 * (time.perf_counter() - t1))
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", size, "--repeat", str(args.repeat), "--warmup", str(args.warmup)], capture_output=True,
                                 text=True, check=True)
            lines = [m.groups() for m in LINE.finditer(out.stderr)][args.warmup:]
            ph = {k: [float(g[i]) for g in lines] for i, k in enumerate(PHASES)}
            host = HD.run(exe, HD.case_input(c, 3, repeats=args.warmup + args.repeat))
            same = (host["track_of_key"] == r["track_of_key"].tolist() and host["track_outlier"] == r["track_outlier"].tolist() and host["track_status"] == r["track_status"].tolist()
                    and host["point_bits"] == r["points"].view(np.uint64).ravel().tolist() and host["stats"][:7] == list(r["stats"].values())
                    and host["corr_have_point3d"] == r["corr_have_point3d"].tolist() and host["visible"] == r["visible"].tolist())
            sizes = np.bincount(np.array(host["comp_of_key"]))
            hist = [(lo, int(((sizes >= lo) & (sizes < hi)).sum())) for lo, hi in ((1, 2), (2, 7), (7, 13), (13, 65), (65, 1025), (1025, 1 << 30))]
            rows.append(dict(size=size, N=int(c["key_ptr"][-1]), E=len(c["corr_key"]), T=len(c["points"]), comps=len(sizes), hist=hist, stats=r["stats"], fstats=rf["stats"],
                             sub=len(s["keys"]), e2e=e2e, closure=closure, framecall=framecall, ph=ph, host_plan=host["ms_plan"][args.warmup:], host_run=host["ms_run"][args.warmup:],
                             same=same))
            print({k: v for k, v in rows[-1].items() if k != "ph"}, flush=True)
    with open(args.out, "w") as f:
        f.write("# Track completion and merging: measured times\n\n")
        f.write("Written by `tools/track_merge_timing.py` (what every row is: its docstring).  A synthetic ring of frames, 8 px, one MI355X; median (min .. max) of %d\n"
                "calls after %d, ms.  The first measurement of this step: no figure existed for the reference or for this library, and no speed-up is claimed.\n\n"
                % (args.repeat, args.warmup))
        f.write("| frames x keys | key points | list entries | tracks | components | of 1 key | 2-6 | 7-12 | 13-64 | 65-1024 | above the limits |\n|---|---|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            f.write("| %s | %d | %d | %d | %d | %s |\n" % (r["size"], r["N"], r["E"], r["T"], r["comps"], " | ".join(str(k) for _, k in r["hist"])))
        f.write("\n| frames x keys | mode | components processed | skipped | largest | merged / connected tracks | continued / connected measurements | equal to the host program |\n"
                "|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            for mode, s, eq in (("map 3", r["stats"], "yes" if r["same"] else "NO"), ("frame, closure of %d keys" % r["sub"], r["fstats"], "-")):
                f.write("| %s | %s | %d | %d | %d | %d / %d | %d / %d | %s |\n" % (r["size"], mode, s["components"], s["skipped"], s["largest"], s["merged"], s["connected_tracks"],
                                                                              s["continued"], s["connected_measurements"], eq))
        f.write("\n| frames x keys | map mode 3, end to end | frame mode: closure (numpy) | frame mode: call | host program: components and plan | host program: loops and counts |\n"
                "|---|---|---|---|---|---|\n")
        for r in rows:
            f.write("| %s | %s | %s | %s | %s | %s |\n" % (r["size"], stat(r["e2e"]), stat(r["closure"]), stat(r["framecall"]), stat(r["host_plan"]), stat(r["host_run"])))
        f.write("\nPhases of a map-mode call with `XRSFM_BA_MERGE_TIMING` (host clocks; the stream is drained between them):\n\n"
                "| frames x keys | host checks + components | upload | k_merge_components | k_merge_counts | back |\n|---|---|---|---|---|---|\n")
        for r in rows:
            f.write("| %s | %s |\n" % (r["size"], " | ".join(stat(r["ph"][k]) for k in PHASES)))
        f.write("\nMeasured: the above.  Not measured: real matches (the ring's components are the six views of a point, chained only by its wrong matches), components\n"
                "above the limits (the ring has none), and the reference's own program.  The host program's times are information, not a bar.\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
