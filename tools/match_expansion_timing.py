"""Time match expansion (xrsfm_ba_expand_candidates) and write profiles/match_expansion.md.

Input: a synthetic ring of n frames.  Points are seen by runs of 6 consecutive frames, about `keys` of them per frame; every frame is
paired with its next two neighbours and matched on the points both see; every frame ranks its 20 nearest; the default options.
Two sizes.

Per size, median (min .. max) of --repeat calls after --warmup:
  end to end   host clock around capi.expand_candidates, XRSFM_BA_EXPAND_TIMING unset
  phases       one line per call with XRSFM_BA_EXPAND_TIMING set: host clocks of the tracks (AddTrack on the host), of the uploads and of
               the rounds (their launches and the one word read back per round), of the final read-back, and HIP-event times of
               k_expand_patch, of the correspondence lists (count, scan, fill), of k_expand_covis and of k_expand_pairs.  The stream is
               drained at the phase boundaries in this mode, so the phases do not add up to the end-to-end time.
  host search  the same search by the stand-alone program of tests/expand_host_driver.py, built from ba_expand_rule.h at -O2: its own
               clock around the search (no parsing), and around make_tracks alone.  Information only: no implementation existed before
               this one, so there is no ratio to hold.

    python tools/match_expansion_timing.py [--repeat 5] [--warmup 1] [--sizes 64x2000,256x4000] [--out profiles/match_expansion.md]
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
SPAN, STEPS, RANKED = 6, 2, 20


def ring(n, keys, seed=1):
    rng = np.random.default_rng(seed)
    pts = n * keys // SPAN
    start = rng.integers(0, n, pts)
    xy0 = np.stack([rng.uniform(0, 1279, pts), rng.uniform(0, 959, pts)], 1)
    seen = [np.flatnonzero(((f - start) % n) < SPAN) for f in range(n)]          # ascending point ids: the key points of frame f
    key_ptr = np.concatenate([[0], np.cumsum([len(s) for s in seen])]).astype(np.int64)
    kx = np.concatenate([np.clip(xy0[s] + rng.normal(0, 4, (len(s), 2)), 0, [1279, 959]) for s in seen])
    keys4 = np.zeros((len(kx), 4), np.float32)
    keys4[:, :2] = kx
    pa, pb, ms = [], [], []
    for f in range(n):
        for d in range(1, STEPS + 1):
            g = (f + d) % n
            if n <= 2 * STEPS and g < f:
                continue
            both = np.intersect1d(seen[f], seen[g])
            pa.append(f); pb.append(g)
            ms.append(np.stack([np.searchsorted(seen[f], both), np.searchsorted(seen[g], both)], 1))
    mp = np.concatenate([[0], np.cumsum([len(m) for m in ms])]).astype(np.int64)
    near = [d for k in range(1, RANKED // 2 + 1) for d in (k, -k)]
    rank_ids = np.array([(f + d) % n for f in range(n) for d in near], np.int32)
    return dict(n=n, key_ptr=key_ptr, keys=keys4, sizes=np.array([(1280, 960)] * n, np.int32), pair_a=np.array(pa, np.int32), pair_b=np.array(pb, np.int32), match_ptr=mp,
                matches=np.ascontiguousarray(np.concatenate(ms), np.int32), rank_ptr=(np.arange(n + 1) * len(near)).astype(np.int64), rank_ids=rank_ids,
                tried=np.stack([pa, pb], 1).astype(np.int32), init=(0, 1), opt={})


PHASES = ("tracks", "uploads", "patch", "lists", "rounds", "covis", "pairs", "back")
LINE = re.compile(r"expand timing: tracks ([\d.]+) ms, uploads ([\d.]+) ms, patch ([\d.]+) ms, lists ([\d.]+) ms, rounds ([\d.]+) ms \((\d+)\), covis ([\d.]+) ms, "
                  r"pairs ([\d.]+) ms, back ([\d.]+) ms")


def stat(v):
    return "%.3f (%.3f .. %.3f)" % (float(np.median(v)), min(v), max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sizes", default="64x2000,256x4000")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "match_expansion.md"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    import torch  # noqa: F401
    from tests import expand_host_driver as HD
    from tests import expand_yardstick as Y
    from xrsfm_amd import capi
    if capi.device_count() <= 0:
        raise SystemExit("no GPU: nothing here can be measured without one")
    call = lambda c: capi.expand_candidates(c["key_ptr"], c["keys"], c["sizes"], c["pair_a"], c["pair_b"], c["match_ptr"], c["matches"], c["rank_ptr"], c["rank_ids"],
                                            c["init"][0], c["init"][1], c["tried"])
    if args.child:                                   # the calls with the phase clocks on: their lines go to stderr
        n, keys = (int(x) for x in args.child.split("x"))
        c = ring(n, keys)
        call(c)
        os.environ["XRSFM_BA_EXPAND_TIMING"] = "1"
        for _ in range(args.warmup + args.repeat):
            call(c)
        return
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        exe = HD.build(tmp, flags=["-O2"])
        for size in args.sizes.split(","):
            n, keys = (int(x) for x in size.split("x"))
            c = ring(n, keys)
            e2e = []
            for k in range(args.warmup + args.repeat):
                t0 = time.perf_counter()
                r = call(c)
                if k >= args.warmup:
                    e2e.append(1e3 * (time.perf_counter() - t0))
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", size, "--repeat", str(args.repeat), "--warmup", str(args.warmup)], capture_output=True,
                                 text=True, check=True)
            lines = [m.groups() for m in LINE.finditer(out.stderr)][args.warmup:]
            ph = {k: [float(g[i if i < 5 else i + 1]) for g in lines] for i, k in enumerate(PHASES)}
            host = HD.run(exe, HD.case_input(c, Y.DEFAULTS, repeats=args.warmup + args.repeat))
            same = (host["out_a"] == r["pair_a"].tolist() and host["out_b"] == r["pair_b"].tolist() and host["visible"] == r["visible"].tolist()
                    and host["cand"] == r["cand"].ravel().tolist())
            rows.append(dict(size=size, n=n, N=int(c["key_ptr"][-1]), M=len(c["matches"]), pairs=len(c["pair_a"]), stats=r["stats"], out=len(r["pair_a"]), cand=len(r["cand"]),
                             e2e=e2e, ph=ph, host_total=host["ms_total"][args.warmup:], host_tracks=host["ms_tracks"][args.warmup:], same=same))
            print({k: v for k, v in rows[-1].items() if k != "ph"}, flush=True)
    with open(args.out, "w") as f:
        f.write("# Match expansion: measured times\n\n")
        f.write("Written by `tools/match_expansion_timing.py` (what every row is: its docstring).  A synthetic ring of frames, default options, one MI355X;\n"
                "median (min .. max) of %d calls after %d, ms.\n\n" % (args.repeat, args.warmup))
        f.write("| frames x keys | key points | pairs | matches | tracks | rounds | items walked | codes kept | directed candidates | pairs out | equal to the host program |\n"
                "|---|---|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            s = r["stats"]
            f.write("| %s | %d | %d | %d | %d | %d | %d | %d | %d | %d | %s |\n" % (r["size"], r["N"], r["pairs"], r["M"], s["tracks"], s["rounds"], s["items_walked"], s["codes_kept"],
                                                                           r["cand"], r["out"], "yes" if r["same"] else "NO"))
        f.write("\n| frames x keys | end to end | host program, whole search | host program, make_tracks |\n|---|---|---|---|\n")
        for r in rows:
            f.write("| %s | %s | %s | %s |\n" % (r["size"], stat(r["e2e"]), stat(r["host_total"]), stat(r["host_tracks"])))
        f.write("\nPhases of a call with `XRSFM_BA_EXPAND_TIMING` (host clocks: tracks, uploads, rounds, back; HIP events: patch, lists, covis, pairs):\n\n"
                "| frames x keys | " + " | ".join(PHASES) + " |\n|---" * 1 + "|---" * len(PHASES) + "|\n")
        for r in rows:
            f.write("| %s | %s |\n" % (r["size"], " | ".join(stat(r["ph"][k]) for k in PHASES)))
        f.write("\nMeasured: the above.  Not measured: real retrieval lists and real matches (every match of the ring is right; its tracks merge only where the\n"
                "ring closes), sets of more frames than one pass of k_expand_covis holds, and the reference's own program.  The host figures are information only.\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
