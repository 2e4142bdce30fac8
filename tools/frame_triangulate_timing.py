"""Time frame triangulation (xrsfm_ba_triangulate_frames) and write profiles/frame_triangulate.md.

Input: the synthetic ring of tools/track_merge_timing.py (points seen by runs of 6 consecutive frames, matches to the next two frames,
one in a hundred wrong), its pixels turned into normalised coordinates.  Of the six views of a point two pairs carry a track; here
every third point loses its tracks (its key points go through the create branch), and in frame mode the middle frame carries no track.

Per size, median (min .. max) of --repeat calls after --warmup, ms:
  frame mode    the middle frame alone: host clock around capi.triangulate_frames, XRSFM_BA_TRIF_TIMING unset
  map mode      every frame ascending, the same
  phases        one line per call with XRSFM_BA_TRIF_TIMING set: host clocks of the checks and the plan, the upload, each kernel class
                summed over the steps, and the read-back.  The stream is drained after every launch in this mode, so a class's time
                holds one launch latency per step.
  create_events the same mode's HIP events around every k_tri_tracks launch of the call, summed over the steps: the kernel's own time
  tri_tracks    xrsfm_ba_triangulate_tracks (unchanged by this step) on the lists of the key points that went through the create branch,
                in one call: its kernel's time by HIP events (XRSFM_BA_TRI_TIMING), the same clock as create_events.  The call runs the
                same kernel on the same lists, one launch per step, each launch with as many waves as the step has slots.  The two
                "match" when their (min .. max) ranges over the repeats overlap: the run-to-run spread this tool records.

    python tools/frame_triangulate_timing.py [--repeat 5] [--warmup 1] [--sizes 32x1000,64x2000] [--out profiles/frame_triangulate.md]
"""
import argparse
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
PHASES = ("host", "upload", "held", "classify", "select", "create", "resolve", "counts", "back")
LINE = re.compile(r"trif timing: " + ", ".join(k + r" ([\d.]+) ms" for k in PHASES))
EVENTS = re.compile(r"create_events ([\d.]+) ms")
TRI = re.compile(r"triangulate: kernel_ms ([\d.]+)")


def scene(n, keys, mode):
    import track_merge_timing as TM
    c = TM.ring(n, keys)
    xyn = (c["key_xy"] - np.array([TM.CX, TM.CY])) / (2 * TM.FX)
    tok = c["track_of_key"].copy()
    tok[(tok >= 0) & ((tok // 2) % 3 == 0)] = -1
    frames = list(range(n))
    if mode == "frame":
        frames = [n // 2]
        tok[c["key_ptr"][n // 2]:c["key_ptr"][n // 2 + 1]] = -1
    return dict(c, key_xyn=xyn, track_of_key=tok), frames


def call(c, frames):
    from xrsfm_amd import capi
    return capi.triangulate_frames(c["key_ptr"], c["key_xyn"], c["registered"], c["cam_q"], c["cam_t"], c["corr_ptr"], c["corr_key"], frames, c["points"], c["track_outlier"],
                                   c["track_of_key"])


def create_lists(c, r):
    """trk_ptr, obs_cam, obs_xy of the key points that went through the create branch (status 1 or 4), in key order"""
    fok = np.repeat(np.arange(len(c["key_ptr"]) - 1), np.diff(c["key_ptr"]))
    ptr, cam, key = [0], [], []
    for p in np.flatnonzero((r["key_status"] == 1) | (r["key_status"] == 4)):
        l = [int(b) for b in c["corr_key"][c["corr_ptr"][p]:c["corr_ptr"][p + 1]] if c["registered"][fok[b]]] + [int(p)]
        key += l; cam += fok[l].tolist(); ptr.append(len(key))
    return np.array(ptr, np.int32), np.array(cam, np.int32), c["key_xyn"][key]


def stat(v):
    return "%.3f (%.3f .. %.3f)" % (float(np.median(v)), min(v), max(v)) if len(v) else "-"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sizes", default="32x1000,64x2000")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frame_triangulate.md"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    import torch  # noqa: F401
    from xrsfm_amd import capi
    if capi.device_count() <= 0:
        raise SystemExit("no GPU: nothing here can be measured without one")
    if args.child:                                   # the calls with the phase clocks on: their lines go to stderr
        size, mode = args.child.split(":")
        c, frames = scene(*(int(x) for x in size.split("x")), mode)
        r = call(c, frames)
        ptr, cam, xy = create_lists(c, r)
        capi.triangulate_tracks(c["cam_q"], c["cam_t"], ptr, cam, xy)
        os.environ["XRSFM_BA_TRIF_TIMING"] = "1"
        for _ in range(args.warmup + args.repeat):
            call(c, frames)
        del os.environ["XRSFM_BA_TRIF_TIMING"]
        os.environ["XRSFM_BA_TRI_TIMING"] = "1"
        for _ in range(args.warmup + args.repeat):
            capi.triangulate_tracks(c["cam_q"], c["cam_t"], ptr, cam, xy)
        return
    rows = []
    for size in args.sizes.split(","):
        for mode in ("frame", "map"):
            c, frames = scene(*(int(x) for x in size.split("x")), mode)
            e2e = []
            for k in range(args.warmup + args.repeat):
                t0 = time.perf_counter()
                r = call(c, frames)
                if k >= args.warmup:
                    e2e.append(1e3 * (time.perf_counter() - t0))
            ptr, cam, xy = create_lists(c, r)
            t = capi.triangulate_tracks(c["cam_q"], c["cam_t"], ptr, cam, xy)
            created = np.flatnonzero(t["status"] == 1)
            same = r["points"][len(c["points"]):].tobytes() == t["points"][created].tobytes() and len(created) == r["stats"]["created"]
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", size + ":" + mode, "--repeat", str(args.repeat), "--warmup", str(args.warmup)],
                                 capture_output=True, text=True, check=True)
            lines = [m.groups() for m in LINE.finditer(out.stderr)][args.warmup:]
            ph = {k: [float(g[i]) for g in lines] for i, k in enumerate(PHASES)}
            tri = [float(m.group(1)) for m in TRI.finditer(out.stderr)][args.warmup:]
            ev = [float(m.group(1)) for m in EVENTS.finditer(out.stderr)][args.warmup:]
            rows.append(dict(size=size, mode=mode, N=int(c["key_ptr"][-1]), E=len(c["corr_key"]), T=len(c["points"]), lists=len(ptr) - 1, obs=int(ptr[-1]), stats=r["stats"], e2e=e2e,
                             ph=ph, tri=tri, ev=ev, same=same))
            print({k: v for k, v in rows[-1].items() if k != "ph"}, flush=True)
    with open(args.out, "w") as f:
        f.write("# Frame triangulation: measured times\n\n")
        f.write("Written by `tools/frame_triangulate_timing.py` (what every row is: its docstring).  A synthetic ring of frames, one MI355X; median (min .. max) of %d\n"
                "calls after %d, ms.  The first measurement of this step: no figure existed for the reference or for this library, and no speed-up is claimed.\n\n"
                % (args.repeat, args.warmup))
        f.write("| frames x keys | mode | key points | list entries | tracks before | steps | split frames | created / create branch | extended / one track / several | most claim rounds |"
                " created points equal xrsfm_ba_triangulate_tracks |\n|---|---|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            s = r["stats"]
            f.write("| %s | %s | %d | %d | %d | %d | %d | %d / %d | %d / %d / %d | %d | %s |\n" % (r["size"], r["mode"], r["N"], r["E"], r["T"], s["steps"], s["split_frames"], s["created"],
                    s["zero_track"], s["extended"], s["one_track"], s["multi_track"], s["claim_rounds"], "yes" if r["same"] else "NO"))
        f.write("\n| frames x keys | mode | end to end | " + " | ".join(PHASES) + " |\n|---|---|---|" + "---|" * len(PHASES) + "\n")
        for r in rows:
            f.write("| %s | %s | %s | %s |\n" % (r["size"], r["mode"], stat(r["e2e"]), " | ".join(stat(r["ph"][k]) for k in PHASES)))
        f.write("\nThe create kernel inside the call against `xrsfm_ba_triangulate_tracks` on the same lists (one call), both by HIP events around `k_tri_tracks`:\n\n"
                "| frames x keys | mode | lists | observations | launches | inside the call, summed (HIP events) | k_tri_tracks alone (HIP events) | ratio of medians | ranges overlap |"
                " create class by the host clock |\n|---|---|---|---|---|---|---|---|---|---|\n")
        verdict = []
        for r in rows:
            ok = len(r["ev"]) > 0 and len(r["tri"]) > 0 and min(r["ev"]) <= max(r["tri"]) and min(r["tri"]) <= max(r["ev"])
            verdict.append(ok)
            f.write("| %s | %s | %d | %d | %d | %s | %s | %.2f | %s | %s |\n" % (r["size"], r["mode"], r["lists"], r["obs"], r["stats"]["steps"], stat(r["ev"]), stat(r["tri"]),
                    float(np.median(r["ev"]) / np.median(r["tri"])) if ok or (len(r["ev"]) and len(r["tri"])) else float("nan"), "yes" if ok else "NO", stat(r["ph"]["create"])))
        f.write("\nThe two event columns are the same kernel on the same lists under the same clock.  They differ in the launches: the call starts the kernel once per step\n"
                "with one wave per slot of the step, of which only the create branch has a list (the other waves meet an empty list and leave); the other column is one\n"
                "launch with one wave per list.  Matching means that the (min .. max) ranges over the repeats overlap; it holds in %d of %d rows%s.\n"
                "Per launch the kernel inside the call lasts %s us (median of the summed events over the launches, row by row), against %s us for the one launch over all\n"
                "lists.  A reading of these figures, not measured per wave: a launch cannot end before its slowest list, so the create kernel's time in a call grows with\n"
                "the steps more than with the lists, and a map-mode call pays that once per step.\n"
                "The host-clock column holds, besides the kernel, one launch and one drain of the stream per step.\n"
                "Not measured: real matches and the reference's own program.\n"
                % (sum(verdict), len(verdict), "" if all(verdict) else ": where it does not hold, the create kernel inside the call does NOT match the stand-alone call, by the ratio shown",
                   ", ".join("%.0f" % (1e3 * np.median(r["ev"]) / max(r["stats"]["steps"], 1)) for r in rows if len(r["ev"])),
                   ", ".join("%.0f" % (1e3 * np.median(r["tri"])) for r in rows if len(r["tri"]))))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
