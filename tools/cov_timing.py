"""Time of one xrsfm_ba_covariance call on bench config L's problem (1000 cameras / 500 000 points / 2M observations) for 1, 10,
100 and all 1000 cameras, next to the time of one LM iteration of the same context; one table.  Then the same for
xrsfm_ba_point_covariance: 1, 21, 210 and 2100 points (1, 1, 10 and 100 chunks of 21) spread over the ring, the 21-point fallback,
and the ratio of every point row to the camera row with the same number of chunks (1, 10, 100, 1000 cameras are 1, 1, 10, 100
chunks of 10).  Then xrsfm_ba_joint_covariance: 2 cameras; 10 cameras + 21 points; 64 cameras + 85 points (spread over the ring),
the fallback at the smallest size, each next to the sum of the two marginal calls on the same selections.  --joint-only times
nothing but the joint rows (--joint-size picks one) and prints the number of joint calls made on the kernel path: under
`rocprofv3 --kernel-trace --stats` that gives the device time of k_cov_joint_gram per call, and --gram-us (one value per joint
size) puts it into the table as a share of the call.  Host clock around blocking calls (every call ends in a device synchronise); the first call of each size is a
warm-up and is not counted.  --map prints the whole-map table of xrsfm_ba_map_covariance instead: config L, config R and the
20 000-camera sequential shape on packed tiles; selected inversion, point pass (the library's own phase clocks, XRSFM_BA_COV_TIMING),
the whole call, and the bytes of the second tile storage.

    python tools/cov_timing.py [--config L] [--repeat 5] [--fallback-cams 10] [--fallback-points 21]
    python tools/cov_timing.py --joint-only [--joint-size 0|1|2] [--gram-us A,B,C]
    python tools/cov_timing.py --map [--repeat 3]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch  # noqa: F401  (first, so that both share one HIP runtime)

from xrsfm_amd import capi, synth


def _stderr_of(f):
    """Run f() and return what the process wrote to file descriptor 2 meanwhile (the library prints from C)."""
    import tempfile
    sys.stderr.flush()
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        saved = os.dup(2)
        os.dup2(tmp.fileno(), 2)
        try:
            f()
        finally:
            os.dup2(saved, 2); os.close(saved)
        tmp.seek(0)
        return tmp.read().decode(errors="replace")


def map_table(repeat):
    """One row per shape: the phases of xrsfm_ba_map_covariance as the library clocks them, median of `repeat` calls after a warm-up."""
    import re
    shapes = [("config L", lambda: synth.make_problem(**synth.CONFIGS["L"]), None),
              ("config R", lambda: synth.make_problem(**synth.CONFIGS["R"]), None),
              ("20 000 cameras, sequential", lambda: synth.make_problem(20000, 400000, 4, seed=13), 2000)]
    print("| shape | tile columns / levels / packed | selected inversion ms | point pass ms | whole call ms | second tile storage bytes |")
    print("|---|---|---|---|---|---|")
    for name, make, const_every in shapes:
        d = make()
        arr = {k: np.array(d[k], copy=True) for k in capi.ProblemArrays.FIELDS}
        cc = arr["cam_const"].copy(); cc[0] |= 3; cc[1] |= 2
        if const_every:
            cc[::const_every] |= 3          # (a loop this long with two constant frames is not positive definite in float64)
        arr["cam_const"] = cc
        plan = capi.debug_chol_plan(capi.ProblemArrays(**arr))
        ctx = capi.Context(capi.ProblemArrays(**arr))
        os.environ["XRSFM_BA_COV_TIMING"] = "1"
        try:
            ctx.map_covariance()
            vals = []
            for _ in range(repeat):
                t0 = time.perf_counter()
                err = _stderr_of(ctx.map_covariance)
                dt = 1e3 * (time.perf_counter() - t0)
                m = re.search(r"selected_inversion_ms ([0-9.]+) point_pass_ms ([0-9.]+) total_ms ([0-9.]+) z_bytes (\d+)", err)
                vals.append((float(m.group(1)), float(m.group(2)), dt, int(m.group(4))))
        finally:
            del os.environ["XRSFM_BA_COV_TIMING"]
            ctx.close()
        med = np.median(np.array([v[:3] for v in vals]), axis=0)
        print(f"| {name} | {plan['tiles']} / {plan['levels']} / {int(plan['facts']['packed'])} | {med[0]:.3f} | {med[1]:.3f} | {med[2]:.3f} | {vals[0][3]} |", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--map", action="store_true", help="the whole-map table of xrsfm_ba_map_covariance (configs L, R, 20 000 cameras) and nothing else")
    ap.add_argument("--config", default="L")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--fallback-cams", type=int, default=10, help="also time the fallback path for this many cameras (0: skip)")
    ap.add_argument("--fallback-points", type=int, default=21, help="also time the point fallback for this many points (0: skip)")
    ap.add_argument("--joint-only", action="store_true", help="time the joint rows only")
    ap.add_argument("--joint-size", type=int, default=-1, help="with --joint-only: only this one of the three joint sizes (and no fallback)")
    ap.add_argument("--gram-us", default="", help="device time of k_cov_joint_gram per call (us, from rocprofv3), one per joint size, comma separated")
    args = ap.parse_args()
    if capi.device_count() < 1:
        raise SystemExit("cov_timing: no HIP device")
    if args.map:
        map_table(max(1, min(args.repeat, 3)))
        return
    d = synth.make_problem(**synth.CONFIGS[args.config])
    arr = {k: np.array(d[k], copy=True) for k in capi.ProblemArrays.FIELDS}
    cc = arr["cam_const"].copy(); cc[0] |= 3; cc[1] |= 2; arr["cam_const"] = cc      # the gauge of the reference's GBA
    n = arr["cam_q"].shape[0]
    plan = capi.debug_chol_plan(capi.ProblemArrays(**arr))
    ctx = capi.Context(capi.ProblemArrays(**arr))
    opt = capi.default_options(linear_solver=capi.SOLVER_CHOLESKY)
    ctx.run(opt)                                   # warm-up (set-up of the factorisation, code objects)
    lm = []
    for _ in range(args.repeat):
        ctx.reset()
        t0 = time.perf_counter(); s = ctx.run(opt); dt = time.perf_counter() - t0
        lm.append(dt / max(1, s.n_successful + s.n_unsuccessful))
    ctx.reset()                                    # the covariance is timed at the uploaded state
    rng = np.random.default_rng(0)
    rows = []
    for m in (() if args.joint_only else (1, 10, 100, n)):
        sel = np.sort(rng.choice(n, m, replace=False)) if m < n else np.arange(n)
        ctx.covariance(sel)
        ts = []
        for _ in range(args.repeat):
            t0 = time.perf_counter(); ctx.covariance(sel); ts.append(time.perf_counter() - t0)
        rows.append((f"{m} cameras", min(ts), float(np.median(ts))))
    if args.fallback_cams > 0 and not args.joint_only:
        sel = np.sort(rng.choice(n, args.fallback_cams, replace=False))
        os.environ["XRSFM_BA_COV_FALLBACK"] = "1"
        try:
            ctx.covariance(sel)
            ts = []
            for _ in range(max(1, args.repeat // 2)):
                t0 = time.perf_counter(); ctx.covariance(sel); ts.append(time.perf_counter() - t0)
        finally:
            del os.environ["XRSFM_BA_COV_FALLBACK"]
        rows.append((f"{args.fallback_cams} cameras, fallback", min(ts), float(np.median(ts))))
    # points: observed points ordered by their first observing camera, taken evenly over that order (spread over the ring)
    n_pts = arr["points"].shape[0]
    first = np.full(n_pts, n, np.int64)
    np.minimum.at(first, arr["obs_pt"], arr["obs_cam"])
    by_cam = np.argsort(first, kind="stable")
    by_cam = by_cam[first[by_cam] < n]

    def spread(m):
        return by_cam[np.linspace(0, by_cam.shape[0] - 1, m).astype(int)].astype(np.int32)

    prow = []
    for m in (() if args.joint_only else (1, 21, 210, 2100)):
        sel = spread(m)
        ctx.point_covariance(sel)
        ts = []
        for _ in range(args.repeat):
            t0 = time.perf_counter(); ctx.point_covariance(sel); ts.append(time.perf_counter() - t0)
        prow.append((f"{m} points", min(ts), float(np.median(ts)), -(-m // 21)))
    if args.fallback_points > 0 and not args.joint_only:
        sel = spread(args.fallback_points)
        os.environ["XRSFM_BA_COV_FALLBACK"] = "1"
        try:
            ctx.point_covariance(sel)
            ts = []
            for _ in range(max(1, args.repeat // 2)):
                t0 = time.perf_counter(); ctx.point_covariance(sel); ts.append(time.perf_counter() - t0)
        finally:
            del os.environ["XRSFM_BA_COV_FALLBACK"]
        prow.append((f"{args.fallback_points} points, fallback", min(ts), float(np.median(ts)), None))
    # joint call: cameras spread over the ring past the two frames of the gauge, points spread as above
    def timed(f):
        f()
        ts = []
        for _ in range(args.repeat):
            t0 = time.perf_counter(); f(); ts.append(time.perf_counter() - t0)
        return min(ts), float(np.median(ts))

    sizes = [(2, 0), (10, 21), (64, 85)]
    gram_us = [float(v) for v in args.gram_us.split(",")] if args.gram_us else []
    jrow, n_joint_calls = [], 0
    for i, (mc, mp) in enumerate(sizes):
        if args.joint_only and args.joint_size >= 0 and i != args.joint_size:
            continue
        cs, ps = np.linspace(2, n - 1, mc).astype(np.int32), spread(mp) if mp else np.zeros(0, np.int32)
        tj = timed(lambda: ctx.joint_covariance(cs, ps))
        n_joint_calls += args.repeat + 1
        tm = timed(lambda: (ctx.covariance(cs), ctx.point_covariance(ps)))
        jrow.append((f"{mc} cameras + {mp} points (N = {6 * mc + 3 * mp})", tj, tm, gram_us[i] if i < len(gram_us) else None))
        if i == 0 and args.joint_size < 0:
            os.environ["XRSFM_BA_COV_FALLBACK"] = "1"
            try:
                tf = timed(lambda: ctx.joint_covariance(cs, ps))
            finally:
                del os.environ["XRSFM_BA_COV_FALLBACK"]
            jrow.append((f"{mc} cameras + {mp} points, fallback", tf, None, None))
    ctx.close()
    print(f"config {args.config}: {n} cameras, {arr['points'].shape[0]} points, {arr['obs_cam'].shape[0]} observations; "
          f"{plan['tiles']} tile columns on {plan['levels']} levels, schedule {plan['facts']['schedule']}, packed {plan['facts']['packed']}")
    print(f"| call | min ms | median ms | x one LM iteration |")
    print(f"|---|---|---|---|")
    lm_ms = 1e3 * float(np.median(lm))
    print(f"| one LM iteration (whole run / iterations) | {1e3 * min(lm):.3f} | {lm_ms:.3f} | 1.0 |")
    for name, tmin, tmed in rows:
        print(f"| covariance, {name} | {1e3 * tmin:.3f} | {1e3 * tmed:.3f} | {1e3 * tmed / lm_ms:.1f} |")
    cam_by_chunks = {-(-m // 10): tmed for (name, _, tmed), m in zip(rows, (1, 10, 100, n))}      # (1 camera and 10 cameras: one chunk; the later row stays)
    print()
    print(f"| call | min ms | median ms | x one LM iteration | x camera call with as many chunks |")
    print(f"|---|---|---|---|---|")
    for name, tmin, tmed, chunks in prow:
        ratio = f"{tmed / cam_by_chunks[chunks]:.2f} ({chunks} chunk{'s' if chunks > 1 else ''})" if chunks in cam_by_chunks else "-"
        print(f"| point covariance, {name} | {1e3 * tmin:.3f} | {1e3 * tmed:.3f} | {1e3 * tmed / lm_ms:.1f} | {ratio} |")
    print()
    if args.joint_only:
        print(f"joint calls on the kernel path: {n_joint_calls}")
    print(f"| call | min ms | median ms | x one LM iteration | covariance + point_covariance, same selections: median ms | k_cov_joint_gram per call: us (share) |")
    print(f"|---|---|---|---|---|---|")
    for name, (tmin, tmed), tm, g in jrow:
        both = f"{1e3 * tm[1]:.3f}" if tm else "-"
        share = f"{g:.1f} ({100.0 * g * 1e-6 / tmed:.1f} %)" if g is not None else "-"
        print(f"| joint covariance, {name} | {1e3 * tmin:.3f} | {1e3 * tmed:.3f} | {1e3 * tmed / lm_ms:.1f} | {both} | {share} |")


if __name__ == "__main__":
    main()
