"""The yardstick of frame triangulation: Point3dProcessor::TriangulateFramePoint for a list of frames, twice.

(A) run_literal: the reference's program on dicts.  A track is a dict with its point and its observations {frame: key point}; it joins
    the map the moment it is created, and the key points of a whole frame are walked in order.  The angle is acos of the dot product, in
    float64 or np.longdouble, compared as the reference compares it (strictly smaller is better, below the threshold is accepted).
(B) run_flat: the library's program on the flat arrays, in float64: the slots and their lists built once, a frame cut into runs
    without a coupled pair, per step the branch of every slot, the creates with ids in key order, and the claims in rounds of bids;
    candidates ordered by the dot product and accepted by dot_bound(), no acos in a decision.

The create arithmetic is a callback: create(lists) -> one dict(status, point, mask, num_inliers, num_trials, best_trial) per list,
a list being (frames [n], xy [n, 2]).  cpu_create runs tests/tri_yardstick.py; the GPU tests hand in capi.triangulate_tracks.

(A) records every decision's margin as (kind, relative margin, exact): "order" the best against the second-best angle, "threshold"
the best angle against extend_angle_rad, "one" every candidate's dot product against 1; exact marks a constructed equality."""
import math

import numpy as np

from tests import tri_yardstick as TY

EXT = np.longdouble
MAX_OBS = 128
NO_BID = 0x7F7F7F7F
EXTEND_ANGLE = 8.0 * 0.0174532925199432954743716805978692718781530857086181640625
STATUS = ("not_visited", "created", "few_observations", "too_many", "no_model", "extended", "none_accepted")
STATS = ("created", "zero_track", "extended", "one_track", "multi_track", "steps", "split_frames", "claim_rounds")
INTEGERS = ("track_of_key", "key_status", "n_tracks", "num_inliers", "num_trials", "best_trial", "corr_have_point3d", "visible", "measured", "track_outlier")


# ---------------------------------------------------------------------------------------------------- the rule
def ray_dot(q, t, X, xy, dt=float):
    """the dot product of GetMaxAngle's rays, operation for operation as csrc/ba_trif_rule.h"""
    x, y, z, w = (dt(v) for v in q)
    P0, P1, P2 = (dt(v) for v in X)
    t0, t1, t2 = (dt(v) for v in t)
    xn, yn = dt(xy[0]), dt(xy[1])
    one, two = dt(1.0), dt(2.0)
    M0, M1, M2 = one - two * (y * y + z * z), two * (x * y - w * z), two * (x * z + w * y)
    M3, M4, M5 = two * (x * y + w * z), one - two * (x * x + z * z), two * (y * z - w * x)
    M6, M7, M8 = two * (x * z - w * y), two * (y * z + w * x), one - two * (x * x + y * y)
    a0 = M0 * P0 + M1 * P1 + M2 * P2 + t0
    a1 = M3 * P0 + M4 * P1 + M5 * P2 + t1
    a2 = M6 * P0 + M7 * P1 + M8 * P2 + t2
    s1 = a0 * a0 + a1 * a1 + a2 * a2
    if s1 > 0:
        n1 = np.sqrt(s1) if dt is not float else math.sqrt(s1)
        a0, a1, a2 = a0 / n1, a1 / n1, a2 / n1
    s2 = xn * xn + yn * yn + one
    n2 = np.sqrt(s2) if dt is not float else math.sqrt(s2)
    return a0 * (xn / n2) + a1 * (yn / n2) + a2 * (one / n2)


def angle_of(d, dt=float):
    """std::acos: NaN outside [-1, 1]"""
    if dt is float:
        return math.acos(d) if -1.0 <= d <= 1.0 else float("nan")
    with np.errstate(invalid="ignore"):
        return np.arccos(d)


def dot_valid(d):
    return -1.0 <= d <= 1.0


def better(d, t, bd, bt):
    return bt < 0 or d > bd or (d == bd and t < bt)


def dot_bound(th):
    """the smallest double whose acos (this host's libm) is below th; 2.0 where there is none"""
    if not math.acos(1.0) < th:
        return 2.0
    if math.acos(-1.0) < th:
        return -1.0
    lo, hi = -1.0, 1.0
    for _ in range(4096):
        mid = lo + (hi - lo) / 2.0
        if not lo < mid < hi:
            break
        if math.acos(mid) < th:
            hi = mid
        else:
            lo = mid
    return hi


# ---------------------------------------------------------------------------------------------------- the create callback
_CPU_CACHE = {}


def cpu_create_for(c):
    """the create callback on the CPU for a case's poses: tests/tri_yardstick.py in float64, kept per list"""
    q, t = np.asarray(c["cam_q"], np.float64), np.asarray(c["cam_t"], np.float64)
    opt = TY.Options()

    def create(lists):
        out = []
        for cams, xy in lists:
            cams, xy = np.asarray(cams, np.int64), np.asarray(xy, np.float64)
            key = (q.tobytes(), t.tobytes(), cams.tobytes(), xy.tobytes())
            if key not in _CPU_CACHE:
                n = len(cams)
                if n > MAX_OBS or n < 2:
                    r = dict(status=3 if n > MAX_OBS else 2, point=np.zeros(3), mask=np.zeros(n, np.uint8), num_inliers=0, num_trials=0, best_trial=-1)
                else:
                    r = TY.run_track(q, t, cams, xy, opt=opt, dtype=np.float64)
                    r = dict(status=int(r["status"]), point=np.asarray(r["point"], np.float64).reshape(3) if r["status"] == 1 else np.zeros(3), mask=np.asarray(r["mask"], np.uint8), num_inliers=int(r["num_inliers"]),
                             num_trials=int(r["num_trials"]), best_trial=int(r["best_trial"]))
                _CPU_CACHE[key] = r
            out.append(_CPU_CACHE[key])
        return out
    return create


# ---------------------------------------------------------------------------------------------------- shared
def frame_of_key(c):
    kp = np.asarray(c["key_ptr"], np.int64)
    return np.repeat(np.arange(len(kp) - 1), np.diff(kp))


def entries(c, k):
    return c["corr_key"][c["corr_ptr"][k]:c["corr_ptr"][k + 1]]


def counts(c, tok):
    """corr_have_point3d [N], visible and measured [n_frames] of a state"""
    kp = c["key_ptr"]
    have = np.array([int(sum(tok[b] >= 0 for b in entries(c, k))) for k in range(kp[-1])], np.int32).reshape(-1)
    vis = np.array([int((have[kp[f]:kp[f + 1]] > 0).sum()) for f in range(len(kp) - 1)], np.int32)
    mea = np.array([int((tok[kp[f]:kp[f + 1]] >= 0).sum()) for f in range(len(kp) - 1)], np.int32)
    return have, vis, mea


def _result(c, tok, status, points, outlier, diag, stats, margins=None):
    have, vis, mea = counts(c, tok)
    N = len(tok)
    ninl, ntr, best = np.zeros(N, np.int32), np.zeros(N, np.int32), np.full(N, -1, np.int32)
    for k, d in diag.items():
        ninl[k], ntr[k], best[k] = d
    return dict(track_of_key=np.asarray(tok, np.int32), key_status=np.asarray(status, np.uint8), n_tracks=len(points), points=np.asarray(points, np.float64).reshape(-1, 3),
                track_outlier=np.asarray(outlier, np.uint8), num_inliers=ninl, num_trials=ntr, best_trial=best, corr_have_point3d=have, visible=vis, measured=mea,
                stats=np.asarray(stats, np.int64), margins=margins or [])


def integer_differences(a, b, stats=8):
    """the names of the integer outputs in which two results differ; stats: how many of the eight are compared"""
    bad = [k for k in INTEGERS if not np.array_equal(np.asarray(a[k]), np.asarray(b[k]))]
    sa = np.asarray(list(a["stats"].values()) if isinstance(a["stats"], dict) else a["stats"])[:stats]
    sb = np.asarray(list(b["stats"].values()) if isinstance(b["stats"], dict) else b["stats"])[:stats]
    return bad + ([] if np.array_equal(sa, sb) else ["stats"])


def point_bits(p):
    return np.ascontiguousarray(np.asarray(p, np.float64)).view(np.uint64)


# ---------------------------------------------------------------------------------------------------- (A) the literal program
def run_literal(c, frames, create, dtype=np.float64):
    dt = float if np.dtype(dtype) == np.float64 else EXT
    fok, kp, reg = frame_of_key(c), c["key_ptr"], c["registered"]
    th = dt(c.get("extend_angle_rad", EXTEND_ANGLE))
    ids = [int(v) for v in c["track_of_key"]]
    tracks = [dict(point=np.array(p, np.float64), outlier=bool(o), obs={}) for p, o in zip(c["points"], c["track_outlier"])]
    for k, t in enumerate(ids):
        if t >= 0:
            tracks[t]["obs"][int(fok[k])] = k
    status, diag, margins = np.zeros(len(ids), np.uint8), {}, []
    n_create = n_zero = n_extend = n_one = n_multi = 0
    for f in frames:
        for p in range(kp[f], kp[f + 1]):
            if ids[p] != -1:
                continue
            observed, obs = set(), []
            for b in entries(c, p):
                if not reg[fok[b]]:
                    continue
                obs.append(int(b))
                if ids[b] != -1:
                    observed.add(ids[b])
            obs.append(p)
            if len(obs) < 2:
                status[p] = 2
                continue
            if not observed:
                n_zero += 1
                r = create([(fok[obs], c["key_xyn"][obs])])[0]
                if r["status"] == 1:                                  # AddTrack on the inlier observations
                    tid = len(tracks)
                    tr = dict(point=np.array(r["point"], np.float64), outlier=False, obs={})
                    for k, inl in zip(obs, r["mask"]):
                        if inl:
                            tr["obs"][int(fok[k])] = k
                            ids[k] = tid
                    tracks.append(tr)
                    n_create += 1
                status[p] = {1: 1, 3: 3}.get(r["status"], 4)
                if r["status"] in (0, 1):
                    diag[p] = (r["num_inliers"], r["num_trials"], r["best_trial"])
                continue
            best, best_angle, seen = -1, dt(100.0), []
            for t in sorted(observed):
                if f in tracks[t]["obs"]:
                    continue
                d = ray_dot(c["cam_q"][f], c["cam_t"][f], tracks[t]["point"], c["key_xyn"][p], dt)
                angle = angle_of(d, dt)
                margins.append(("one", float(abs(EXT(1) - EXT(d))), False))
                if angle == angle:
                    seen.append(angle)
                if angle < best_angle:
                    best, best_angle = t, angle
            seen.sort()
            if len(seen) > 1:
                margins.append(("order", float((seen[1] - seen[0]) / seen[1]) if seen[1] > 0 else 0.0, bool(seen[1] == seen[0])))
            if seen:
                margins.append(("threshold", float(abs(seen[0] - th) / th) if th > 0 else 1.0, False))
            if best_angle < th:
                tracks[best]["obs"][f] = p
                ids[p] = best
                n_extend += 1
                status[p] = 5
            else:
                status[p] = 6
            if len(observed) == 1:
                n_one += 1
            else:
                n_multi += 1
    return _result(c, np.array(ids, np.int32), status, [t["point"] for t in tracks], [t["outlier"] for t in tracks], diag,
                   [n_create, n_zero, n_extend, n_one, n_multi, 0, 0, 0], margins)


# ---------------------------------------------------------------------------------------------------- (B) the flat program
def plan(c, frames):
    """the slots, their lists and the steps, as csrc/ba_trif_rule.h: make_plan"""
    fok, kp, reg, tok = frame_of_key(c), c["key_ptr"], c["registered"], c["track_of_key"]
    slot_key, lists, steps, status0, split = [], [], [], np.zeros(len(tok), np.uint8), 0
    for f in frames:
        run, runs, marked = [], 0, set()
        for p in range(kp[f], kp[f + 1]):
            if tok[p] != -1:
                continue
            obs = [int(b) for b in entries(c, p) if reg[fok[b]]]
            if not obs:
                status0[p] = 2
                continue
            free = {b for b in obs if tok[b] == -1}                  # (an entry that carries a track at the start keeps it: no create writes it)
            if run and marked & free:                                 # coupled with a slot of the open run
                steps.append((f, run))
                run, marked = [], set()
            if not run:
                runs += 1
            marked |= free
            run.append(len(slot_key))
            slot_key.append(p)
            lists.append(obs + [p])
        if run:
            steps.append((f, run))
        split += runs > 1
    return dict(slot_key=slot_key, lists=lists, steps=steps, status0=status0, split=split)


def all_lists(c, frames):
    """every slot's list as the create callback takes it"""
    fok = frame_of_key(c)
    return [(fok[l], c["key_xyn"][l]) for l in plan(c, frames)["lists"]]


def capacity(c, frames):
    return len(c["points"]) + len(plan(c, frames)["slot_key"])


def run_flat(c, frames, create):
    fok, kp = frame_of_key(c), c["key_ptr"]
    P = plan(c, frames)
    tok = np.array(c["track_of_key"], np.int32)
    points, outlier = [np.array(p, np.float64) for p in c["points"]], [int(o) for o in c["track_outlier"]]
    status, diag = P["status0"].copy(), {}
    dot_min = dot_bound(float(c.get("extend_angle_rad", EXTEND_ANGLE)))
    cap = len(points) + len(P["slot_key"])
    held, bid = np.zeros(cap, np.int64), np.full(cap, NO_BID, np.int64)
    stats = [0] * 8
    T0, events, made_in, first_step = len(points), set(), {}, {}
    for step, (f, slots) in enumerate(P["steps"]):
        stamp = step + 1
        first_step.setdefault(f, step)
        if len(slots) > 256:
            events.add("wide_step")
        for k in range(kp[f], kp[f + 1]):
            if tok[k] >= 0:
                held[tok[k]] = stamp
        cand, todo_create, undecided = {}, [], []
        for s in slots:                                               # the branch of every slot, on the state at the step's start
            p, obs = P["slot_key"][s], P["lists"][s][:-1]
            if tok[p] != -1:
                events.add("not_visited")
                continue
            if any(not c["registered"][fok[b]] for b in entries(c, p)):
                events.add("unregistered_skipped")
            distinct, cs, low = [], [], False
            for b in obs:
                t = int(tok[b])
                if t < 0 or t in distinct:
                    continue
                distinct.append(t)
                if t >= T0 and made_in[t] == (f, "earlier run"):
                    events.add("coupled_sees_new_track")
                if held[t] == stamp:
                    events.add("holds_frame")
                    continue
                d = ray_dot(c["cam_q"][f], c["cam_t"][f], points[t], c["key_xyn"][p])
                if d == 0.0:
                    events.add("zero_ray")
                if dot_valid(d) and d >= dot_min:
                    cs.append((t, d))
                else:
                    low = True
            if distinct and all(held[t] == stamp for t in distinct):
                events.add("all_ineligible")
            if low and not cs:
                events.add("rejected")
            if len(distinct) > 1:
                events.add("multi_track")
            if not distinct:
                stats[1] += 1
                todo_create.append(s)
            else:
                stats[3 if len(distinct) == 1 else 4] += 1
                cand[s] = cs
                undecided.append(s)
        short = [s for s in todo_create if len(P["lists"][s]) <= MAX_OBS]
        events |= {"list_%d" % len(P["lists"][s]) for s in todo_create if len(P["lists"][s]) in (128, 129)}
        for s in todo_create:
            if len(P["lists"][s]) > MAX_OBS:
                status[P["slot_key"][s]] = 3
        made = create([(fok[P["lists"][s]], c["key_xyn"][P["lists"][s]]) for s in short]) if short else []
        for s, r in zip(short, made):                                 # ids in key order
            p = P["slot_key"][s]
            diag[p] = (r["num_inliers"], r["num_trials"], r["best_trial"])
            if r["status"] != 1:
                status[p] = 4
                continue
            tid = len(points)
            made_in[tid] = f
            if not all(r["mask"]):
                events.add("outliers_left")
            points.append(np.array(r["point"], np.float64)); outlier.append(0)
            for k, inl in zip(P["lists"][s], r["mask"]):
                if inl:
                    tok[k] = tid
            status[p] = 1
            stats[0] += 1
        rounds = 0
        for _ in range(len(slots) + 1):                               # the claims: rounds of bids
            if not undecided:
                break
            rounds += 1
            for s in undecided:
                for t, _d in cand[s]:
                    if held[t] != stamp:
                        bid[t] = min(bid[t], s)
            won, left = [], []
            for s in undecided:
                bt, bd = -1, 0.0
                for t, d in cand[s]:
                    if held[t] != stamp and bt >= 0 and d == bd:
                        events.add("tie")
                    if held[t] != stamp and better(d, t, bd, bt):
                        bt, bd = t, d
                if bt < 0:
                    status[P["slot_key"][s]] = 6
                elif bid[bt] == s:
                    won.append((s, bt))
                else:
                    left.append(s)
            for s in undecided:
                for t, _d in cand[s]:
                    bid[t] = NO_BID
            for s, bt in won:
                held[bt] = stamp
                tok[P["slot_key"][s]] = bt
                status[P["slot_key"][s]] = 5
                stats[2] += 1
                events.add("accepted")
                if bt >= T0 and made_in[bt] not in (f, (f, "earlier run")):
                    events.add("later_frame_extends_created")
            undecided = left
        assert not undecided
        stats[7] = max(stats[7], rounds)
        if rounds in (3, 64, 65, 200):
            events.add("rounds_%d" % rounds)
        for t in made_in:                                             # the tracks this frame created are "earlier run" for its later steps
            if made_in[t] == f:
                made_in[t] = (f, "earlier run")
    stats[5], stats[6] = len(P["steps"]), P["split"]
    r = _result(c, tok, status, points, outlier, diag, stats)
    r["events"] = events
    return r
