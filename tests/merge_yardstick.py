"""The yardstick of track completion and merging: ContinueTrack, MergeTrack and MergeTracks of the reference
(src/geometry/track_processor.cc:426-618) restated twice.

  (A) run_literal: a literal restatement on dicts (Track::observations_ as a map walked in key order, Frame::track_ids_ as lists,
      the correspondence lists of every key point), the whole map in global order, in float64 (Python floats) or np.longdouble.  It
      also notes which rules of the catalogue it met and how close every comparison came to max_reproj_error.
  (B) run_components: the component-wise program on flat arrays (union-find, per component the keys ascending with local lists,
      the tracks ascending, the loops over local arrays), in float64.

A case is a dict: key_ptr, key_xy, registered, cam_q (x, y, z, w), cam_t, cam_intr, intr_model, intr_params, corr_ptr, corr_key,
points, track_outlier, track_of_key, max_re, frame (of mode 4)."""
import math

import numpy as np

CONTINUE, MERGE, FRAME = 1, 2, 4
MODES = (1, 2, 3, 4)
MAX_KEYS, MAX_TRACKS = 1024, 512

RULES = (
    "a merge that succeeds", "a merge that fails on t's own observation", "a merge that fails on t2's observation", "a same-frame conflict inside a merge",
    "a visited track not retried after t's point moved", "a second merge whose verdict depends on the moved point",
    "frame mode: an observation gained in a later frame is visited", "frame mode: an observation gained in an earlier frame is not visited",
    "frame mode: a seed key reset by an earlier seed's merge", "a continue blocked by a frame gained a step earlier", "two tracks compete for one free key",
    "an unregistered neighbour frame", "a point behind a camera", "z == 0: NaN in a merge test", "z == 0: NaN in a map-mode continue", "z == 0: NaN in a frame-mode continue",
    "a track with one observation", "exactly max_reproj_error in a merge test", "exactly max_reproj_error in a map-mode continue",
    "exactly max_reproj_error in a frame-mode continue", "a component of 63 keys", "a component of 64 keys", "a component of 65 keys", "a component of 128 keys",
    "a component of 129 keys", "a track with 64 observations", "a track with 65 observations", "a component of exactly 1024 keys", "a component of 1025 keys",
    "a component of exactly 512 tracks", "a component of 513 tracks",
)


# ---------------------------------------------------------------------------------------------------- the error
def _div(a, b):
    if isinstance(a, float) and isinstance(b, float):
        try:
            return a / b
        except ZeroDivisionError:
            return math.nan if (a == 0.0 or a != a) else math.copysign(math.inf, a) * math.copysign(1.0, b)
    with np.errstate(all="ignore"):
        return a / b


def _sqrt(a):
    if isinstance(a, float):
        return math.sqrt(a) if a >= 0.0 else math.nan if a == a else a
    with np.errstate(all="ignore"):
        return np.sqrt(a)


def reprojection_error(cam, P, u, v):
    """Reprojection_Error (track_processor.cc:19-26), one rounding per operation, in the operands' type.  cam: (q, t, model, k).
    -> (re, depth)"""
    (x, y, z, w), t, model, k = cam
    two = type(x)(2.0)
    one = type(x)(1.0)
    M0, M1, M2 = one - two * (y * y + z * z), two * (x * y - w * z), two * (x * z + w * y)
    M3, M4, M5 = two * (x * y + w * z), one - two * (x * x + z * z), two * (y * z - w * x)
    M6, M7, M8 = two * (x * z - w * y), two * (y * z + w * x), one - two * (x * x + y * y)
    X = M0 * P[0] + M1 * P[1] + M2 * P[2] + t[0]
    Y = M3 * P[0] + M4 * P[1] + M5 * P[2] + t[1]
    Z = M6 * P[0] + M7 * P[1] + M8 * P[2] + t[2]
    with np.errstate(all="ignore"):
        xn, yn = _div(X, Z), _div(Y, Z)
        r2 = xn * xn + yn * yn
        if model == 0:
            fx, fy, cx, cy, du, dv = k[0], k[0], k[1], k[2], xn, yn
        elif model == 1:
            fx, fy, cx, cy, du, dv = k[0], k[1], k[2], k[3], xn, yn
        elif model == 2:
            fx, fy, cx, cy, du, dv = k[0], k[0], k[1], k[2], xn * (k[3] * r2), yn * (k[3] * r2)
        elif model == 3:
            fx, fy, cx, cy, du, dv = k[0], k[1], k[2], k[3], xn * (k[4] * r2), yn * (k[4] * r2)
        else:
            fx, fy, cx, cy = k[0], k[1], k[2], k[3]
            rad, xy = k[4] * r2 + k[5] * r2 * r2, xn * yn
            du = xn * rad + two * k[6] * xy + k[7] * (r2 + two * xn * xn)
            dv = yn * rad + two * k[7] * xy + k[6] * (r2 + two * yn * yn)
        e0, e1 = fx * (xn + du) + cx - u, fy * (yn + dv) + cy - v
        return _sqrt(e0 * e0 + e1 * e1), Z


def merged_point(w1, P1, w2, P2):
    s = w1 + w2
    return [_div(w1 * P1[k] + w2 * P2[k], s) for k in range(3)]


def _cams(case, ft):
    c = lambda v: ft(float(v))
    out = []
    for f in range(len(case["registered"])):
        ci = int(case["cam_intr"][f])
        out.append((tuple(c(v) for v in case["cam_q"][f]), tuple(c(v) for v in case["cam_t"][f]), int(case["intr_model"][ci]), tuple(c(v) for v in case["intr_params"][ci])))
    return out


# ---------------------------------------------------------------------------------------------------- (A) the literal restatement
class _Map:
    def __init__(self, case, ft):
        self.ft = ft
        kp = case["key_ptr"]
        self.n = len(kp) - 1
        self.kp = [int(x) for x in kp]
        self.cams = _cams(case, ft)
        self.registered = [bool(x) for x in case["registered"]]
        frame_of = np.repeat(np.arange(self.n), np.diff(kp))
        self.xy = [[(ft(float(u)), ft(float(v))) for u, v in case["key_xy"][kp[f]:kp[f + 1]]] for f in range(self.n)]
        self.track_ids = [[int(t) for t in case["track_of_key"][kp[f]:kp[f + 1]]] for f in range(self.n)]
        cp, ck = case["corr_ptr"], case["corr_key"]
        self.corrs = [[[(int(frame_of[g]), int(g - kp[frame_of[g]])) for g in ck[cp[kp[f] + k]:cp[kp[f] + k + 1]]] for k in range(kp[f + 1] - kp[f])] for f in range(self.n)]
        T = len(case["points"])
        self.point = [[ft(float(v)) for v in case["points"][t]] for t in range(T)]
        self.outlier = [bool(x) for x in case["track_outlier"]]
        self.obs = [dict() for _ in range(T)]
        for f in range(self.n):
            for k, t in enumerate(self.track_ids[f]):
                if t >= 0:
                    self.obs[t][f] = k
        self.max_re = ft(float(case["max_re"]))
        self.counters = [0, 0, 0, 0]
        self.rules = set()
        self.margins = []                      # (|re - max_re|, form, exact or NaN) of every comparison
        self.involved = [max(abs(float(v)) for v in case["points"][t]) if T else 0.0 for t in range(T)]
        self.initial_ids = [list(v) for v in self.track_ids]
        self.received = set()                  # tracks whose point a merge has set
        self.by_continue = set()               # keys that gained their track by a continue of this run

    def re(self, f, k, P, form):
        r, Z = reprojection_error(self.cams[f], P, *self.xy[f][k])
        if Z < 0:
            self.rules.add("a point behind a camera")
        nan = r != r
        if nan and Z == 0:
            self.rules.add("z == 0: NaN in " + form)
        if r == self.max_re:
            self.rules.add("exactly max_reproj_error in " + form)
        self.margins.append((math.inf if nan else abs(float(r - self.max_re)), form, bool(nan or r == self.max_re)))
        return r

    def observations(self, t, live):
        """the walk of a range-for over observations_: a snapshot, or the live map (what is inserted beyond the iterator is met)"""
        obs = self.obs[t]
        if not live:
            for f in sorted(obs):
                yield f, obs[f]
            return
        cur = min(obs) if obs else None
        while cur is not None:
            yield cur, obs[cur]
            later = [f for f in obs if f > cur]
            cur = min(later) if later else None

    def merge(self, t, live):
        form = "a merge test"
        obs = self.obs[t]
        start_frames, walked = set(obs), set()
        start_point, moved = list(self.point[t]), 0
        if len(obs) == 1:
            self.rules.add("a track with one observation")
        visited = {}
        for f, k in self.observations(t, live):
            walked.add(f)
            if f not in start_frames:
                self.rules.add("frame mode: an observation gained in a later frame is visited")
            for cf, ck in self.corrs[f][k]:
                if cf in obs:
                    continue
                if not self.registered[cf]:
                    self.rules.add("an unregistered neighbour frame")
                    continue
                t2 = self.track_ids[cf][ck]
                if t2 == -1:
                    continue
                if t2 in visited:
                    if moved > visited[t2]:
                        self.rules.add("a visited track not retried after t's point moved")
                    continue
                self.counters[1] += 1
                visited[t2] = moved
                obs2 = self.obs[t2]
                for n_obs in (len(obs), len(obs2)):
                    if n_obs in (64, 65):
                        self.rules.add("a track with %d observations" % n_obs)
                w1, w2 = self.ft(float(len(obs))), self.ft(float(len(obs2)))
                m = merged_point(w1, self.point[t], w2, self.point[t2])
                ok, failed_on = True, None
                for which, o in (("t's own", obs), ("t2's", obs2)):
                    for tf in sorted(o):
                        if self.re(tf, o[tf], m, form) > self.max_re:
                            ok, failed_on = False, which
                            break
                    if not ok:
                        break
                if moved:                      # would the verdict be another with the point t had when the loop began?
                    m0 = merged_point(w1, start_point, w2, self.point[t2])
                    keep, self.margins = self.margins, []
                    rules = set(self.rules)
                    ok0 = not any(self.re(tf, o[tf], m0, form) > self.max_re for o in (obs, obs2) for tf in sorted(o))
                    self.margins, self.rules = keep, rules
                    if ok0 != ok:
                        self.rules.add("a second merge whose verdict depends on the moved point")
                if not ok:
                    self.rules.add("a merge that fails on %s observation" % failed_on)
                    continue
                self.rules.add("a merge that succeeds")
                self.counters[0] += 1
                moved += 1
                self.point[t] = m
                self.received.add(t)
                self.involved[t] = max(self.involved[t], self.involved[t2])
                for tf in sorted(obs2):
                    tk = obs2[tf]
                    if tf not in obs:
                        obs[tf] = tk
                        self.track_ids[tf][tk] = t
                    else:
                        self.track_ids[tf][tk] = -1
                        self.rules.add("a same-frame conflict inside a merge")
                self.outlier[t2] = True
        if live and any(f not in start_frames and f not in walked for f in obs):
            self.rules.add("frame mode: an observation gained in an earlier frame is not visited")

    def continue_(self, t, live):
        form = "a frame-mode continue" if live else "a map-mode continue"
        obs = self.obs[t]
        start_frames = set(obs)
        if len(obs) == 1:
            self.rules.add("a track with one observation")
        visited = set()
        for f, k in self.observations(t, live):
            for cf, ck in self.corrs[f][k]:
                if cf in obs:
                    if cf not in start_frames and self.track_ids[cf][ck] == -1:
                        self.rules.add("a continue blocked by a frame gained a step earlier")
                    continue
                if not self.registered[cf]:
                    self.rules.add("an unregistered neighbour frame")
                    continue
                if self.track_ids[cf][ck] != -1 or (cf, ck) in visited:
                    if (cf, ck) in self.by_continue and self.track_ids[cf][ck] != t:
                        self.rules.add("two tracks compete for one free key")
                    continue
                self.counters[3] += 1
                visited.add((cf, ck))
                r = self.re(cf, ck, self.point[t], form)
                if (r < self.max_re) if live else (not r > self.max_re):
                    self.counters[2] += 1
                    obs[cf] = ck
                    self.track_ids[cf][ck] = t
                    self.by_continue.add((cf, ck))

    def run(self, mode, frame):
        T = len(self.point)
        if mode == FRAME:
            for k in range(len(self.track_ids[frame])):
                t = self.track_ids[frame][k]           # read live
                if t == -1:
                    if self.initial_ids[frame][k] != -1:
                        self.rules.add("frame mode: a seed key reset by an earlier seed's merge")
                    continue
                self.merge(t, True)
                self.continue_(t, True)
            return
        if mode & CONTINUE:
            for t in range(T):
                if not self.outlier[t]:
                    self.continue_(t, False)
        if mode & MERGE:
            for t in range(T):
                if not self.outlier[t]:
                    self.merge(t, False)


def components(case):
    """comp_of_key [N] with the components by size (largest first, then first key), and their sizes"""
    N = int(case["key_ptr"][-1])
    parent = list(range(N))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    def join(a, b):
        a, b = find(a), find(b)
        if a != b:
            parent[max(a, b)] = min(a, b)

    cp, ck, tok = case["corr_ptr"], case["corr_key"], case["track_of_key"]
    seen = {}
    for k in range(N):
        for g in ck[cp[k]:cp[k + 1]]:
            join(k, int(g))
        if tok[k] >= 0:
            join(k, seen.setdefault(int(tok[k]), k))
    roots = [find(k) for k in range(N)]
    size = {}
    for r in roots:
        size[r] = size.get(r, 0) + 1
    order = sorted(size, key=lambda r: (-size[r], r))
    idx = {r: c for c, r in enumerate(order)}
    return np.array([idx[r] for r in roots], np.int32), [size[r] for r in order]


def _plan(case, mode, frame):
    """the components in order: (keys, tracks, processed, above a limit)"""
    comp, sizes = components(case)
    N = len(comp)
    frame_of = np.repeat(np.arange(len(case["key_ptr"]) - 1), np.diff(case["key_ptr"]))
    keys_of = [[] for _ in sizes]
    for k in range(N):
        keys_of[comp[k]].append(k)
    out = []
    tok = case["track_of_key"]
    for keys in keys_of:
        tracks = sorted({int(tok[k]) for k in keys if tok[k] >= 0})
        wanted = any(tok[k] >= 0 and (mode != FRAME or frame_of[k] == frame) for k in keys)
        over = len(keys) > MAX_KEYS or len(tracks) > MAX_TRACKS
        out.append((keys, tracks, wanted and not over, wanted and over))
    return out, frame_of


def _outputs(case, tok, points, outlier, status, counters, plan):
    cp, ck = case["corr_ptr"], case["corr_key"]
    kp = case["key_ptr"]
    N = len(tok)
    have = np.array([sum(1 for g in ck[cp[k]:cp[k + 1]] if tok[g] >= 0) for k in range(N)], np.int32)
    n = len(kp) - 1
    done = [len(keys) for keys, _, processed, _ in plan if processed]
    stats = list(counters) + [len(done), sum(1 for p in plan if p[3]), max(done) if done else 0, 0]
    return dict(track_of_key=np.array(tok, np.int32), points=points, track_outlier=np.array(outlier, np.uint8), track_status=np.array(status, np.uint8), corr_have_point3d=have,
                visible=np.array([int((have[kp[f]:kp[f + 1]] > 0).sum()) for f in range(n)], np.int32),
                measured=np.array([int((np.asarray(tok[kp[f]:kp[f + 1]]) >= 0).sum()) for f in range(n)], np.int32), stats=np.array(stats, np.int64))


def run_literal(case, mode, ft=float):
    """(A).  Components above a limit are taken out beforehand (the call does not attempt them); the rest runs as one map in global
    order.  -> the outputs, and rules / margins / involved for the catalogue's tables"""
    plan, _ = _plan(case, mode, case["frame"])
    c = dict(case, track_of_key=np.array(case["track_of_key"], np.int32))
    status = [0] * len(case["points"])
    for keys, tracks, processed, over in plan:
        if not processed:
            c["track_of_key"][keys] = -1          # neither skipped nor unwanted components are walked (their keys reach no other component)
        for t in tracks:
            status[t] = 1 if processed else 3 if over else 0
    m = _Map(c, ft)
    N, T = int(case["key_ptr"][-1]), len(case["points"])
    no_work = N == 0 or T == 0 or (mode == FRAME and not any(t >= 0 for t in case["track_of_key"][case["key_ptr"][case["frame"]]:case["key_ptr"][case["frame"] + 1]]))
    if not no_work:
        m.run(mode, case["frame"])
    tok = np.array(case["track_of_key"], np.int32)
    flat = np.array([t for f in m.track_ids for t in f], np.int32)
    outlier = np.array(case["track_outlier"], np.uint8)
    for keys, tracks, processed, _ in plan:
        if processed:
            tok[keys] = flat[keys]
            for t in tracks:
                if m.outlier[t]:
                    outlier[t], status[t] = 1, 2
    if no_work:
        status, plan = [0] * T, []
    out = _outputs(case, tok, m.point, outlier, status, m.counters, plan)
    out.update(rules=m.rules, margins=m.margins, involved=m.involved, received=sorted(m.received))
    return out


# ---------------------------------------------------------------------------------------------------- (B) component-wise, flat arrays
def run_components(case, mode):
    frame = case["frame"]
    plan, frame_of = _plan(case, mode, frame)
    cams = _cams(case, float)
    reg = case["registered"]
    xy = [(float(u), float(v)) for u, v in case["key_xy"]]
    cp, ck = case["corr_ptr"], case["corr_key"]
    max_re = float(case["max_re"])
    tok = np.array(case["track_of_key"], np.int32)
    points = [[float(v) for v in p] for p in case["points"]]
    outlier = np.array(case["track_outlier"], np.uint8)
    status = [0] * len(points)
    counters = [0, 0, 0, 0]
    N, T = len(tok), len(points)
    if N == 0 or T == 0 or (mode == FRAME and not any(t >= 0 for t in tok[case["key_ptr"][frame]:case["key_ptr"][frame + 1]])):
        return _outputs(case, tok, points, outlier, status, counters, [])
    for keys, tracks, processed, over in plan:
        if over:
            for t in tracks:
                status[t] = 3
        if not processed:
            continue
        nk, nt = len(keys), len(tracks)
        local = {g: i for i, g in enumerate(keys)}
        ltrack = {t: j for j, t in enumerate(tracks)}
        fr = [int(frame_of[g]) for g in keys]
        trk = [ltrack[int(tok[g])] if tok[g] >= 0 else -1 for g in keys]
        lists = [[local[int(g)] for g in ck[cp[k]:cp[k + 1]]] for k in keys]
        pts = [list(points[t]) for t in tracks]
        out = [False] * nt
        size = [trk.count(j) for j in range(nt)]
        has_frame = lambda t, f: any(trk[i] == t and fr[i] == f for i in range(nk))

        def walk(t, live):
            snap = [trk[i] == t for i in range(nk)]
            pos = -1
            while True:
                nxt = next((i for i in range(pos + 1, nk) if (trk[i] == t if live else snap[i])), nk)
                if nxt == nk:
                    return
                pos = nxt
                yield nxt

        def merge(t, live):
            mark = [False] * nt
            for k in walk(t, live):
                for c in lists[k]:
                    if has_frame(t, fr[c]) or not reg[fr[c]]:
                        continue
                    t2 = trk[c]
                    if t2 < 0 or mark[t2]:
                        continue
                    mark[t2] = True
                    counters[1] += 1
                    m = merged_point(float(size[t]), pts[t], float(size[t2]), pts[t2])
                    if any((trk[i] == t or trk[i] == t2) and reprojection_error(cams[fr[i]], m, *xy[keys[i]])[0] > max_re for i in range(nk)):
                        continue
                    counters[0] += 1
                    pts[t] = m
                    for i in range(nk):
                        if trk[i] == t2:
                            if has_frame(t, fr[i]):
                                trk[i] = -1
                            else:
                                trk[i] = t
                                size[t] += 1
                    size[t2] = 0
                    out[t2] = True

        def cont(t, live):
            mark = [False] * nk
            for k in walk(t, live):
                for c in lists[k]:
                    if has_frame(t, fr[c]) or not reg[fr[c]] or trk[c] >= 0 or mark[c]:
                        continue
                    mark[c] = True
                    counters[3] += 1
                    r = reprojection_error(cams[fr[c]], pts[t], *xy[keys[c]])[0]
                    if (r < max_re) if live else (not r > max_re):
                        counters[2] += 1
                        trk[c] = t
                        size[t] += 1

        if mode == FRAME:
            for i in range(nk):
                if fr[i] == frame and trk[i] >= 0:
                    t = trk[i]
                    merge(t, True)
                    cont(t, True)
        else:
            if mode & CONTINUE:
                for t in range(nt):
                    if not out[t]:
                        cont(t, False)
            if mode & MERGE:
                for t in range(nt):
                    if not out[t]:
                        merge(t, False)
        for i, g in enumerate(keys):
            tok[g] = tracks[trk[i]] if trk[i] >= 0 else -1
        for j, t in enumerate(tracks):
            points[t] = pts[j]
            status[t] = 2 if out[j] else 1
            if out[j]:
                outlier[t] = 1
    return _outputs(case, tok, points, outlier, status, counters, plan)


# ---------------------------------------------------------------------------------------------------- comparing
INTEGERS = ("track_of_key", "track_outlier", "track_status", "corr_have_point3d", "visible", "measured", "stats")


def integer_differences(a, b):
    """the names of the integer outputs in which two results differ"""
    return [k for k in INTEGERS if not np.array_equal(np.asarray(a[k]), np.asarray(b[k]))]


def point_bits(points):
    return np.array([[float(v) for v in p] for p in points], np.float64).reshape(-1, 3).view(np.uint64)


def point_bars(r64, rld):
    """per track the bar of a merged point against the longdouble value: 16 x the float64 restatement's own deviation from it,
    at least 4 ulp of the largest coordinate involved.  Nothing of a result under test enters."""
    bars = []
    for t in range(len(r64["points"])):
        dev = max(abs(float(np.longdouble(r64["points"][t][k]) - rld["points"][t][k])) for k in range(3))
        big = max(r64["involved"][t], max(abs(float(v)) for v in rld["points"][t]))
        bars.append(max(16.0 * dev, 4.0 * float(np.spacing(np.float64(big)))))
    return bars
