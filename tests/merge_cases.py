"""The catalogue of track completion and merging: cases for tests/merge_yardstick.py, the library and the stand-alone host program.

  rules    (frame 0) one small component per rule in a toy world: every camera has the identity pose and the pinhole parameters
           (0.5, 0.5, 0, 0), so a point (x, y, 1) lands on pixel (x, y) (the pinhole models double the focal length) and every
           error is the distance between integers: the merges that succeed and fail, the conflict, the visited and the moved
           point, the competition for a free key, the blocked continue, the unregistered frame, the point behind the camera, z == 0
           and the error of exactly max_reproj_error in all three comparison forms
  live     (frame 2) what only the live walk of MergeTracks shows: an observation gained in a later frame is visited, one gained
           in an earlier frame is not, a seed key is reset by an earlier seed's merge
  sizes    chains of 63, 64, 65, 128 and 129 keys over 70 frames; tracks of 64 and of 65 observations
  limits   chains of exactly 1024 keys, of 1025 keys, of exactly 512 tracks and of 513 tracks
  scene_a, scene_b   random scenes (24 x up to 200 and 40 x up to 200 keys): points projected through posed cameras of the models 0..4,
           tracks in fragments, free observations, wrong correspondences

The constructed rule cases stay within 12 frames x 40 keys; the size cases need a frame per observation of their longest track
and a key per key of their largest component, so they do not.  coverage(name) is the table: which rule a case meets in any mode."""
import functools

import numpy as np

from tests import merge_yardstick as Y

NAMES = ("rules", "live", "sizes", "limits", "scene_a", "scene_b")
QUICK = ("rules", "live", "sizes", "scene_a", "scene_b")          # everything but the 1024-key chains


def build(n_frames, keys, edges, points, frame=0, registered=None, max_re=8.0, cams=None):
    """keys: (name, frame, u, v, track or -1); edges: (name, name) in Map::Init's insertion order; points: {track: (x, y, z)}"""
    order = sorted(range(len(keys)), key=lambda i: keys[i][1])            # stable: frame-major, a frame's keys in the order given
    index = {keys[i][0]: g for g, i in enumerate(order)}
    assert len(index) == len(keys)
    fr = np.array([keys[i][1] for i in order], np.int64)
    key_ptr = np.searchsorted(fr, np.arange(n_frames + 1)).astype(np.int64)
    lists = [[] for _ in keys]
    for a, b in edges:
        lists[index[a]].append(index[b])
        lists[index[b]].append(index[a])
    corr_ptr = np.concatenate([[0], np.cumsum([len(v) for v in lists])]).astype(np.int64)
    T = max(points) + 1 if points else 0
    c = dict(key_ptr=key_ptr, key_xy=np.array([[keys[i][2], keys[i][3]] for i in order], np.float64).reshape(-1, 2),
             registered=np.array([1] * n_frames if registered is None else registered, np.uint8),
             corr_ptr=corr_ptr, corr_key=np.array([g for v in lists for g in v], np.int32), points=np.array([points[t] for t in range(T)], np.float64).reshape(-1, 3),
             track_outlier=np.zeros(T, np.uint8), track_of_key=np.array([keys[i][4] for i in order], np.int32), max_re=float(max_re), frame=int(frame), index=index)
    if cams is None:                          # the toy world
        cams = dict(cam_q=np.tile([0.0, 0.0, 0.0, 1.0], (n_frames, 1)), cam_t=np.zeros((n_frames, 3)), cam_intr=np.zeros(n_frames, np.int32),
                    intr_model=np.array([1], np.int32), intr_params=np.array([[0.5, 0.5, 0, 0, 0, 0, 0, 0]], np.float64))
    c.update(cams)
    return c


class _Toy:
    def __init__(self):
        self.keys, self.edges, self.points = [], [], {}

    def track(self, point, obs):
        """a track at `point` with obs (name, frame, u, v); -> its id"""
        t = len(self.points)
        self.points[t] = point
        self.keys += [(n, f, u, v, t) for n, f, u, v in obs]
        return t

    def free(self, name, frame, u, v):
        self.keys.append((name, frame, u, v, -1))

    def edge(self, *pairs):
        self.edges += list(pairs)


def _rules():
    w = _Toy()
    # a merge that succeeds: m = (2, 0, 1), every error 2
    w.track((0, 0, 1), [("a0", 0, 0, 0), ("a1", 1, 0, 0)]); w.track((4, 0, 1), [("b2", 2, 4, 0), ("b3", 3, 4, 0)]); w.edge(("a1", "b2"))
    # fails on t's own observation (one observation; m = (30, 0, 1))
    w.track((0, 0, 1), [("c0", 0, 0, 0)]); w.track((40, 0, 1), [("d1", 1, 40, 0), ("d2", 2, 40, 0), ("d3", 3, 40, 0)]); w.edge(("c0", "d1"))
    # fails on t2's: m = (7, 0, 1), t's errors 7, t2's 21
    w.track((0, 0, 1), [("e0", 0, 0, 0), ("e1", 1, 0, 0), ("e2", 2, 0, 0)]); w.track((28, 0, 1), [("f3", 3, 28, 0)]); w.edge(("e2", "f3"))
    # a same-frame conflict: both tracks have a key in frame 1
    w.track((0, 0, 1), [("g0", 0, 0, 0), ("g1", 1, 0, 0)]); w.track((0, 0, 1), [("h1", 1, 0, 0), ("h2", 2, 0, 0)]); w.edge(("g0", "h2"))
    # visited and not retried; a verdict that depends on the moved point: i0's list is j1 (fails: m = (20, 0, 1)), k2 (merges: the point moves
    # to (4, 0, 1)), j3 (the same track again: skipped), l4 (m = (7, 0, 1) passes; from the first point m = (13/3, 0, 1) would leave l4 8.67 away)
    w.track((0, 0, 1), [("i0", 0, 0, 0)]); w.track((30, 0, 1), [("j1", 1, 30, 0), ("j3", 3, 30, 0)]); w.track((8, 0, 1), [("k2", 2, 8, 0)]); w.track((13, 0, 1), [("l4", 4, 13, 0)])
    w.edge(("i0", "j1"), ("i0", "k2"), ("i0", "j3"), ("i0", "l4"))
    # two tracks compete for the free key z2; an unregistered neighbour frame (6)
    w.track((0, 0, 1), [("m0", 0, 0, 0)]); w.track((0, 0, 1), [("n1", 1, 0, 0)]); w.free("z2", 2, 0, 0); w.free("u6", 6, 0, 0)
    w.edge(("m0", "z2"), ("n1", "z2"), ("m0", "u6"))
    # a continue blocked because the track gained frame 3 a step earlier
    w.track((0, 0, 1), [("o0", 0, 0, 0)]); w.free("p3", 3, 0, 0); w.free("q3", 3, 0, 0); w.edge(("o0", "p3"), ("o0", "q3"))
    # a point behind the camera: (0, 0, -1) lands on (0, 0)
    w.track((0, 0, -1), [("r0", 0, 0, 0)]); w.free("r1", 1, 0, 0); w.edge(("r0", "r1"))
    # z == 0 under the identity pose: NaN in a merge test (s0 / s1) and in a continue (t0 / t1)
    w.track((0, 0, 0), [("s0", 0, 0, 0)]); w.track((0, 0, 0), [("s1", 1, 0, 0)]); w.edge(("s0", "s1"))
    w.track((0, 0, 0), [("t0", 0, 0, 0)]); w.free("t1", 1, 0, 0); w.edge(("t0", "t1"))
    # an error of exactly 8: a merge (m = (8, 0, 1) between keys at 0 and 16) and a continue (a key 8 away)
    w.track((0, 0, 1), [("v0", 0, 0, 0)]); w.track((16, 0, 1), [("v1", 1, 16, 0)]); w.edge(("v0", "v1"))
    w.track((0, 0, 1), [("x0", 0, 0, 0)]); w.free("x1", 1, 8, 0); w.edge(("x0", "x1"))
    return build(7, w.keys, w.edges, w.points, frame=0, registered=[1, 1, 1, 1, 1, 1, 0])


def _live():
    w = _Toy()
    # the seed s2's list: x4 (frame 4, later: visited in the same loop, so z5 merges too), y1 (frame 1, earlier: not visited, so w0 stays)
    w.track((0, 0, 1), [("s2", 2, 0, 0)]); w.track((0, 0, 1), [("x4", 4, 0, 0)]); w.track((0, 0, 1), [("y1", 1, 0, 0)]); w.track((0, 0, 1), [("z5", 5, 0, 0)])
    w.track((0, 0, 1), [("w0", 0, 0, 0)])
    w.edge(("s2", "x4"), ("s2", "y1"), ("x4", "z5"), ("y1", "w0"))
    # the second seed c2 is reset when the first seed's track merges its track through a3 - b4
    w.track((0, 0, 1), [("a2", 2, 0, 0), ("a3", 3, 0, 0)]); w.track((0, 0, 1), [("c2", 2, 0, 0), ("b4", 4, 0, 0)]); w.edge(("a3", "b4"))
    # the continue loop of a seed: free keys in a later and in an earlier frame, one of them 9 away
    w.track((0, 0, 1), [("d2", 2, 0, 0)]); w.free("d3", 3, 0, 0); w.free("d1", 1, 9, 0); w.free("e5", 5, 0, 0); w.edge(("d2", "d3"), ("d2", "d1"), ("d3", "e5"))
    return build(6, w.keys, w.edges, w.points, frame=2)


def _chains(specs, n_frames=70):
    """per (keys, observations per track): a chain key i - key i + 1, key i in frame i % n_frames, tracks of consecutive keys, the
    keys scattered a few pixels so that some merges fail"""
    w = _Toy()
    for c, (n, per_track) in enumerate(specs):
        u = lambda i: float((i * 7) % 11) + 0.37 * ((i * 13) % 5) + 0.013 * c
        for i0 in range(0, n, per_track):
            ids = range(i0, min(i0 + per_track, n))
            w.track((float(np.mean([u(i) for i in ids])), 0.25, 1.0), [("c%d_%d" % (c, i), i % n_frames, u(i), 0.0) for i in ids])
        w.edge(*[("c%d_%d" % (c, i), "c%d_%d" % (c, i + 1)) for i in range(n - 1)])
    return build(n_frames, w.keys, w.edges, w.points, frame=3)


def _scene(seed, n_frames, n_points, frame):
    rng = np.random.default_rng(seed)
    models = np.arange(5, dtype=np.int32)
    params = np.array([[400, 320, 240, 0, 0, 0, 0, 0], [410, 405, 320, 240, 0, 0, 0, 0], [400, 320, 240, 0.05, 0, 0, 0, 0], [410, 405, 320, 240, -0.04, 0, 0, 0],
                       [420, 415, 320, 240, 0.03, -0.01, 0.001, -0.002]], np.float64)
    q, t = [], []
    for f in range(n_frames):                 # on a circle of radius 6, looking at the origin
        a = 2 * np.pi * f / n_frames
        c = np.array([6 * np.cos(a), 0.3 * np.sin(3 * a), 6 * np.sin(a)])
        zc = -c / np.linalg.norm(c)
        xc = np.cross([0, 1, 0], zc); xc /= np.linalg.norm(xc)
        R = np.stack([xc, np.cross(zc, xc), zc])
        w4 = np.sqrt(max(0.0, 1 + R[0, 0] + R[1, 1] + R[2, 2])) / 2
        if w4 > 1e-6:
            qq = [(R[2, 1] - R[1, 2]) / (4 * w4), (R[0, 2] - R[2, 0]) / (4 * w4), (R[1, 0] - R[0, 1]) / (4 * w4), w4]
        else:
            qq = [0.0, 1.0, 0.0, 0.0]
        qq = np.array(qq) / np.linalg.norm(qq)
        q.append(qq); t.append(-R @ c)
    cam_intr = (np.arange(n_frames) % 5).astype(np.int32)
    cams = dict(cam_q=np.array(q), cam_t=np.array(t), cam_intr=cam_intr, intr_model=models, intr_params=params)
    ycam = Y._cams(dict(cams, registered=np.ones(n_frames)), float)
    w = _Toy()
    per_frame = [0] * n_frames
    views = []
    for p in range(n_points):
        P = rng.uniform(-1.0, 1.0, 3)
        seen = [f for f in range(n_frames) if rng.random() < 0.3 and per_frame[f] < 200]
        names = []
        for f in seen:                         # the key point: where the error against it is zero, plus noise
            lo, hi = np.array([-2000.0, -2000.0]), np.array([2000.0, 2000.0])
            uv = np.array([320.0, 240.0])
            for _ in range(2):                 # re(uv) is the distance to the projection: walk to it
                r0 = Y.reprojection_error(ycam[f], [float(v) for v in P], float(uv[0]), float(uv[1]))[0]
                rx = Y.reprojection_error(ycam[f], [float(v) for v in P], float(uv[0]) + r0, float(uv[1]))[0]
                ry = Y.reprojection_error(ycam[f], [float(v) for v in P], float(uv[0]), float(uv[1]) + r0)[0]
                if r0 == 0:
                    break
                # the projection p satisfies |uv - p| = r0, |uv + (r0, 0) - p| = rx, |uv + (0, r0) - p| = ry
                dx, dy = (r0 * r0 + r0 * r0 - rx * rx) / (2 * r0), (r0 * r0 + r0 * r0 - ry * ry) / (2 * r0)
                uv = np.clip(uv + [dx, dy], lo, hi)
            uv = uv + rng.normal(0, 0.6, 2)
            names.append(("p%d_%d" % (p, f), f, float(uv[0]), float(uv[1])))
            per_frame[f] += 1
        # fragments: tracks of 2-4 consecutive views, some views left free
        i = 0
        while i < len(names):
            n = int(rng.integers(1, 5))
            part = names[i:i + n]
            if rng.random() < 0.25 or len(part) < 2:
                for nm in part:
                    w.free(*nm)
            else:
                w.track(tuple(P + rng.normal(0, 0.01, 3)), part)
            i += n
        for a in range(len(names)):
            for b in range(a + 1, len(names)):
                if rng.random() < 0.5:
                    w.edge((names[a][0], names[b][0]))
        views.append(names)
    flat = [v for names in views for v in names]
    for _ in range(len(flat) // 12):          # wrong correspondences
        a, b = flat[int(rng.integers(len(flat)))], flat[int(rng.integers(len(flat)))]
        if a[1] != b[1] and a[0].split("_")[0] != b[0].split("_")[0]:
            w.edge((a[0], b[0]))
    registered = [0 if f == n_frames - 1 else 1 for f in range(n_frames)]
    return build(n_frames, w.keys, w.edges, w.points, frame=frame, registered=registered, cams=cams)


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "rules":
        return _rules()
    if name == "live":
        return _live()
    if name == "sizes":
        return _chains([(63, 3), (64, 4), (65, 5), (128, 64), (129, 65)])
    if name == "limits":
        return _chains([(1024, 2), (1025, 3), (512, 1), (513, 1)])
    if name == "scene_a":
        return _scene(11, 24, 260, frame=5)
    if name == "scene_b":
        return _scene(12, 40, 420, frame=17)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def expected(name, mode):
    """(A) in float64, computed once and shared; leave it unchanged"""
    return Y.run_literal(case(name), mode, float)


@functools.lru_cache(maxsize=None)
def expected_long(name, mode):
    return Y.run_literal(case(name), mode, np.longdouble)


@functools.lru_cache(maxsize=None)
def coverage(name):
    met = set()
    for mode in Y.MODES:
        met |= expected(name, mode)["rules"]
    plan, _ = Y._plan(case(name), 3, 0)
    for keys, tracks, processed, over in plan:
        if len(keys) in (63, 64, 65, 128, 129, 1025):
            met.add("a component of %d keys" % len(keys))
        if len(keys) == 1024 and processed:
            met.add("a component of exactly 1024 keys")
        if len(tracks) == 512 and processed:
            met.add("a component of exactly 512 tracks")
        if len(tracks) == 513 and over:
            met.add("a component of 513 tracks")
    assert met <= set(Y.RULES), met - set(Y.RULES)
    return {r: r in met for r in Y.RULES}


def arrays(c):
    """the positional arguments of capi.merge_tracks"""
    return (c["key_ptr"], c["key_xy"], c["registered"], c["cam_q"], c["cam_t"], c["cam_intr"], c["intr_model"], c["intr_params"], c["corr_ptr"], c["corr_key"], c["points"],
            c["track_outlier"], c["track_of_key"])
