"""The catalogue of frame triangulation: constructed maps on which every rule of tests/trif_yardstick.py is exercised, and
the table that shows it (coverage()).

  rules     12 frames, at most 40 key points each: every key_status value, unregistered neighbours, a candidate that holds the frame, a
            tie, accepted and rejected by the threshold, a key point whose only track is ineligible, a created track with an outlier
            observation, a coupled pair, a later frame extending a track an earlier one created, a zero ray1, a list of 129 observations
  sizes     lists of 128 and 129 observations (a frame per observation)
  chain_L   claim chains of length 3, 64, 65 and 200: key point i prefers the track key point i - 1 is pushed onto
  wide      a frame whose slots exceed one workgroup's threads: creates and extends alternating, then a chain across the boundary
  scene_a/b two seeded scenes (at most 40 frames x 200 key points), one-to-one matches, a part of the points already tracked

Every case runs in two modes: "frame" (the case's frame alone) and "map" (every registered frame ascending)."""
import functools

import numpy as np

from tests import trif_yardstick as Y

NAMES = ("rules", "sizes", "chain_3", "chain_64", "chain_65", "chain_200", "wide", "scene_a", "scene_b")
MODES = ("frame", "map")
RULES = tuple("status_" + s for s in Y.STATUS) + ("unregistered_skipped", "holds_frame", "tie", "accepted", "rejected", "all_ineligible", "outliers_left",
                                                  "coupled_sees_new_track", "later_frame_extends_created", "zero_ray", "multi_track", "list_128", "list_129",
                                                  "rounds_3", "rounds_64", "rounds_65", "rounds_200", "wide_step")
NOISE = 1e-3


class Builder:
    """frames with identity rotation at given centres; key points by handle (frame, index); symmetric links; tracks"""

    def __init__(self, centres, registered=None, seed=1):
        self.c = np.asarray(centres, np.float64).reshape(-1, 3)
        n = len(self.c)
        self.reg = np.ones(n, np.uint8) if registered is None else np.asarray(registered, np.uint8)
        self.keys = [[] for _ in range(n)]           # per frame: [xy, links (handles), track]
        self.points, self.rng = [], np.random.default_rng(seed)

    def project(self, f, X, noise=NOISE):
        d = np.asarray(X, np.float64) - self.c[f]
        return d[:2] / d[2] + self.rng.normal(0, noise, 2)

    def key(self, f, xy=None, X=None, noise=NOISE):
        self.keys[f].append([np.asarray(xy, np.float64) if xy is not None else self.project(f, X, noise), [], -1])
        return (f, len(self.keys[f]) - 1)

    def link(self, a, b):
        self.keys[a[0]][a[1]][1].append(b)
        self.keys[b[0]][b[1]][1].append(a)

    def clique(self, hs):
        for i, a in enumerate(hs):
            for b in hs[i + 1:]:
                self.link(a, b)

    def track(self, X, hs):
        self.points.append(np.asarray(X, np.float64))
        for f, i in hs:
            self.keys[f][i][2] = len(self.points) - 1
        return len(self.points) - 1

    def done(self, frame, **extra):
        n = len(self.c)
        key_ptr = np.concatenate([[0], np.cumsum([len(k) for k in self.keys])]).astype(np.int64)
        g = lambda h: int(key_ptr[h[0]] + h[1])
        flat = [k for ks in self.keys for k in ks]
        corr_ptr = np.concatenate([[0], np.cumsum([len(k[1]) for k in flat])]).astype(np.int64)
        q = np.zeros((n, 4)); q[:, 3] = 1.0
        return dict(key_ptr=key_ptr, key_xyn=np.array([k[0] for k in flat], np.float64).reshape(-1, 2), registered=self.reg.copy(), cam_q=q, cam_t=-self.c.copy(),
                    corr_ptr=corr_ptr, corr_key=np.array([g(h) for k in flat for h in k[1]], np.int32), points=np.array(self.points, np.float64).reshape(-1, 3),
                    track_outlier=np.zeros(len(self.points), np.uint8), track_of_key=np.array([k[2] for k in flat], np.int32), frame=frame,
                    index={name: g(h) for name, h in extra.items()})


def _rules():
    F = 5
    b = Builder([(0.5 * i, 0.02 * (i % 3), 0.0) for i in range(12)], registered=[1, 1, 1, 0] + [1] * 8, seed=11)
    ix = {}
    # created, with a neighbour in the unregistered frame 3
    Xa = (1.0, 0.3, 6.0)
    hs = [b.key(f, X=Xa) for f in (0, 1, 2, 3, F)]
    b.clique(hs); ix["create"] = hs[-1]
    # created with an outlier observation (a wrong match in frame 4) that stays without a track
    Xb = (1.5, -0.4, 7.0)
    hs = [b.key(f, X=Xb) for f in (0, 1, 2, F)]
    wrong = b.key(4, xy=(0.45, 0.4))
    b.clique(hs + [wrong]); ix["create_outlier"], ix["wrong"] = hs[-1], wrong
    # fewer than two observations: no entry; an entry in the unregistered frame only
    ix["lonely"] = b.key(F, xy=(0.1, 0.1))
    ix["unreg_only"] = b.key(F, xy=(0.2, 0.1))
    b.link(ix["unreg_only"], b.key(3, xy=(0.2, 0.1)))
    # no model: two rays that diverge
    ix["no_model"] = b.key(F, xy=(0.3, 0.0))
    b.link(ix["no_model"], b.key(1, xy=(-0.3, 0.0)))
    # extended: a track seen in frames 0, 1, 2
    X0 = (2.0, 0.5, 5.0)
    hs = [b.key(f, X=X0) for f in (0, 1, 2)]
    b.track(X0, hs)
    ix["extend"] = b.key(F, X=X0)
    for h in hs:
        b.link(ix["extend"], h)
    # rejected by the threshold: the key point lies 15 degrees off the track's ray
    X1 = (3.0, -0.5, 6.0)
    hs = [b.key(f, X=X1) for f in (0, 1)]
    b.track(X1, hs)
    off = np.array(X1) + np.array([0.0, 1.6, 0.0])
    ix["reject"] = b.key(F, X=off)
    b.link(ix["reject"], hs[0])
    # a candidate that already holds the frame: T2 is the better one but holds frame F through `holder`, so T3 is taken
    X2, X3 = (2.2, 0.1, 8.0), (2.25, 0.1, 8.0)
    h2 = [b.key(f, X=X2) for f in (0, 1)]
    ix["holder"] = b.key(F, X=X2)
    b.track(X2, h2 + [ix["holder"]])
    h3 = [b.key(f, X=X3) for f in (1, 2)]
    b.track(X3, h3)
    ix["second_choice"] = b.key(F, X=X2)
    b.link(ix["second_choice"], h2[0]); b.link(ix["second_choice"], h3[0])
    # every track ineligible: the only track seen holds the frame; nothing is created
    ix["ineligible"] = b.key(F, X=X2)
    b.link(ix["ineligible"], h2[1])
    # a tie: two tracks with the same point, the larger id first in the list
    X4 = (2.8, 0.6, 7.0)
    h4 = [b.key(0, X=X4)]; b.track(X4, h4)
    h5 = [b.key(1, X=X4)]; b.track(X4, h5)
    ix["tie"] = b.key(F, X=X4)
    b.link(ix["tie"], h5[0]); b.link(ix["tie"], h4[0])
    # several tracks, the best is taken
    X7, X8 = (1.2, -0.6, 6.0), (1.5, -0.6, 6.0)
    h7 = [b.key(0, X=X7)]; b.track(X7, h7)
    h8 = [b.key(2, X=X8)]; b.track(X8, h8)
    ix["multi"] = b.key(F, X=(1.42, -0.6, 6.0))
    b.link(ix["multi"], h7[0]); b.link(ix["multi"], h8[0])
    # a zero ray1: the track's point is the centre of frame F
    h6 = [b.key(0, xy=(0.4, 0.0))]; b.track(b.c[F].copy(), h6)
    ix["zero_ray"] = b.key(F, xy=(0.05, -0.05))
    b.link(ix["zero_ray"], h6[0])
    # a coupled pair: both lists hold `shared`, which has no track; the second must see the track the first creates
    Xc = (3.2, 0.2, 6.5)
    shared = b.key(0, X=Xc)
    ix["couple_1"] = b.key(F, X=Xc)
    for h in (shared, b.key(1, X=Xc), b.key(2, X=Xc)):
        b.link(ix["couple_1"], h)
    ix["couple_2"] = b.key(F, X=Xc)
    b.link(ix["couple_2"], shared); b.link(ix["couple_2"], b.key(4, X=Xc))
    # a later frame extends what an earlier frame of the list created: k6 is linked to k2 only
    Xd = (0.6, 0.7, 5.5)
    k0, k1, k2, k6 = (b.key(f, X=Xd) for f in (0, 1, 2, 6))
    b.clique([k0, k1, k2]); b.link(k6, k2); ix["later"] = k6
    # 129 observations: thirteen key points in each of ten registered frames see the key point (one-to-many matches)
    Xl = (2.6, -0.2, 9.0)
    ix["long"] = b.key(F, X=Xl)
    others = [f for f in range(12) if f not in (3, F)]
    for j in range(128):
        b.link(ix["long"], b.key(others[j % 10], X=Xl))
    return b.done(F, **ix)


def _sizes():
    """frame 130 holds two key points: one with 128 observations (created), one with 129 (status 3)"""
    n = 131
    b = Builder([(0.05 * i, 0.01 * (i % 5), 0.0) for i in range(n)], seed=21)
    X, Z = (3.0, 0.2, 8.0), (3.5, -0.3, 9.0)
    p128, p129 = b.key(n - 1, X=X), b.key(n - 1, X=Z)
    for f in range(127):
        b.link(p128, b.key(f, X=X))
    for f in range(128):
        b.link(p129, b.key(f, X=Z))
    return b.done(n - 1, p128=p128, p129=p129)


def _chain(b, F, L, x0=0.0, y=0.0):
    """tracks t_0 .. t_L-1 along x, each seen in frame 0; key point i of frame F lies between t_i-1 and t_i, nearer t_i-1"""
    X = [np.array([x0 + 0.06 * j, y, 5.0]) for j in range(L)]
    hk = []
    for j in range(L):
        h = b.key(0, X=X[j])
        b.track(X[j], [h])
        hk.append(h)
    out = []
    for i in range(L):
        p = b.key(F, X=X[0] if i == 0 else X[i - 1] + 0.3 * (X[i] - X[i - 1]), noise=5e-4)
        if i > 0:
            b.link(p, hk[i - 1])
        b.link(p, hk[i])
        out.append(p)
    return out


def _chain_case(L):
    b = Builder([(0.0, 0.0, 0.0), (0.4, 0.0, 0.0), (0.8, 0.1, 0.0)], seed=30 + L)
    ps = _chain(b, 2, L, x0=-0.03 * L)
    return b.done(2, first=ps[0], last=ps[-1])


def _wide():
    b = Builder([(0.0, 0.0, 0.0), (0.4, 0.0, 0.0), (0.8, 0.1, 0.0), (1.2, 0.0, 0.0)], seed=41)
    F = 3
    for i in range(280):
        X = np.array([-1.5 + 0.011 * i, 0.5 + 0.1 * (i % 7), 6.0 + 0.05 * (i % 11)])
        if i % 2:
            hs = [b.key(f, X=X) for f in (0, 1)]
            b.track(X, hs)
            p = b.key(F, X=X)
            b.link(p, hs[i % 4 // 2])
        else:
            b.clique([b.key(f, X=X) for f in (0, 1, 2, F)])
    ps = _chain(b, F, 40, x0=-0.6, y=-0.8)
    return b.done(F, first=ps[0], last=ps[-1])


def _scene(seed, n_frames, n_points, n_new):
    """cameras on a line looking down +z; every frame sees a random part of the points; one-to-one matches between frames at most three
    apart, a few of them wrong; the points seen by enough of the first frames are tracked there; the last n_new frames carry no track;
    one frame in the middle is unregistered"""
    rng = np.random.default_rng(seed)
    b = Builder([(0.3 * i, 0.05 * np.sin(i), 0.0) for i in range(n_frames)], registered=[0 if i == n_frames // 2 else 1 for i in range(n_frames)], seed=seed + 1)
    P = np.stack([rng.uniform(-1, 0.3 * n_frames + 1, n_points), rng.uniform(-1.5, 1.5, n_points), rng.uniform(5, 9, n_points)], 1)
    seen = [dict() for _ in range(n_frames)]                # per frame: point -> handle
    for f in range(n_frames):
        near = np.nonzero(np.abs(P[:, 0] - 0.3 * f) < 2.5)[0]
        for j in rng.permutation(near)[:min(len(near), 190)]:
            if rng.random() < 0.6:
                seen[f][int(j)] = b.key(f, X=P[j])
    for f in range(n_frames):
        for g in range(f + 1, min(f + 4, n_frames)):
            common = [j for j in seen[f] if j in seen[g]]
            used = set()
            for j in common:
                if rng.random() < 0.85:
                    tgt = j
                    if rng.random() < 0.05:                  # a wrong match
                        tgt = common[int(rng.integers(len(common)))]
                    if tgt in used:
                        continue
                    used.add(tgt)
                    b.link(seen[f][j], seen[g][tgt])
    old = n_frames - n_new
    for j in range(n_points):
        hs = [seen[f][j] for f in range(old) if j in seen[f] and b.reg[f]]
        if len(hs) >= 2 and rng.random() < 0.6:
            b.track(P[j] + rng.normal(0, 2e-3, 3), [h for h in hs if rng.random() < 0.8])
    return b.done(old)


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "rules":
        return _rules()
    if name == "sizes":
        return _sizes()
    if name.startswith("chain_"):
        return _chain_case(int(name[6:]))
    if name == "wide":
        return _wide()
    if name == "scene_a":
        return _scene(101, 14, 260, 3)
    if name == "scene_b":
        return _scene(202, 36, 420, 2)
    raise KeyError(name)


def frames_of(c, mode):
    return [int(c["frame"])] if mode == "frame" else [f for f in range(len(c["registered"])) if c["registered"][f]]


def arrays(c, mode):
    """the arguments of capi.triangulate_frames"""
    return (c["key_ptr"], c["key_xyn"], c["registered"], c["cam_q"], c["cam_t"], c["corr_ptr"], c["corr_key"], frames_of(c, mode), c["points"], c["track_outlier"],
            c["track_of_key"])


@functools.lru_cache(maxsize=None)
def expected(name, mode):
    """(B) with the CPU create"""
    c = case(name)
    return Y.run_flat(c, frames_of(c, mode), Y.cpu_create_for(c))


@functools.lru_cache(maxsize=None)
def literal(name, mode, dtype="float64"):
    c = case(name)
    return Y.run_literal(c, frames_of(c, mode), Y.cpu_create_for(c), np.dtype(dtype))


def coverage(name):
    """rule -> whether the case exercises it in one of its modes"""
    c = case(name)
    hit = dict.fromkeys(RULES, False)
    for mode in MODES:
        r = expected(name, mode)
        for s, word in enumerate(Y.STATUS):
            if s == 0:
                hit["status_not_visited"] |= "not_visited" in r["events"]
            else:
                hit["status_" + word] |= bool((r["key_status"] == s).any())
        for e in r["events"]:
            if e in hit:
                hit[e] = True
    return hit
