"""The seeded catalogue of match-expansion cases (tests/expand_yardstick.py describes a case): the smallest shapes at which each rule
of the search can go wrong, three random ring scenes for breadth, and `coverage`, the table that proves from the yardstick's own
bookkeeping that every rule is exercised by some case.  8 - 70 frames, at most 200 key points each; every case but `star` runs with
min_visible 3 or lower, `star` with the defaults throughout."""
import functools

import numpy as np

from tests import expand_yardstick as Y

W, H = 640, 480


class Scene:
    def __init__(self, n, n_keys, seed, opt=None):
        self.n = n
        self.n_keys = [n_keys] * n if isinstance(n_keys, int) else list(n_keys)
        self.rng = np.random.default_rng(seed)
        self.xy = [np.stack([self.rng.uniform(0, W - 1, k), self.rng.uniform(0, H - 1, k)], axis=1) if k else np.zeros((0, 2)) for k in self.n_keys]
        self.sizes = [(W, H)] * n
        self.pairs, self.rank, self.tried, self.init, self.opt = [], [[] for _ in range(n)], [], (0, 1), dict(opt or {})

    def pair(self, a, b, matches):
        self.pairs.append((a, b, [(int(i), int(j)) for i, j in matches]))

    def case(self):
        key_ptr = np.concatenate([[0], np.cumsum(self.n_keys)]).astype(np.int64)
        keys = np.zeros((int(key_ptr[-1]), 4), np.float32)
        keys[:, :2] = np.concatenate(self.xy)
        keys[:, 2] = 1.0
        mp = np.concatenate([[0], np.cumsum([len(m) for _, _, m in self.pairs])]).astype(np.int64)
        m = np.array([ij for _, _, ms in self.pairs for ij in ms], np.int32).reshape(-1, 2)
        return dict(n=self.n, key_ptr=key_ptr, keys=keys, sizes=np.array(self.sizes, np.int32), pair_a=np.array([p[0] for p in self.pairs], np.int32),
                    pair_b=np.array([p[1] for p in self.pairs], np.int32), match_ptr=mp, matches=m,
                    rank_ptr=np.concatenate([[0], np.cumsum([len(r) for r in self.rank])]).astype(np.int64),
                    rank_ids=np.array([i for r in self.rank for i in r], np.int32), tried=np.array(self.tried, np.int32).reshape(-1, 2), init=self.init, opt=self.opt)


def all_others(s, frames=None):
    for f in (range(s.n) if frames is None else frames):
        s.rank[f] = [g for g in range(s.n) if g != f]


def chain():
    """Three tracks through frames 0 .. 7, matched between neighbours and (0, 2): the first initial frame fires into 1 and 2, then every
    frame registers alone in its round off its predecessor, 8 last and with exactly min_visible marks; 9 ends at one less.  Keys 0 and 1 share a patch and
    key 2 has its own, so a (frame, patch) is seen twice and another once; key 2 of frame 5 lies at x == width.  Every frame ranks every
    other, so most pairs are proposed from both directions; (3, 6) is tried."""
    s = Scene(10, 4, 11, dict(min_visible=3))
    same = [(c, c) for c in range(3)]
    for a, b in [(0, 1), (0, 2), (1, 2)] + [(f, f + 1) for f in range(2, 7)]:
        s.pair(a, b, same)
    s.pair(7, 8, same)
    s.pair(9, 0, same[:2])
    for f in range(10):
        s.xy[f][0] = (100.0, 100.0); s.xy[f][1] = (110.0, 105.0); s.xy[f][2] = (400.0 + f, 300.0)
    s.xy[5][2] = (float(W), 300.0)
    all_others(s)
    s.rank[4] = [4] + s.rank[4]                              # itself in its own list
    s.tried = [(6, 3)]
    return s.case()


def tracks():
    """All four branches of AddTrack in an order that leaves every quirk behind: a key point kept out by the insert that does not
    overwrite (frame 4 key 1 points at a track that holds frame 4 with key 0: GetMatcheNum(4, x) != GetMatcheNum(x, 4)), a merge that
    moves one observation, drops three on same-frame conflicts and leaves a key point (frame 5 key 3) pointing at the invalid track,
    which then still takes an observation."""
    s = Scene(8, 8, 12, dict(min_visible=1))
    s.pair(0, 1, [(0, 0), (1, 1)])                           # two new tracks
    s.pair(1, 2, [(0, 0), (2, 1)])                           # the second key point joins track 0; a third track {1: 2, 2: 1}
    s.pair(3, 2, [(0, 0), (1, 1)])                           # the first key point joins: tracks 0 and 2
    s.pair(4, 0, [(0, 0)])
    s.pair(4, 1, [(1, 0)])                                   # frame 4 is in track 0 with key 0: key 1 points at it and is kept out
    s.pair(2, 5, [(1, 0)])                                   # track 2 gains (5, 0)
    s.pair(5, 1, [(3, 2)])                                   # (5, 3) points at track 2 and is kept out
    s.pair(4, 3, [(0, 1)])                                   # track 2 merges into track 0: (5, 0) moves, frames 1, 2, 3 conflict
    s.pair(5, 6, [(3, 0)])                                   # the invalid track takes (6, 0)
    s.pair(6, 7, [(1, 1), (2, 2)])
    s.pair(7, 0, [(2, 2), (3, 3)])
    all_others(s)
    return s.case()


def rounds():
    """The initial pair is stored as (1, 0) and asked for as (0, 1).  Frames 2 and 4 register in the same round and are paired with
    each other; key points of 2 have correspondents in two registered frames; the key points of 5 are each in the lists of a key point
    of 2 and of one of 4, so two frames mark them in one round and 5 ends at exactly min_visible.  3, 10 and 11 have no key points,
    8 and 9 are a component of their own, 6 and 7 are isolated.  Two key points of frame 1 are matched to one of frame 0, which so ends
    with two marks: an initial frame that is not among the registered."""
    s = Scene(12, [6, 6, 6, 0, 6, 6, 2, 2, 5, 5, 0, 0], 13, dict(min_visible=3))
    tri = [(c, c) for c in range(3)]
    s.pair(1, 0, [(0, 0), (1, 1), (2, 1)])
    s.pair(1, 2, tri)
    s.pair(4, 1, tri)
    s.pair(2, 4, tri + [(3, 3)])
    s.pair(2, 5, tri)
    s.pair(5, 4, tri)
    s.pair(9, 8, [(c, c) for c in range(5)])
    for f in range(12):
        for c in range(min(3, s.n_keys[f])):
            s.xy[f][c] = (200.0 + 3 * c, 200.0)
    all_others(s)
    s.init = (0, 1)
    return s.case()


def shared():
    """A hub (frame 0, initial with 1) whose key points are matched into X = 2 (60), Y = 3 (50) and Z = 4 (51): GetMatcheNum(X, Y) is
    exactly 50 and the pair is proposed, GetMatcheNum(X, Z) is 51 and it is not.  The key points of frame 1 sit two to a patch."""
    s = Scene(8, [64, 64, 64, 64, 64, 4, 4, 4], 14, dict(min_visible=3))
    s.pair(0, 1, [(k, k) for k in range(60)])
    s.pair(0, 2, [(k, k) for k in range(60)])
    s.pair(3, 0, [(k, k) for k in range(50)])
    s.pair(0, 4, [(k, k) for k in range(51)])
    for k in range(64):
        s.xy[1][k] = (10.0 + 64 * ((k // 2) % 10), 10.0 + 48 * ((k // 2) // 10))
    all_others(s)
    return s.case()


def star():
    """The default options.  Frame 0 has 30 key points matched into each of frames 1 .. 40, which so register with exactly 30 marks.
    41 .. 46 are not connected: 41 has 15 registered frames at ranks 6 .. 20, 42 has 14 there and 21 at ranks 26 .. 46 (35 in all),
    43 has 14 and 20 (34), 44 has 14 and nothing.  The fillers repeat one id, so ids are listed twice.  42's registered frames reach
    past rank 40: those at 41 and beyond are no similarity pairs.  (41, 7) is tried."""
    s = Scene(47, [30] + [30] * 40 + [1] * 6, 15)
    for f in range(1, 41):
        s.pair(0, f, [(k, k) for k in range(30)])
    fill = [45] * 5
    s.rank[41] = fill + list(range(1, 16))
    s.rank[42] = fill + list(range(1, 15)) + [46] * 6 + list(range(15, 36))
    s.rank[43] = fill + list(range(1, 15)) + [46] * 6 + list(range(15, 35))
    s.rank[44] = fill + list(range(1, 15))
    s.rank[5] = [41, 42, 6, 7, 6]
    s.tried = [(41, 7)]
    return s.case()


def ring(n, seed, keys=40, wrong=0.06):
    """n frames around a ring of points, each seen by a run of frames; pairs up to two steps apart, some stored backwards, a few wrong
    matches so that tracks merge and conflict; rank lists of the ten nearest frames with a repeat; a second component at the end."""
    s = Scene(n, keys, seed, dict(min_visible=3))
    main = n - 3
    pts = 3 * main
    span = 5
    seen_by = [[] for _ in range(n)]                         # per frame: the point of each key point
    for p in range(pts):
        start = int(s.rng.integers(0, main))
        base = (s.rng.uniform(0, W - 1), s.rng.uniform(0, H - 1))
        for d in range(span):
            f = (start + d) % main
            if len(seen_by[f]) < keys:
                s.xy[f][len(seen_by[f])] = (min(max(base[0] + s.rng.normal(0, 6), 0), W), min(max(base[1] + s.rng.normal(0, 6), 0), H))
                seen_by[f].append(p)
    for f in range(main):
        for d in (1, 2):
            g = (f + d) % main
            if g == f or any({a, b} == {f, g} for a, b, _ in s.pairs):
                continue
            a, b = (f, g) if s.rng.random() < 0.7 else (g, f)
            ms = []
            for i, p in enumerate(seen_by[a]):
                if p in seen_by[b] and s.rng.random() < 0.9:
                    j = seen_by[b].index(p)
                    if s.rng.random() < wrong:
                        j = int(s.rng.integers(0, keys))
                    ms.append((i, j))
            if ms:
                s.pair(a, b, ms)
    s.pair(n - 2, n - 1, [(k, k) for k in range(5)])
    for f in range(n):
        near = [(f + d) % main for d in (1, -1, 2, -2, 3, -3, 4, -4, 5, -5)]
        s.rank[f] = [int(x) for x in s.rng.permutation(near)] + [near[0], n - 1]
    first = s.pairs[0]
    s.init = (first[1], first[0])
    s.tried = [(s.rank[0][0], 0)]
    return s.case()


CASES = dict(chain=chain, tracks=tracks, rounds=rounds, shared=shared, star=star, ring12=lambda: ring(12, 21), ring33=lambda: ring(33, 22, 24),
             ring65=lambda: ring(65, 23, 16))
NAMES = tuple(CASES)


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def expected(name):
    """the yardstick's result, computed once and shared; nobody writes into it"""
    return Y.literal(case(name))


def coverage(name):
    """rule -> whether this case exercises it, from the yardstick's bookkeeping"""
    c, r = case(name), expected(name)
    o, seen = Y.options(c), r["seen"]
    n = c["n"]
    paired = {(int(a), int(b)) for a, b in zip(c["pair_a"], c["pair_b"])}
    paired |= {(b, a) for a, b in paired}
    stored = [(int(a), int(b)) for a, b in zip(c["pair_a"], c["pair_b"]) if {int(a), int(b)} == set(c["init"])][0]
    reg = r["registered"]
    kp = c["key_ptr"]
    shared = {(a, b): sh for a, b, sh, _ in r["cand"]}
    rank_of = lambda f: c["rank_ids"][c["rank_ptr"][f]:c["rank_ptr"][f + 1]].tolist()
    sim = [(a, b) for a, b, src in r["pairs"] if src == 2]
    passing = {(a, b) for a, b, sh, cv in r["cand"] if sh <= o["max_shared_matches"] and cv >= o["min_covisible_patches"]}

    def best_rank(a, b):
        out = []
        for x, y in ((a, b), (b, a)):
            lst = rank_of(x)
            if y in lst:
                out.append(len(lst) - lst[::-1].index(y))
        return min(out) if out else 0

    ranks_sim = {best_rank(a, b) for a, b in sim}
    not_sim = {best_rank(a, b) for a in range(n) if r["may_register"][a] for b in range(n) if reg[b] and (min(a, b), max(a, b)) not in {(x, y) for x, y in sim}}
    bands = seen["band_counts"].values()
    return {
        "one frame per round, three rounds or more": len(seen["round_frames"]) >= 3 and all(len(x) == 1 for x in seen["round_frames"]),
        "a frame ends at exactly min_visible": any(v == o["min_visible"] for f, v in enumerate(r["visible"]) if f not in stored),
        "a frame ends one below min_visible": any(v == o["min_visible"] - 1 for v in r["visible"]),
        "an initial frame ends below min_visible": any(r["visible"][f] < o["min_visible"] for f in stored),
        "two frames of one round are paired": any((a, b) in paired for x in seen["round_frames"] for a in x for b in x),
        "the initial pair is stored backwards": stored[0] > stored[1] and tuple(c["init"]) != stored,
        "a key point with correspondents in two registered frames": any(sum(1 for h in lst if reg[h]) >= 2 for f in seen["corr_frames"] for lst in f),
        "a second component": any(not r["connected"][a] for a, _ in paired),
        "a frame without key points": any(kp[f + 1] == kp[f] for f in range(n)),
        "AddTrack: a new track": seen["new"] > 0,
        "AddTrack: the first key point joins": seen["first_joins"] > 0,
        "AddTrack: the second key point joins": seen["second_joins"] > 0,
        "AddTrack: a merge": seen["merges"] > 0,
        "AddTrack: a same-frame conflict in a merge": seen["conflicts"] > 0,
        "AddTrack: insert does not overwrite": seen["kept_out"] > 0,
        "a key point points at an invalid track": any(t >= 0 and r["tracks"][t][1] for t in r["key_track"]),
        "GetMatcheNum differs by direction": any(shared.get((b, a), sh) != sh for (a, b), sh in shared.items()),
        "exactly max_shared_matches shared": any(sh == o["max_shared_matches"] for sh in shared.values()),
        "one above max_shared_matches shared": any(sh == o["max_shared_matches"] + 1 for sh in shared.values()),
        "a (frame, patch) seen once": 1 in seen["patch_counts"],
        "a (frame, patch) seen twice": 2 in seen["patch_counts"],
        "a third frame skipped because it is paired": seen["skipped_paired"] > 0,
        "a key point at x == width": any(float(c["keys"][k][0]) == float(c["sizes"][f][0]) for f in range(n) for k in range(kp[f], kp[f + 1])),
        "a frame index of 32 or more": n >= 33,
        "a frame index of 64 or more": n >= 65,
        "an id twice in a rank list": any(len(set(rank_of(f))) < len(rank_of(f)) for f in range(n)),
        "a frame in its own rank list": any(f in rank_of(f) for f in range(n)),
        "may register at exactly mayreg_count_mid": any(c2 == o["mayreg_count_mid"] for c2, _ in bands),
        "may register at one below mid and exactly the sum": any(c2 == o["mayreg_count_mid"] - 1 and c2 + c3 == o["mayreg_count_sum"] for c2, c3 in bands),
        "does not register at one below mid and one below the sum": any(c2 == o["mayreg_count_mid"] - 1 and c2 + c3 == o["mayreg_count_sum"] - 1 for c2, c3 in bands),
        "a similarity pair at exactly similarity_rank_max": o["similarity_rank_max"] in ranks_sim,
        "no similarity pair one rank beyond": o["similarity_rank_max"] + 1 in not_sim,
        "a pair proposed from both directions": any((b, a) in passing for a, b in passing),
        "a tried pair among the ranked": any(int(b) in rank_of(int(a)) or int(a) in rank_of(int(b)) for a, b in c["tried"]),
        "a covisibility pair": any(src == 1 for _, _, src in r["pairs"]),
        "a similarity pair": any(src == 2 for _, _, src in r["pairs"]),
    }


# ---------------------------------------------------------------- the scene of the ExpansionAndMatching test
LOOP_FRAMES = 6
LOOP_INIT_PAIRS = np.array([(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (0, 2)], np.int32)
LOOP_OPT = dict(min_visible=20)


@functools.lru_cache(maxsize=None)
def loop_scene():
    """Six views of one point cloud in the style of tests/frames_cases.py: 30 points in a narrow region seen by every frame (so the
    frames two apart share 30 tracks, below max_shared_matches, and see two of them in one patch of a third frame), 25 points per pair
    of neighbours seen by those two alone, 10 unrelated key points per frame.  -> (key_ptr, keys [N][4] float32, desc [N][128],
    sizes [6][2], rank_ptr, rank_ids)"""
    from tests import fund_yardstick as YF
    from tests import match_yardstick as YM
    rng = np.random.default_rng(606)
    common = np.stack([rng.uniform(-0.8, 0.8, 30), rng.uniform(-0.4, 0.4, 30), rng.uniform(6, 7, 30)], 1)
    groups = [(common, range(LOOP_FRAMES))]
    for f in range(LOOP_FRAMES - 1):
        groups.append((np.stack([rng.uniform(-1.5, 1.5, 25), rng.uniform(-1.2, 1.2, 25), rng.uniform(5, 9, 25)], 1), (f, f + 1)))
    X = np.concatenate([g for g, _ in groups])
    base = YM.sift_like(rng, len(X))
    sees = np.zeros((LOOP_FRAMES, len(X)), bool)
    at = 0
    for g, frames in groups:
        sees[list(frames), at:at + len(g)] = True
        at += len(g)
    ks, ds, ptr = [], [], [0]
    for f in range(LOOP_FRAMES):
        R, t = YF._rot([0.1, 1.0, 0.05], -0.02 * f), np.array([-0.25 * f, 0.02 * f, 0.03 * f])
        Yc = X[sees[f]] @ R.T + t
        uv = ((Yc / Yc[:, 2:]) @ YF.K.T)[:, :2]
        assert uv.min() > 1 and (uv[:, 0] < YF.WIDTH - 1).all() and (uv[:, 1] < YF.HEIGHT - 1).all()
        uv = np.concatenate([uv, np.stack([rng.uniform(0, YF.WIDTH - 1, 10), rng.uniform(0, YF.HEIGHT - 1, 10)], 1)])
        d = np.concatenate([YM.perturb(rng, base[sees[f]]), YM.sift_like(rng, 10)])
        perm = rng.permutation(len(d))
        ks.append(np.concatenate([uv[perm], np.ones((len(d), 2))], 1).astype(np.float32)); ds.append(d[perm]); ptr.append(ptr[-1] + len(d))
    sizes = np.array([(int(YF.WIDTH), int(YF.HEIGHT))] * LOOP_FRAMES, np.int32)
    rank = [[g for g in range(LOOP_FRAMES) if g != f] for f in range(LOOP_FRAMES)]
    return (np.array(ptr, np.int64), np.ascontiguousarray(np.concatenate(ks), np.float32), np.ascontiguousarray(np.concatenate(ds)), sizes,
            np.arange(0, 5 * LOOP_FRAMES + 1, 5).astype(np.int64), np.array([g for r in rank for g in r], np.int32))
