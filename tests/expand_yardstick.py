"""The yardstick of match expansion: MatchExpansionSolver::Run of the reference restated in pure Python on integers,
twice and independently.

`literal` keeps the reference's containers: dict for std::map (insert that does not overwrite, iteration in ascending key order),
set for std::set, the sequential loops of SimulationSfM and of GetCandidateCovisibility with its growing matched_ids.  `arrays` works
on sorted numpy arrays in synchronous, order-free steps, the way the kernels do.  The two must agree exactly on every field; the
library is compared with `literal`.

A case is a dict: n, key_ptr [n+1], keys [N][4] float32, sizes [n][2] (width, height), pair_a, pair_b, match_ptr, matches [M][2],
rank_ptr, rank_ids, tried [k][2], init (a, b), opt (overrides of DEFAULTS).  A result is a dict of plain lists / arrays:
key_track, tracks [(obs [(frame, key)], invalid)], connected, visible, rounds, registered, codes (per frame, ascending), cand
[(id1, id2, shared, covis)], may_register, pairs [(a, b, source)]."""
import bisect

import numpy as np

DEFAULTS = dict(patch_cols=10, patch_rows=10, min_patch_obs=2, min_visible=30, max_shared_matches=50, min_covisible_patches=1, similarity_rank_max=40,
                mayreg_rank_lo=5, mayreg_rank_mid=25, mayreg_rank_hi=50, mayreg_count_mid=15, mayreg_count_sum=35)


def options(case):
    o = dict(DEFAULTS)
    o.update(case.get("opt", {}))
    return o


def c_div(a, b):
    """C integer division: toward zero"""
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b >= 0) else -q


def patch_of(x, y, width, height, o):
    """PatchInit; (int) of a float truncates toward zero"""
    step_x, step_y = width // o["patch_cols"], height // o["patch_rows"]
    px, py = c_div(int(x), step_x), c_div(int(y), step_y)
    assert px >= 0 and py >= 0
    return min(py, o["patch_rows"] - 1) * o["patch_cols"] + min(px, o["patch_cols"] - 1)


def patches_of(case, o):
    kp = case["key_ptr"]
    return [[patch_of(float(case["keys"][k][0]), float(case["keys"][k][1]), int(case["sizes"][f][0]), int(case["sizes"][f][1]), o) for k in range(kp[f], kp[f + 1])]
            for f in range(case["n"])]


def pair_matches(case):
    mp = case["match_ptr"]
    for p, (a, b) in enumerate(zip(case["pair_a"], case["pair_b"])):
        yield int(a), int(b), [(int(i), int(j)) for i, j in case["matches"][mp[p]:mp[p + 1]]]


# ---------------------------------------------------------------- literal
def literal_tracks(case):
    kp = case["key_ptr"]
    ids = [[-1] * int(kp[f + 1] - kp[f]) for f in range(case["n"])]
    tracks = []                                          # [obs dict frame -> key, invalid]
    seen = dict(new=0, first_joins=0, second_joins=0, merges=0, conflicts=0, kept_out=0)          # what the catalogue's table reads

    def insert(t, fr, ky):
        seen["kept_out"] += 1 if fr in tracks[t][0] else 0          # std::map::insert on a key that is there
        tracks[t][0].setdefault(fr, ky)

    for f1, f2, matches in pair_matches(case):
        for i1, i2 in matches:
            if ids[f1][i1] == -1 and ids[f2][i2] == -1:
                ids[f1][i1] = ids[f2][i2] = len(tracks)
                tracks.append([{}, False])
                insert(len(tracks) - 1, f1, i1); insert(len(tracks) - 1, f2, i2)
                seen["new"] += 1
            elif ids[f1][i1] == -1:
                t = ids[f1][i1] = ids[f2][i2]
                insert(t, f1, i1)
                seen["first_joins"] += 1
            elif ids[f2][i2] == -1:
                t = ids[f2][i2] = ids[f1][i1]
                insert(t, f2, i2)
                seen["second_joins"] += 1
            elif ids[f1][i1] != ids[f2][i2]:
                t1, t2 = ids[f1][i1], ids[f2][i2]
                o1, o2 = tracks[t1][0], tracks[t2][0]
                for fr in sorted(o2):
                    ky = o2[fr]
                    if fr not in o1:
                        o1[fr] = ky
                        ids[fr][ky] = t1
                    elif o1[fr] == ky:
                        ids[fr][ky] = t1
                    else:
                        ids[fr][ky] = -1
                        seen["conflicts"] += 1
                tracks[t2][1] = True
                seen["merges"] += 1
    return ids, tracks, seen


def literal(case):
    o = options(case)
    n, kp = case["n"], case["key_ptr"]
    # MakeIdPair, MakeCorrGraph
    id_pair = [dict() for _ in range(n)]
    corrs = [[[] for _ in range(kp[f + 1] - kp[f])] for f in range(n)]
    pairs = []
    for p, (a, b, matches) in enumerate(pair_matches(case)):
        id_pair[a][b] = p; id_pair[b][a] = p
        pairs.append((a, b))
        for i, j in matches:
            corrs[a][i].append((b, j)); corrs[b][j].append((a, i))
    init = id_pair[case["init"][0]][case["init"][1]]
    f0, g0 = pairs[init]
    # GetConnectedFrames
    connected = [False] * n
    connected[f0] = connected[g0] = True
    cand = {f0, g0}
    while cand:
        new = set()
        for f in sorted(cand):
            for g in sorted(id_pair[f]):
                if not connected[g]:
                    new.add(g); connected[g] = True
        cand = new
    # SimulationSfM, tri_points
    tri = [[False] * len(c) for c in corrs]
    visible = [0] * n
    registered = [False] * n

    def tri_points(f, g):
        for lst in corrs[f]:
            if any(h == g for h, _ in lst):
                for h, m in lst:
                    if not tri[h][m]:
                        tri[h][m] = True
                        visible[h] += 1

    registered[f0] = registered[g0] = True
    tri_points(f0, g0)
    rounds = 0
    round_frames = []
    while True:
        nxt = []
        for f in range(n):
            if not registered[f] and visible[f] >= o["min_visible"]:
                nxt.append(f); registered[f] = True
        if not nxt:
            break
        rounds += 1
        round_frames.append(nxt)
        for f in nxt:
            for g in sorted(id_pair[f]):
                if registered[g]:
                    tri_points(f, g)
    assert visible == [sum(t) for t in tri]
    reg = [v != 0 and v >= o["min_visible"] for v in visible]
    # MakeTrack, PatchInit, GetCovisibilityInfo
    ids, tracks, seen = literal_tracks(case)
    seen.update(round_frames=round_frames, skipped_paired=0, band_counts={})
    patch = patches_of(case, o)
    npatch = o["patch_cols"] * o["patch_rows"]
    valid = lambda t: t != -1 and not tracks[t][1]
    info = [dict() for _ in range(n)]
    for i in range(n):
        if not connected[i]:
            continue
        for t in ids[i]:
            if not valid(t):
                continue
            for fr in sorted(tracks[t][0]):
                if fr == i or fr in id_pair[i]:
                    seen["skipped_paired"] += 1 if fr != i else 0
                    continue
                info[i].setdefault(fr, [0] * npatch)[patch[fr][tracks[t][0][fr]]] += 1
    codes = [[fr * npatch + q for fr in sorted(info[i]) for q in range(npatch) if info[i][fr][q] >= o["min_patch_obs"]] for i in range(n)]

    def match_num(a, b):
        return sum(1 for t in ids[a] if valid(t) and b in tracks[t][0])

    def covisible(a, b):
        return sum(1 for fr in sorted(info[a]) if fr in info[b] for q in range(npatch)
                   if info[a][fr][q] >= o["min_patch_obs"] and info[b][fr][q] >= o["min_patch_obs"])

    # GetId2RankVec
    rp, ri = case["rank_ptr"], case["rank_ids"]
    rank = [dict() for _ in range(n)]
    for f in range(n):
        for k in range(rp[f], rp[f + 1]):
            rank[f][int(ri[k])] = int(k - rp[f]) + 1
    matched = [set() for _ in range(n)]
    for a, b in case["tried"]:
        matched[int(a)].add(int(b)); matched[int(b)].add(int(a))
    tried0 = [set(s) for s in matched]
    # GetCandidateCovisibility, with matched_ids growing as it goes
    frame_pairs = []
    rows = []
    for a in range(n):
        for b in sorted(rank[a]):
            if a != b and b not in tried0[a] and (reg[a] or reg[b]) and connected[a] and connected[b]:
                rows.append((a, b, match_num(a, b), covisible(a, b)))          # the interface's cand: against the tried pairs as given
            if a == b or b in matched[a]:
                continue
            if not reg[a] and not reg[b]:
                continue
            if not connected[a] or not connected[b]:
                continue
            if match_num(a, b) > o["max_shared_matches"]:
                continue
            if covisible(a, b) >= o["min_covisible_patches"]:
                frame_pairs.append((a, b, 1))
                matched[a].add(b); matched[b].add(a)
    # GetMayreg, GetCandidateSimilarity
    may = [False] * n
    for f in range(n):
        if connected[f]:
            continue
        c2 = c3 = 0
        for g in sorted(rank[f]):
            if reg[g]:
                r = rank[f][g]
                if r <= o["mayreg_rank_lo"]:
                    pass
                elif r <= o["mayreg_rank_mid"]:
                    c2 += 1
                elif r <= o["mayreg_rank_hi"]:
                    c3 += 1
        may[f] = c2 >= o["mayreg_count_mid"] or c2 + c3 >= o["mayreg_count_sum"]
        seen["band_counts"][f] = (c2, c3)
    for a in [f for f in range(n) if may[f]]:
        for b in [f for f in range(n) if reg[f]]:
            if b in matched[a]:
                continue
            if (b in rank[a] and rank[a][b] <= o["similarity_rank_max"]) or (a in rank[b] and rank[b][a] <= o["similarity_rank_max"]):
                frame_pairs.append((a, b, 2))
                matched[a].add(b); matched[b].add(a)
    # remove duplicate frame pairs
    lists = [dict() for _ in range(n)]
    for a, b, src in frame_pairs:
        lists[min(a, b)].setdefault(max(a, b), src)
    out = [(a, b, lists[a][b]) for a in range(n) for b in sorted(lists[a])]
    return dict(key_track=[t for f in ids for t in f], tracks=[(sorted(t[0].items()), t[1]) for t in tracks], connected=connected, visible=visible, rounds=rounds,
                registered=reg, codes=codes, cand=rows, may_register=may, pairs=out,
                seen=dict(seen, patch_counts=sorted({c for d in info for v in d.values() for c in v if c}), emitted=[(a, b) for a, b, _ in frame_pairs],
                          corr_frames=[[sorted({h for h, _ in lst}) for lst in c] for c in corrs]))


# ---------------------------------------------------------------- arrays
def array_tracks(case):
    """AddTrack on sorted lists of frame * 2^32 + key"""
    kp = case["key_ptr"]
    key_track = [-1] * int(kp[-1])
    obs, invalid = [], []
    SH = 1 << 32

    def held(t, fr):
        k = bisect.bisect_left(obs[t], fr * SH)
        return obs[t][k] % SH if k < len(obs[t]) and obs[t][k] // SH == fr else -1

    def put(t, fr, ky):
        if held(t, fr) < 0:
            bisect.insort(obs[t], fr * SH + ky)

    for f1, f2, matches in pair_matches(case):
        for i1, i2 in matches:
            k1, k2 = int(kp[f1]) + i1, int(kp[f2]) + i2
            t1, t2 = key_track[k1], key_track[k2]
            if t1 < 0 and t2 < 0:
                key_track[k1] = key_track[k2] = len(obs)
                obs.append([]); invalid.append(False)
                put(len(obs) - 1, f1, i1); put(len(obs) - 1, f2, i2)
            elif t1 < 0:
                key_track[k1] = t2
                put(t2, f1, i1)
            elif t2 < 0:
                key_track[k2] = t1
                put(t1, f2, i2)
            elif t1 != t2:
                for code in list(obs[t2]):
                    fr, ky = code // SH, code % SH
                    h = held(t1, fr)
                    if h < 0:
                        put(t1, fr, ky)
                    key_track[int(kp[fr]) + ky] = t1 if h < 0 or h == ky else -1
                invalid[t2] = True
    return key_track, [[(c // SH, c % SH) for c in t] for t in obs], invalid


def arrays(case):
    o = options(case)
    n = case["n"]
    kp = np.asarray(case["key_ptr"], np.int64)
    N = int(kp[-1])
    frame_of = np.repeat(np.arange(n), np.diff(kp))
    pa, pb = np.asarray(case["pair_a"], np.int64), np.asarray(case["pair_b"], np.int64)
    mp = np.asarray(case["match_ptr"], np.int64)
    m = np.asarray(case["matches"], np.int64).reshape(-1, 2)
    pair_of = np.repeat(np.arange(len(pa)), np.diff(mp))
    ka, kb = kp[pa[pair_of]] + m[:, 0], kp[pb[pair_of]] + m[:, 1]
    # correspondence lists as sorted (owner, entry) rows
    own, ent = np.concatenate([ka, kb]), np.concatenate([kb, ka])
    order = np.argsort(own, kind="stable")
    own, ent = own[order], ent[order]
    paired = np.zeros((n, n), bool)
    paired[pa, pb] = True; paired[pb, pa] = True
    hit = np.flatnonzero(((pa == case["init"][0]) & (pb == case["init"][1])) | ((pa == case["init"][1]) & (pb == case["init"][0])))
    f0, g0 = int(pa[hit[0]]), int(pb[hit[0]])
    # the component: closure of the adjacency
    conn = np.zeros(n, bool); conn[[f0, g0]] = True
    while True:
        more = conn | paired[conn].any(axis=0)
        if (more == conn).all():
            break
        conn = more
    # synchronous rounds
    registered = np.zeros(n, bool); registered[[f0, g0]] = True
    mark = np.zeros(N, bool)
    work = np.array([f0])
    rounds = 0
    while True:
        in_work = np.isin(frame_of[own], work)
        fire_row = in_work & registered[frame_of[ent]]
        firing = np.zeros(N, bool); firing[own[fire_row]] = True
        mark[ent[firing[own] & in_work]] = True
        visible = np.bincount(frame_of[mark], minlength=n)
        work = np.flatnonzero(~registered & (visible >= o["min_visible"]))
        if len(work) == 0:
            break
        registered[work] = True
        rounds += 1
    reg = visible >= o["min_visible"]
    key_track, tracks, invalid = array_tracks(case)
    npatch = o["patch_cols"] * o["patch_rows"]
    patch = np.array([q for f in patches_of(case, o) for q in f], np.int64)
    vt = np.array([t if t >= 0 and not invalid[t] else -1 for t in key_track], np.int64)
    # observations of all tracks as rows (track, frame, key of the set)
    t_of = np.array([t for t, ob in enumerate(tracks) for _ in ob], np.int64)
    o_fr = np.array([fr for ob in tracks for fr, _ in ob], np.int64)
    o_gk = np.array([int(kp[fr]) + ky for ob in tracks for fr, ky in ob], np.int64)
    t_beg = np.searchsorted(t_of, np.arange(len(tracks) + 1))
    codes = []
    for i in range(n):
        mine = vt[kp[i]:kp[i + 1]]
        mine = mine[mine >= 0]
        rows = np.concatenate([np.arange(t_beg[t], t_beg[t + 1]) for t in mine]) if conn[i] and len(mine) else np.zeros(0, np.int64)
        rows = rows[(o_fr[rows] != i) & ~paired[i, o_fr[rows]]]
        c, cnt = np.unique(o_fr[rows] * npatch + patch[o_gk[rows]], return_counts=True)
        codes.append(c[cnt >= o["min_patch_obs"]].tolist())
    # rank table: last position of each id
    rp, ri = np.asarray(case["rank_ptr"], np.int64), np.asarray(case["rank_ids"], np.int64)
    rank = np.zeros((n, n), np.int64)
    for f in range(n):
        rank[f, ri[rp[f]:rp[f + 1]]] = np.arange(1, rp[f + 1] - rp[f] + 1)          # (a later assignment wins)
    tried = np.zeros((n, n), bool)
    t = np.asarray(case["tried"], np.int64).reshape(-1, 2)
    tried[t[:, 0], t[:, 1]] = True; tried[t[:, 1], t[:, 0]] = True
    ok = (rank > 0) & ~np.eye(n, dtype=bool) & ~tried & (reg[:, None] | reg[None, :]) & conn[:, None] & conn[None, :]
    cand = []
    for a, b in zip(*np.nonzero(ok)):
        mine = vt[kp[a]:kp[a + 1]]
        mine = mine[mine >= 0]
        shared = sum(1 for t_ in mine if b in o_fr[t_beg[t_]:t_beg[t_ + 1]])
        cand.append((int(a), int(b), int(shared), len(np.intersect1d(codes[a], codes[b]))))
    keys = {}
    for a, b, sh, cv in cand:
        if sh <= o["max_shared_matches"] and cv >= o["min_covisible_patches"]:
            keys[(min(a, b), max(a, b))] = 1
    band = lambda lo, hi: ((rank > lo) & (rank <= hi) & reg[None, :]).sum(axis=1)
    c2, c3 = band(o["mayreg_rank_lo"], o["mayreg_rank_mid"]), band(o["mayreg_rank_mid"], o["mayreg_rank_hi"])
    may = ~conn & ((c2 >= o["mayreg_count_mid"]) | (c2 + c3 >= o["mayreg_count_sum"]))
    near = ((rank > 0) & (rank <= o["similarity_rank_max"]))
    sim = may[:, None] & reg[None, :] & ~tried & (near | near.T)
    for a, b in zip(*np.nonzero(sim)):
        keys.setdefault((min(int(a), int(b)), max(int(a), int(b))), 2)
    return dict(key_track=key_track, tracks=[(ob, inv) for ob, inv in zip(tracks, invalid)], connected=conn.tolist(), visible=visible.tolist(), rounds=rounds,
                registered=reg.tolist(), codes=codes, cand=cand, may_register=may.tolist(), pairs=[(a, b, keys[(a, b)]) for a, b in sorted(keys)])


FIELDS = ("key_track", "tracks", "connected", "visible", "rounds", "registered", "codes", "cand", "may_register", "pairs")


def same(x, y):
    """the fields in which two results differ"""
    norm = lambda v: [tuple(norm(e)) if isinstance(e, (list, tuple)) else (bool(e) if isinstance(e, (bool, np.bool_)) else int(e)) for e in v] if isinstance(v, (list, tuple)) else int(v)
    return [k for k in FIELDS if norm(x[k]) != norm(y[k])]
