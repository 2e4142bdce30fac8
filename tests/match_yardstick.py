"""The yardstick of xrsfm_ba_match_descriptors: the SIFT matcher restated in numpy on exact integers, twice, and the
catalogue of pairs the CPU and GPU tests run.  Not collected as a test.

Formulation 1: scores by int64 matmul, the triples (best, idx, next) by a stable sort, the table in np.longdouble rounded to float32.
Formulation 2: scores by float64 matmul (exact: every partial sum is an integer below 2^53) and a running update over ascending
positions, the update of RowMatch_Kernel.  Every output is an integer; the tests demand equality."""
import functools

import numpy as np

DIM = 128
TAB_MAX = 1 << 18
MAX_FEATURES = 16384
DEFAULTS = dict(max_distance=0.7, max_ratio=0.8, mutual_best=1, max_features=16384)
SIZES = (0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 257)
STRIP, COLS, TILE = 128, 64, 16              # the kernel's strip of rows, LDS block of columns and matrix tile


@functools.lru_cache(None)
def table():
    """dist(d) = (float) acos(min((double) ((float) d * 2^-18f), 1.0)), d = 0 .. 2^18, through np.longdouble"""
    x = (np.arange(TAB_MAX + 1, dtype=np.float32) * np.float32(2.0 ** -18)).astype(np.longdouble)
    return np.arccos(np.minimum(x, np.longdouble(1))).astype(np.float32)


def dist(d):
    return table()[np.minimum(np.asarray(d, np.int64), TAB_MAX)]


def options(**kw):
    o = dict(DEFAULTS)
    o.update(kw)
    return o


# ---------------------------------------------------------------------------------------------------- formulation 1
def scores(a, b):
    return a.astype(np.int64) @ b.astype(np.int64).T


def top2_rows(S):
    """[n][3] (best, idx, next) of every row of S by a stable sort: the lowest index of a tied best comes first"""
    n, m = S.shape
    out = np.zeros((n, 3), np.int64)
    out[:, 1] = -1
    if n == 0 or m == 0:
        return out
    order = np.argsort(-S, axis=1, kind="stable")
    first = S[np.arange(n), order[:, 0]]
    out[:, 0] = np.maximum(first, 0)
    out[:, 1] = np.where(first > 0, order[:, 0], -1)
    if m > 1:
        out[:, 2] = np.maximum(S[np.arange(n), order[:, 1]], 0)
    return out


# ---------------------------------------------------------------------------------------------------- formulation 2
def top2_rows_running(Sf):
    """the same by the running update (v > best) over ascending columns, on a float64 score matrix"""
    n, m = Sf.shape
    best, idx, nxt = np.zeros(n), np.full(n, -1, np.int64), np.zeros(n)
    for j in range(m):
        v = Sf[:, j]
        test = v > best
        nxt = np.where(test, best, np.maximum(nxt, v))
        idx = np.where(test, j, idx)
        best = np.where(test, v, best)
    return np.stack([best.astype(np.int64), idx, nxt.astype(np.int64)], 1)


def keep(top, o):
    d, dn = dist(top[:, 0]), dist(top[:, 2])
    return (d < np.float32(o["max_distance"])) & (d < dn * np.float32(o["max_ratio"]))           # float32 throughout


def run_pair(a, b, o=None, running=False):
    o = options() if o is None else o
    a, b = a[:o["max_features"]], b[:o["max_features"]]
    if running:
        S = a.astype(np.float64) @ b.astype(np.float64).T
        row_top, col_top = top2_rows_running(S), top2_rows_running(S.T)
    else:
        S = scores(a, b)
        row_top, col_top = top2_rows(S), top2_rows(S.T.copy())
    row_match = np.where(keep(row_top, o), row_top[:, 1], -1)
    col_match = np.where(keep(col_top, o), col_top[:, 1], -1)
    m = [(i, int(j)) for i, j in enumerate(row_match) if j >= 0 and (not o["mutual_best"] or col_match[j] == i)]
    return dict(row_top=row_top.astype(np.int32), col_top=col_top.astype(np.int32), row_match=row_match, col_match=col_match,
                matches=np.array(m, np.int32).reshape(-1, 2), num_row=int((row_match >= 0).sum()), num_col=int((col_match >= 0).sum()))


# ---------------------------------------------------------------------------------------------------- synthetic descriptors
def sift_like(rng, n):
    x = rng.gamma(0.5, 1.0, (n, DIM))
    x /= np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-30)
    x = np.minimum(x, 0.2)
    x /= np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-30)
    return np.minimum(np.floor(512.0 * x + 0.5), 255).astype(np.uint8)


def perturb(rng, d, amp=6):
    return np.clip(d.astype(np.int64) + rng.integers(-amp, amp + 1, d.shape), 0, 255).astype(np.uint8)


def related(rng, a, n_b, share=2.0 / 3.0):
    """frame B of n_b descriptors: perturbed copies of distinct descriptors of `a` at random positions, the rest unrelated.
    Returns (B, src) with src[k] the descriptor of a that B[k] copies, or -1."""
    b, src = sift_like(rng, n_b), np.full(n_b, -1, np.int64)
    k = min(int(share * n_b), len(a))
    pos, pick = rng.permutation(n_b)[:k], rng.permutation(len(a))[:k]
    b[pos], src[pos] = perturb(rng, a[pick]), pick
    return b, src


# ---------------------------------------------------------------------------------------------------- the catalogue
@functools.lru_cache(None)
def catalogue():
    """(frames, entries): frames a list of uint8 [n][128]; entries dicts tag, a, b (frame indices), opt (overrides of DEFAULTS)"""
    rng = np.random.default_rng(20260519)
    frames, entries = [], []

    def frame(d):
        frames.append(np.ascontiguousarray(d, np.uint8).reshape(-1, DIM))
        return len(frames) - 1

    def entry(tag, a, b, **opt):
        entries.append(dict(tag=tag, a=a, b=b, opt=opt))

    # shapes: every combination of SIZES; A_n = M[:n], B_m = Bm[:m], Bm related to M
    M = sift_like(rng, SIZES[-1])
    Bm, _ = related(rng, M, SIZES[-1])
    fa = {n: frame(M[:n]) for n in SIZES}
    fb = {m: frame(Bm[:m]) for m in SIZES}
    for n in SIZES:
        for m in SIZES:
            entry("shape_%dx%d" % (n, m), fa[n], fb[m])
    for m in SIZES:                                               # the transposes of a row of shapes: frame A_257 in 24 pairs
        entry("shapeT_%dx257" % m, fb[m], fa[257])
    entry("self_129", fa[129], fa[129])
    # several strips: the merge of the column partials
    for na, nb in ((1000, 1200), (300, 129)):
        a = sift_like(rng, na)
        b, _ = related(rng, a, nb)
        entry("strips_%dx%d" % (na, nb), frame(a), frame(b))
    # the best and the second best of row 7 in the last partial tile; of column 3 in strips 0 and 2
    a, b = sift_like(rng, 300), sift_like(rng, 131)
    b[129], b[130] = perturb(rng, a[7], 3), perturb(rng, a[7], 12)
    a[5], a[290] = perturb(rng, b[3], 3), perturb(rng, b[3], 12)
    entry("edge_300x131", frame(a), frame(b))
    # extreme values
    f_hi_a, f_hi_b = frame(rng.integers(128, 256, (40, DIM))), frame(rng.integers(128, 256, (50, DIM)))
    entry("high_40x50", f_hi_a, f_hi_b)
    f255 = frame(np.full((20, DIM), 255))
    entry("all255_20x20", f255, f255)
    entry("all255_high", f255, f_hi_b)
    a = sift_like(rng, 66)
    b, src = related(rng, a, 70)
    a[3] = 0; a[17] = 0; b[5] = 0
    fz_a, fz_b = frame(a), frame(b)
    entry("zero_rows_66x70", fz_a, fz_b)
    entry("all_zero_17x33", frame(np.zeros((17, DIM))), frame(np.zeros((33, DIM))))
    # ties: a duplicated descriptor in B (row tie), in A (column tie)
    a = sift_like(rng, 65)
    b, src = related(rng, a, 70)
    k1 = int(np.flatnonzero(src >= 0)[0]); k2 = int(np.flatnonzero(src < 0)[0])
    b[k2] = b[k1]
    ft_a, ft_b = frame(a), frame(b)
    entry("tie_row", ft_a, ft_b)
    a2 = a.copy()
    r1 = int(src[np.flatnonzero(src >= 0)[1]]); r2 = next(r for r in range(65) if r not in set(src.tolist()))
    a2[r2] = a2[r1]
    ft_a2 = frame(a2)
    entry("tie_col", ft_a2, ft_b)
    # options
    entry("no_mutual_129x257", fa[129], fb[257], mutual_best=0)
    entry("no_mutual_tie_col", ft_a2, ft_b, mutual_best=0)
    a = sift_like(rng, 130)
    b, _ = related(rng, a, 130)
    f130a, f130b = frame(a), frame(b)
    entry("clip100", f130a, f130b, max_features=100)
    entry("clip100_T", f130b, f130a, max_features=100)
    entry("ratio1_129x257", fa[129], fb[257], max_ratio=1.0)
    entry("ratio1_tie_row", ft_a, ft_b, max_ratio=1.0)
    a = sift_like(rng, 65)                                        # a second, slightly worse copy of a matched descriptor: the ratio decides
    b, src = related(rng, a, 70)
    k1 = int(np.flatnonzero(src >= 0)[0])
    shrunk = lambda f: perturb(rng, np.floor(f * a[int(src[k1])]).astype(np.uint8), 4)      # below the clamp of the distance at 2^18
    b[k1], b[int(np.flatnonzero(src < 0)[0])] = shrunk(0.92), shrunk(0.90)
    f_near_a, f_near_b = frame(a), frame(b)
    entry("near_65x70", f_near_a, f_near_b)
    entry("ratio1_near", f_near_a, f_near_b, max_ratio=1.0)
    r = run_pair(frames[fa[129]], frames[fb[257]])
    i = int(r["matches"][0][0])
    entry("distance_at_best", fa[129], fb[257], max_distance=float(dist(r["row_top"][i, 0])))
    # structure: (a, b) and (b, a)
    entry("ab", f130a, f130b)
    entry("ba", f130b, f130a)
    return frames, entries


def frames():
    return catalogue()[0]


def entries():
    return catalogue()[1]


def entry_options(e):
    return options(**e["opt"])


def option_groups():
    """options (sorted tuple of the overrides) -> the entries that use them, in catalogue order"""
    g = {}
    for k, e in enumerate(entries()):
        g.setdefault(tuple(sorted(e["opt"].items())), []).append(k)
    return g


@functools.lru_cache(None)
def reference(k, running=False):
    e = entries()[k]
    return run_pair(frames()[e["a"]], frames()[e["b"]], entry_options(e), running)


def call_arrays(ks):
    """(desc_ptr, desc, pair_a, pair_b) of a call with the pairs of the entries ks: every frame of the catalogue, in its order"""
    F = frames()
    ptr = np.zeros(len(F) + 1, np.int64)
    ptr[1:] = np.cumsum([len(f) for f in F])
    E = entries()
    return ptr, np.concatenate(F), np.array([E[k]["a"] for k in ks], np.int32), np.array([E[k]["b"] for k in ks], np.int32)


def expected(ks):
    """the outputs of a call with the entries ks (all of one option set): match_ptr, matches, num_row, num_col"""
    R = [reference(k) for k in ks]
    ptr = np.zeros(len(ks) + 1, np.int64)
    ptr[1:] = np.cumsum([len(r["matches"]) for r in R])
    m = np.concatenate([r["matches"] for r in R]) if R else np.zeros((0, 2), np.int32)
    return dict(match_ptr=ptr, matches=m.astype(np.int32).reshape(-1, 2), num_row=np.array([r["num_row"] for r in R], np.int32),
                num_col=np.array([r["num_col"] for r in R], np.int32))


def main_group():
    return option_groups()[()]


def batch257():
    """257 pairs: the small entries of the main group, repeated"""
    F, E = frames(), entries()
    small = [k for k in main_group() if len(F[E[k]["a"]]) <= 300 and len(F[E[k]["b"]]) <= 300]
    return [small[(7 * i) % len(small)] for i in range(257)]
