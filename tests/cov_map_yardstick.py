"""Yardstick of the whole-map covariance tests (tests/test_cov_map_cpu.py, tests/test_gpu_map_covariance.py).

The yardstick is never the library: the camera blocks come from the dense routes of tests/cov_yardstick.py, the point blocks from
those of tests/cov_point_yardstick.py (route A: the dense inverse of J^T J; route B: the Schur complement; eps_ref = their
disagreement; the library stays within 50 x eps_ref + 1e-12 of route A per block).

One more fixture, `deep3`: the smallest sequential problem (tens of cameras at a time, gauge fixed by fix_gauge) that the plan puts
on a level schedule of at least 3 levels with at least one tile column of two or more off-diagonal tiles.  Only there does the
recurrence read a tile Z_im with m > i, that is tile (m, i) TRANSPOSED: level40 has 2 levels and one ancestor per leaf and cannot show
such a read wrong.  The tests assert these facts with xrsfm_ba_debug_chol_plan; they do not assume them.

And a numpy restatement of the tile recurrence of xrsfm_amd/csrc/ba_cov.h on 64-row tiles with a given tile pattern."""
import numpy as np

from tests import cov_point_yardstick as P
from tests import cov_yardstick as Y
from tests import helpers as H

NB = 64
DEEP3_CAMS, DEEP3_POINTS, DEEP3_KOBS, DEEP3_SEED = 36, 540, 3, 32      # (31 .. 35 cameras: 2 levels, or a panel schedule)


def _deep3():
    return Y.fix_gauge(H.make(DEEP3_CAMS, DEEP3_POINTS, DEEP3_KOBS, seed=DEEP3_SEED))


def _long70():
    """Tracks of 70 and 66 observations on a level schedule: nine groups of 10 cameras that share tracks only with a separator of 70
    cameras (7 tile columns: a chain of 7 levels above the leaves), and two points that most or all of the separator sees.  A track
    of more than 64 slots takes the workgroup-per-point kernel of the point pass."""
    rng = np.random.default_rng(2)
    leaves, per, sep = 9, 10, 70
    tracks = []
    for l in range(leaves):
        base = l * per
        for _ in range(60):
            tracks.append(np.sort(rng.choice(per, 3, replace=False) + base))
        for _ in range(30):
            a = rng.choice(per, 2, replace=False) + base
            b = rng.choice(sep, 2, replace=False) + leaves * per
            tracks.append(np.sort(np.concatenate([a, b])))
    for _ in range(150):
        tracks.append(np.sort(rng.choice(sep, 3, replace=False) + leaves * per))
    tracks.append(np.arange(sep) + leaves * per)
    tracks.append(np.sort(rng.choice(sep, 66, replace=False) + leaves * per))
    return Y.fix_gauge(H.make_tracks(leaves * per + sep, tracks, seed=3))


LONG70_POINTS = (-2, -1)          # its two long tracks

FIXTURES = dict(Y.FIXTURES)
FIXTURES["deep3"] = (_deep3, "level")
FIXTURES["long70"] = (_long70, "level")


def deep3_facts(arr):
    """(level schedule?, levels, tile columns, structurally non-zero tiles) of the plan."""
    from xrsfm_amd import capi
    plan = capi.debug_chol_plan(H.to_product(arr))
    return plan["level_schedule"] == 1, plan["levels"], plan["tiles"], plan["tiles_nz"]


def is_deep3(arr):
    lv, n_lv, T, nz = deep3_facts(arr)
    return lv and n_lv >= 3 and nz >= 2 * T


def yard(name):
    """(arr, camera route A, camera eps_ref, point route A, point eps_ref) of a fixture."""
    arr = FIXTURES[name][0]()
    Ac, Bc = Y.route_a(arr), Y.route_b(arr)
    Ap, Bp = P.route_a(arr), P.route_b(arr)
    return arr, Ac, Y.eps_ref(Ac, Bc), Ap, P.eps_ref(Ap, Bp)


# ------------------------------------------------------------------------------------------------ the tile recurrence in numpy
def fill_closed_pattern(nz):
    """Symbolic factorisation of a lower tile pattern nz [T][T] (bool, diagonal set): tile (i, m) fills in when both (i, k) and
    (m, k) are set for a k < m < i."""
    nz = np.array(nz, bool, copy=True)
    T = nz.shape[0]
    for k in range(T):
        rows = [i for i in range(k + 1, T) if nz[i, k]]
        for a in rows:
            for b in rows:
                if a >= b:
                    nz[a, b] = True
    return nz


def levels_of(nz):
    T = nz.shape[0]
    level = np.zeros(T, int)
    for k in range(T):
        for j in range(k):
            if nz[k, j]:
                level[k] = max(level[k], level[j] + 1)
    return level


def selected_inverse(Lf, nz):
    """Z = (L L^T)^-1 on the tiles of the fill-closed lower pattern nz, from the Cholesky factor Lf alone, by the recurrence of
    ba_cov.h (the levels from the root down, m ascending):
        Z_ik = -(sum_{m in I_k} Z_im L_mk) Linv_k,      Z_kk = Linv_k^T (Linv_k - sum_{m in I_k} L_mk^T Z_mk),
    Z_im = tile (i, m) for m <= i, tile (m, i) transposed for m > i.  Returns {(i, k): 64x64 tile}, i >= k."""
    T = nz.shape[0]
    t = lambda M, i, k: M[NB * i:NB * i + NB, NB * k:NB * k + NB]
    level = levels_of(nz)
    Z = {}
    for lv in range(level.max(), -1, -1):
        for k in np.nonzero(level == lv)[0]:
            I = [i for i in range(k + 1, T) if nz[i, k]]
            Linv = np.linalg.inv(t(Lf, k, k))
            for i in I:
                acc = np.zeros((NB, NB))
                for m in I:
                    Zim = Z[(i, m)] if m <= i else Z[(m, i)].T
                    acc += Zim @ t(Lf, m, k)
                Z[(i, k)] = -acc @ Linv
            acc = np.zeros((NB, NB))
            for m in I:
                acc += t(Lf, m, k).T @ Z[(m, k)]
            X = Linv.T @ (Linv - acc)
            Z[(k, k)] = 0.5 * (X + X.T)
    return Z
