"""The case catalogue of the track filter tests (tests/test_filter_cpu.py, tests/test_gpu_filter.py): small problems, each with a list of
(max_re, min_angle) settings, grouped as

  generated   two scenes with track lengths 2 .. 9 (dropout), one with all five camera models; gross outliers, points behind the cameras,
              points beyond depth 1e3, far points with small angles; each at the mapper's (4.0, 1.5 deg) and at (2.0, 3 deg)
  lengths     tracks of 0, 1, 2, 3, 5, 33, 65 and 130 observations in one problem, with the deletions that the n - 1 rule distinguishes
  launch      n_points in {1, 127, 128, 129, 257} (128 tracks per block) and n_cams in {1, 255, 256, 257} (256 cameras per block of
              k_cam_centres), the last camera observed
  order       one scene with gaps, the same with its observation list permuted, the same with its points relabelled
  exit        hand-built tracks: the first pair exits; a later pair exits while a still later one is larger; no pair exits
  degenerate  a point on a camera centre (den == 0), two observations with one centre (alone and with a third camera, also at min_angle = 0),
              a pair with a baseline 1e-7 of the depth whose float64 operand of acos lies above 1, an obtuse pair (the fold)
  exact       thresholds met exactly, from small integers and powers of two: every float64 operation is exact under any contraction and the
              expectations are written by hand (EXACT_EXPECT); the only group that may hold a fragile decision
  near        for one observation max_re just outside re +- 4 bars, for one track min_angle just outside angle +- 4 bars, for four points the
              depth moved to 1e-3 +- 1e-12 and 1e3 +- 1e-6
  nonfinite   one track whose point is NaN

Every problem is built once and must not be modified by a caller; the yardstick of a (case, setting) is computed once (reference())."""
import math

import numpy as np

from tests import filter_yardstick as Y
from tests import helpers as H

LD, F64 = Y.LD, np.float64
MAPPER = (4.0, math.radians(1.5))               # rec_1dsfm.cc:90-91
OTHER = (2.0, math.radians(3.0))
KITTI = (718.856, 607.1928, 185.27157, 0.0)


# ------------------------------------------------------------------------------------------------ builders
def _own(arr):
    return {k: np.array(arr[k], copy=True) for k in H.FIELDS}


def _cam_of(arr, c):
    i = arr["cam_intr"][c]
    return arr["cam_q"][c], arr["cam_t"][c], int(arr["intr_model"][i]), arr["intr_params"][i]


def projection(arr, c, P):
    """float64 projection (u, v) of the point P into camera c"""
    with np.errstate(all="ignore"):
        u, v, _ = Y.project64(*_cam_of(arr, c), np.asarray(P, F64))
    return np.array([u, v])


def resynth(arr, seed, sigma, only=None):
    """observations := the float64 projections at the problem's own state + N(0, sigma) noise (where the projection is finite)"""
    rng = np.random.default_rng(seed)
    noise = rng.normal(0, sigma, arr["obs_uv"].shape)
    for i in (range(arr["obs_cam"].shape[0]) if only is None else only):
        uv = projection(arr, arr["obs_cam"][i], arr["points"][arr["obs_pt"][i]])
        if np.isfinite(uv).all():
            arr["obs_uv"][i] = uv + noise[i]
    return arr


def obs_index(arr, pt, cam):
    i = np.nonzero((arr["obs_pt"] == pt) & (arr["obs_cam"] == cam))[0]
    assert len(i) == 1
    return int(i[0])


def centre64(q, t):
    M = np.array(Y._mat64(q)).reshape(3, 3)
    return -(M.T @ np.asarray(t, F64))


def assemble(cams, points, obs):
    """cams: list of (q, t, model, params); every camera gets its own intrinsics record.  obs: list of (cam, point, u, v) or (cam, point) -
    the latter observed at the float64 projection."""
    n = len(cams)
    prm = np.zeros((n, 8))
    for i, c in enumerate(cams):
        prm[i, :len(c[3])] = c[3]
    arr = dict(cam_q=np.array([c[0] for c in cams], F64).reshape(n, 4), cam_t=np.array([c[1] for c in cams], F64).reshape(n, 3), cam_const=np.zeros(n, np.uint8),
               cam_intr=np.arange(n, dtype=np.int32), intr_model=np.array([c[2] for c in cams], np.int32), intr_params=prm,
               points=np.array(points, F64).reshape(len(points), 3), point_const=np.zeros(len(points), np.uint8),
               obs_cam=np.array([o[0] for o in obs], np.int32), obs_pt=np.array([o[1] for o in obs], np.int32), obs_uv=np.zeros((len(obs), 2)))
    for i, o in enumerate(obs):
        arr["obs_uv"][i] = o[2:4] if len(o) == 4 else projection(arr, o[0], arr["points"][o[1]])
    return arr


def mat_ld(q):
    """M(q) in long double"""
    return np.array([[x.v[0] for x in row] for row in Y._quat_mat(np.asarray(q, F64)[None])], LD)


def posed(rng, centre, tilt=0.05, forward=None):
    """(q, t): a unit quaternion `tilt` radians from the identity (or from `forward`), t = -M c rounded once from long double"""
    d = rng.normal(0, tilt, 3)
    q = np.concatenate([d / 2, [1.0]]) if forward is None else np.asarray(forward, F64) + np.concatenate([d / 2, [0.0]])
    q = q / np.linalg.norm(q)
    return q, np.asarray(-(mat_ld(q) @ np.asarray(centre, LD)), F64)


def scene(seed, models, n_cams=12, n_points=240):
    arr = _own(H.make(n_cams, n_points, 9, seed=seed, dropout=0.5, outlier_frac=0.0, min_tri_angle_deg=0.2))
    if models:
        arr = _own(H.with_models(arr, seed=seed))
    P = arr["points"]
    first = np.full(n_points, -1)
    first[arr["obs_pt"][::-1]] = arr["obs_cam"][::-1]
    P[::40] += np.array([0.0, 0.0, -70.0])                            # behind the cameras
    P[7::60] *= 40.0                                                  # beyond depth 1e3 (or behind)
    for j in range(11, n_points, 45):                                 # far: ten times the distance from its first camera, small angles
        c = centre64(arr["cam_q"][first[j]], arr["cam_t"][first[j]])
        P[j] = c + 10.0 * (P[j] - c)
    resynth(arr, seed, 1.6)
    rng = np.random.default_rng(1000 + seed)
    gross = rng.random(arr["obs_uv"].shape[0]) < 0.05
    arr["obs_uv"][gross] += rng.uniform(15, 40, (int(gross.sum()), 2)) * rng.choice([-1.0, 1.0], (int(gross.sum()), 2))
    return arr


# ------------------------------------------------------------------------------------------------ lengths and launch boundaries
LENGTHS = dict(empty=0, single=1, pair=2, pair_one_deleted=3, triple=4, triple_n_minus_2=5, triple_n_minus_1=6, triple_all=7, five=8, l33=9, l65=10, l130=11,
               empty_last_but_one=12, last_camera=13)


def lengths():
    tracks = [[], [3], [0, 5], [1, 6], [0, 4, 9], [2, 5, 8], [1, 4, 7], [3, 6, 9], [10, 20, 30, 40, 50], list(range(0, 132, 4)), list(range(0, 130, 2)),
              list(range(5, 135)), [], [2, 139]]
    arr = resynth(_own(H.make_tracks(140, [np.array(t, np.int64) for t in tracks], seed=21, outlier_frac=0.0)), 21, 0.5)
    for pt, cam in ((3, 6), (5, 5), (6, 1), (6, 7), (7, 3), (7, 6), (7, 9)):
        arr["obs_uv"][obs_index(arr, pt, cam)] += (100.0, -60.0)
    return arr


def launch_points(n):
    return resynth(_own(H.make(6, n, 3, seed=300 + n, min_tri_angle_deg=0.2)), n, 1.5)


def launch_cams(n):
    if n == 1:
        arr = _own(H.make_tracks(2, [np.array([0])] * 5, seed=1, outlier_frac=0.0))
        for k in ("cam_q", "cam_t", "cam_const", "cam_intr"):
            arr[k] = np.ascontiguousarray(arr[k][:1])
        return resynth(arr, 1, 0.5)
    rng = np.random.default_rng(n)
    tracks = [np.sort(rng.choice(n, 3, replace=False)) for _ in range(60)] + [np.array([0, n - 1]), np.array([n - 2, n - 1]), np.array([n // 2, n - 1])]
    return resynth(_own(H.make_tracks(n, tracks, seed=n, outlier_frac=0.0)), n, 1.5)


# ------------------------------------------------------------------------------------------------ caller order
def _order_base():
    arr = scene(5, True, n_points=200)
    rng = np.random.default_rng(3)
    keep = rng.random(arr["obs_cam"].shape[0]) > 0.15
    keep &= ~np.isin(arr["obs_pt"], (0, 17, 199))                    # three points without an observation: the first, one inside, the last
    for f in ("obs_cam", "obs_pt", "obs_uv"):
        arr[f] = np.ascontiguousarray(arr[f][keep])
    return arr


def _order_shuffled():
    arr = dict(case("order_base"))
    perm = np.random.default_rng(4).permutation(arr["obs_cam"].shape[0])
    for f in ("obs_cam", "obs_pt", "obs_uv"):
        arr[f] = np.ascontiguousarray(arr[f][perm])
    ORDER_MAPS["order_shuffled"] = (perm, np.arange(arr["points"].shape[0]))
    return arr


def _order_relabel():
    base = case("order_base")
    arr, perm = H.relabel_points(base, seed=6)
    inv = np.empty(len(perm), np.int64); inv[perm] = np.arange(len(perm))
    ORDER_MAPS["order_relabel"] = (np.lexsort((inv[base["obs_pt"]], base["obs_cam"])), perm)
    return arr


ORDER_MAPS = {}          # name -> (obs_map, pt_map): observation k / point j of the case is observation obs_map[k] / point pt_map[j] of order_base


# ------------------------------------------------------------------------------------------------ early exit
EXIT = dict(first=0, later_below_max=1, none=2, third_pair=3, two_small_then_exit=4)


def exits():
    """five cameras tilted a few degrees, centres on a line: 0.1 apart (0, 1, 2), then at 3 and 9; the points 10 in front"""
    rng = np.random.default_rng(8)
    cams = [posed(rng, c) + (2, KITTI) for c in ((0, 0, 0), (0.1, 0, 0), (0.2, 0.05, 0), (3, 0, 0), (9, 0, 0.5))]
    points = [(0.5, 0.3, 10.0), (0.4, -0.2, 10.5), (0.1, 0.1, 9.5), (-0.3, 0.2, 11.0), (0.2, -0.4, 10.0)]
    tracks = [(0, 3), (0, 1, 3, 4), (0, 1, 2), (0, 1, 2, 3), (1, 2, 4)]
    return resynth(assemble(cams, points, [(c, j) for j, t in enumerate(tracks) for c in t]), 8, 0.3)


# ------------------------------------------------------------------------------------------------ degenerate angles
SHARED = dict(alone=0, with_third=1)


def shared_centre():
    """cameras 1 and 2 have one pose bit for bit"""
    rng = np.random.default_rng(9)
    twin = posed(rng, (1, 0, -10))
    cams = [posed(rng, (0, 0, -10)) + (2, KITTI), twin + (2, KITTI), twin + (2, KITTI), posed(rng, (4, 0, -10)) + (2, KITTI)]
    return resynth(assemble(cams, [(0.5, 0.2, -1.0), (-0.5, 0.1, 0.0)], [(1, 0), (2, 0), (1, 1), (2, 1), (3, 1)]), 9, 0.3)


DEGENERATE = dict(on_centre=0, obtuse=1, above_one=2)


def degenerate():
    """camera 0: q = (1, 0, 0, 1) as given (not normalised: M M^T = diag(1, 5, 5)), t = (0, 0, -1): centre (0, 2, -1), and the point there has
    X = Y = 0 and Z = 4 in that camera, all in integers.  cameras 1, 2: ordinary.  cameras 3, 4: facing each other along z with the point
    between them.  cameras 5, 6: one rotation, centres 1e-6 apart at depth 10, nearly along the ray; the point is searched (deterministically) for a float64
    operand of acos above 1."""
    rng = np.random.default_rng(10)
    cams = [((1.0, 0.0, 0.0, 1.0), (0.0, 0.0, -1.0), 2, KITTI), posed(rng, (0.5, 0, -10)) + (2, KITTI), posed(rng, (4, 1, -10)) + (2, KITTI),
            ((0.0, 0.0, 0.0, 1.0), (0.0, 0.0, 10.0), 2, KITTI), ((0.0, 1.0, 0.0, 0.0), (0.0, -1.0, 10.0), 2, KITTI)]
    points = [(0.0, 2.0, -1.0), (0.3, 0.2, 0.0)]
    obs = [(0, 0, KITTI[1], KITTI[2]), (1, 0), (2, 0), (3, 1), (4, 1)]
    stats = dict(den_zero=0, arg_above_1=0, arg_is_1=0, fold=0)
    for _ in range(500):
        q, t5 = posed(rng, (0.3, -0.2, -10.0))
        P = np.array([0.4, 0.1, 0.0]) + rng.normal(0, 0.3, 3)
        d = (P - np.array([0.3, -0.2, -10.0])) / 10.0 + rng.normal(0, 0.05, 3)          # mostly along the ray: an angle below 1e-8
        c6 = np.array([0.3, -0.2, -10.0]) + 1e-6 * d / np.linalg.norm(d)
        t6 = np.asarray(-(mat_ld(q) @ c6.astype(LD)), F64)
        with np.errstate(all="ignore"):
            Y._angle64(centre64(q, t5), centre64(q, t6), P, (), stats)
        if stats["arg_above_1"]:
            break
    assert stats["arg_above_1"] == 1
    cams += [(q, t5, 2, KITTI), (q, t6, 2, KITTI)]
    points.append(tuple(P))
    obs += [(5, 2), (6, 2)]
    arr = assemble(cams, points, obs)
    return resynth(arr, 10, 0.3, only=range(1, len(obs)))


# ------------------------------------------------------------------------------------------------ exact thresholds
UNIT = (1.0, 0.0, 0.0, 0.0)                                                # f = 1, c = (0, 0), k = 0
Z_LO, Z_HI = F64(1e-3), F64(1e3)
RE_EXACT = (5.0, float(np.nextafter(F64(5.0), F64(0.0))))
# per setting of the case `exact` (max_re = 5, max_re = the double below 5): obs_delete, track_outlier, num_filtered, written by hand.
# tracks: Z = 1e-3 | the double below | Z = 1e3 | the double above | re = 5 (model 2) | re = 5 (model 0 and 2, one centre) | Z = 0 (X = 0 and X = 1)
EXACT_EXPECT = (dict(obs_delete=[0, 0, 1, 1, 0, 0, 1, 1, 0, 0, 0, 0, 1, 1], track_outlier=[0, 1, 2, 1, 0, 2, 1], num_filtered=[6, 2]),
                dict(obs_delete=[0, 0, 1, 1, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1], track_outlier=[0, 1, 2, 1, 1, 1, 1], num_filtered=[10, 1]))
EXACT_Z = [Z_LO, Z_LO, np.nextafter(Z_LO, F64(0)), np.nextafter(Z_LO, F64(0)), Z_HI, Z_HI, np.nextafter(Z_HI, F64(np.inf)), np.nextafter(Z_HI, F64(np.inf)),
           1.0, 1.0, 2.0, 2.0, 0.0, 0.0]
EXACT_RE5 = (8, 9, 10, 11)                                                  # the observations whose re is exactly 5


def exact():
    """cameras 0, 1, 2: identity rotation, t = 0, (1, 0, 0), 0; f = 1, principal point 0, no distortion; camera 2 is model 0 (doubled focal
    length).  Every observation of a depth track sits at its float64 projection."""
    I = (0.0, 0.0, 0.0, 1.0)
    cams = [(I, (0.0, 0.0, 0.0), 2, UNIT), (I, (1.0, 0.0, 0.0), 2, UNIT), (I, (0.0, 0.0, 0.0), 0, UNIT[:3])]
    points = [(0, 0, z) for z in EXACT_Z[0:8:2]] + [(0, 0, 1), (1, 2, 2), (0, 0, 0)]
    obs = [(c, j) for j in range(4) for c in (0, 1)] + [(0, 4, -3.0, -4.0), (1, 4, 4.0, 4.0), (0, 5, 3.5, 5.0), (2, 5, 4.0, 6.0), (0, 6, 0.0, 0.0), (1, 6, 0.0, 0.0)]
    return assemble(cams, points, obs)


ANGLE_EXACT = float(np.sqrt(F64(2.0)) * F64(2.0) ** -26)


def exact_angle():
    """centres 0, (2^-20, 2^-20, 0) and (8, 0, 0), the point (0, 0, 64): for the first pair r1 = 2^12, r2 = 2^12 + 2^-39, b2 = 2^-39, all exact;
    r1 r2 = 2^24 + 2^-27 is exact, its correctly rounded root is 2^12 + 2^-40, den = 2^13 + 2^-39 and the quotient 2^13 / den rounds to
    1 - 2^-52.  acos(1 - 2^-52) = 2^-26 sqrt(2) (1 + 1.8e-17), which lies 0.32 ulp below the double ANGLE_EXACT = 2^-26 sqrt(2) and 0.68 ulp
    above the next one down: an acos with less than 0.68 ulp of error returns ANGLE_EXACT or that neighbour.  With min_angle = ANGLE_EXACT the
    first pair does not exit under `>` (float64: equal or below; long double: below) and the second pair (7 deg) does; under `>=` the first
    pair would."""
    I = (0.0, 0.0, 0.0, 1.0)
    s = 2.0 ** -20
    cams = [(I, (0.0, 0.0, 0.0), 2, UNIT), (I, (-s, -s, 0.0), 2, UNIT), (I, (-8.0, 0.0, 0.0), 2, UNIT)]
    return assemble(cams, [(0.0, 0.0, 64.0)], [(0, 0), (1, 0), (2, 0)])


# ------------------------------------------------------------------------------------------------ near thresholds
NEAR = {}                # what near() chose: obs, track, settings, the moved points


def _outside(x, up):
    return float(np.nextafter(F64(x), F64(np.inf if up else -np.inf)))


def near():
    arr = scene(2, False, n_points=120)
    ci, pi = arr["obs_cam"], arr["obs_pt"]
    ref = Y.reference(arr, *MAPPER)
    live = ref["track_outlier"] == 0
    # four points moved along the optical axis of their first camera until Z = 1e-3 -+ 1e-12, 1e3 -+ 1e-6 (in long double)
    movable = [j for j in np.nonzero(live)[0] if ref["facts"]["n"][j] >= 3][:6]
    targets = (LD(Z_LO) - LD(1e-12), LD(Z_LO) + LD(1e-12), LD(Z_HI) - LD(1e-6), LD(Z_HI) + LD(1e-6))
    moved = []
    for j, target in zip(movable[2:6], targets):
        i = int(np.nonzero(pi == j)[0][0])
        c = ci[i]
        M = mat_ld(arr["cam_q"][c])
        P = arr["points"][j].astype(LD)
        for _ in range(3):
            z = M[2] @ P + LD(arr["cam_t"][c][2])
            P = np.asarray(P + (target - z) / (M[2] @ M[2]) * M[2], F64).astype(LD)
        arr["points"][j] = np.asarray(P, F64)
        arr["obs_uv"][i] = projection(arr, c, arr["points"][j]) + (0.3, -0.2)
        moved.append((i, int(j), target))
    ref = Y.reference(arr, *MAPPER)
    # one kept observation and one track that exits, of the untouched tracks
    i_re = next(int(i) for i in np.nonzero(np.isin(pi, movable[:1]))[0] if 1.0 < ref["re"].v[i] < 3.0)
    j_ang = int(movable[1])
    assert ref["track_outlier"][j_ang] == 0 and ref["facts"]["exit_kind"][j_ang] == "first"
    re, ang = ref["re"][i_re], ref["track_angle"][j_ang]
    settings = [MAPPER, (_outside(re.v + 4 * re.e, True), MAPPER[1]), (_outside(re.v - 4 * re.e, False), MAPPER[1]),
                (MAPPER[0], _outside(ang.v + 4 * ang.e, True)), (MAPPER[0], _outside(ang.v - 4 * ang.e, False))]
    NEAR.update(obs=i_re, track=j_ang, moved=moved, settings=settings)
    return arr


def _near_settings():
    case("near")
    return NEAR["settings"]


# ------------------------------------------------------------------------------------------------ non-finite
NAN_TRACK = 4


def nonfinite():
    arr = resynth(_own(H.make(6, 20, 3, seed=12, min_tri_angle_deg=0.2)), 12, 1.0)
    arr["points"][NAN_TRACK] = np.nan
    return arr


# ------------------------------------------------------------------------------------------------ the catalogue
N_POINTS = (1, 127, 128, 129, 257)
N_CAMS = (1, 255, 256, 257)
# name -> (group, factory, settings or a function that returns them)
CASES = {
    "scene_kitti": ("generated", lambda: scene(1, False), (MAPPER, OTHER)),
    "scene_models": ("generated", lambda: scene(3, True), (MAPPER, OTHER)),
    "lengths": ("lengths", lengths, (MAPPER, (4.0, math.radians(100.0)))),
    **{f"points_{n}": ("launch", (lambda n=n: launch_points(n)), (MAPPER,)) for n in N_POINTS},
    **{f"cams_{n}": ("launch", (lambda n=n: launch_cams(n)), (MAPPER,)) for n in N_CAMS},
    "order_base": ("order", _order_base, (MAPPER,)), "order_shuffled": ("order", _order_shuffled, (MAPPER,)), "order_relabel": ("order", _order_relabel, (MAPPER,)),
    "exits": ("exit", exits, (MAPPER, (4.0, math.radians(20.0)))),
    "shared_centre": ("degenerate", shared_centre, (MAPPER, (4.0, 0.0))),
    "degenerate": ("degenerate", degenerate, (MAPPER, OTHER)),
    "exact": ("exact", exact, tuple((m, MAPPER[1]) for m in RE_EXACT)),
    "exact_angle": ("exact", exact_angle, ((4.0, ANGLE_EXACT),)),
    "near": ("near", near, _near_settings),
    "nonfinite": ("nonfinite", nonfinite, (MAPPER, (4.0, 0.0))),
}
NAMES = tuple(CASES)
GROUPS = tuple(dict.fromkeys(g for g, _, _ in CASES.values()))
_ARR, _REF = {}, {}


def group_of(name):
    return CASES[name][0]


def case(name):
    if name not in _ARR:
        _ARR[name] = CASES[name][1]()
    return _ARR[name]


def settings(name):
    s = CASES[name][2]
    return tuple(s() if callable(s) else s)


def n_settings(name):
    """without building the case (for parametrising)"""
    return 5 if name == "near" else len(CASES[name][2])


RUNS = tuple((n, k) for n in NAMES for k in range(n_settings(n)))


def reference(name, k):
    if (name, k) not in _REF:
        _REF[(name, k)] = Y.reference(case(name), *settings(name)[k])
    return _REF[(name, k)]


# ------------------------------------------------------------------------------------------------ coverage
ROWS = ("by_re_alone", "by_zmin_alone", "by_zmax_alone", "outlier_1", "outlier_2", "model_0", "model_1", "model_2", "model_3", "model_4",
        "exit_first", "exit_later", "exit_below_max", "exit_none", "fold", "beyond_1", "f64_above_1", "f64_exactly_1", "den_zero", "nan_track",
        "len_0", "len_1", "len_2", "len_3", "len_5", "len_33", "len_65", "len_130", "pair_one_deleted", "triple_n_minus_2_kept", "triple_n_minus_1_dropped",
        "all_deleted", "unsorted_obs", "gap_tracks", "last_camera_observed", "more_than_one_block_of_tracks", "more_than_one_block_of_cameras")


def coverage(name):
    """{row: count} of a case, summed over its settings (structure rows counted once)"""
    arr = case(name)
    out = dict.fromkeys(ROWS, 0)
    for k, s in enumerate(settings(name)):
        r = reference(name, k)
        f = r["facts"]
        live = r["track_outlier"] != 1
        out["by_re_alone"] += int((f["by_re"] & ~f["by_zmin"] & ~f["by_zmax"]).sum())
        out["by_zmin_alone"] += int((f["by_zmin"] & ~f["by_re"]).sum())
        out["by_zmax_alone"] += int((f["by_zmax"] & ~f["by_re"]).sum())
        out["outlier_1"] += int((r["track_outlier"] == 1).sum()); out["outlier_2"] += int((r["track_outlier"] == 2).sum())
        kinds = list(f["exit_kind"].values())
        out["exit_first"] += kinds.count("first"); out["exit_later"] += kinds.count("later"); out["exit_none"] += kinds.count("none")
        out["exit_below_max"] += int(f["below_max"].sum())
        out["fold"] += int(f["fold"].sum()); out["beyond_1"] += int(f["beyond"].sum()); out["den_zero"] += int(f["den_zero"].sum())
        out["nan_track"] += int(f["nan_pair"].sum())
        n, nd = f["n"], f["ndel"]
        out["pair_one_deleted"] += int(((n == 2) & (nd == 1)).sum())
        out["triple_n_minus_2_kept"] += int(((n == 3) & (nd == 1) & live).sum())
        out["triple_n_minus_1_dropped"] += int(((n == 3) & (nd == 2) & ~live).sum())
        out["all_deleted"] += int(((n >= 2) & (nd == n)).sum())
        st = Y.restate64(arr, *s)["stats"]
        out["f64_above_1"] += st["arg_above_1"]; out["f64_exactly_1"] += st["arg_is_1"]
    n = reference(name, 0)["facts"]["n"]
    for m in range(5):
        out[f"model_{m}"] = int((reference(name, 0)["facts"]["model"] == m).sum())
    for L in (0, 1, 2, 3, 5, 33, 65, 130):
        out[f"len_{L}"] = int((n == L).sum())
    ci, pi = arr["obs_cam"], arr["obs_pt"]
    by_track = np.argsort(pi, kind="stable")                      # the caller's order inside every track
    out["unsorted_obs"] = int(((np.diff(ci[by_track]) < 0) & (np.diff(pi[by_track]) == 0)).sum())
    out["gap_tracks"] = int((n == 0).sum())
    out["last_camera_observed"] = int((ci == arr["cam_q"].shape[0] - 1).sum())
    out["more_than_one_block_of_tracks"] = int(arr["points"].shape[0] > 128)
    out["more_than_one_block_of_cameras"] = int(arr["cam_q"].shape[0] > 256)
    return out
