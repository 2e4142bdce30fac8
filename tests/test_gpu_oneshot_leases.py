"""The one-shot entries hand everything they took from the process-wide pools back: after a call the device blocks are
in the allocation cache, a second call with the same input leaves the cache exactly as the first did, and computes the same bits.
The inputs are the smallest ones of each entry's own GPU test: one or two catalogue entries of its yardstick, not a workload."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _filter_tracks(capi):
    from tests import helpers as H
    arr = H.make(4, 60, 3, seed=150, outlier_frac=0.08, min_tri_angle_deg=0.2)
    return capi.filter_tracks(H.to_product(arr), 4.0, float(np.deg2rad(1.5)))


def _triangulate_tracks(capi):
    from tests import tri_yardstick as Y
    quat, t, _ = Y.cameras()
    tracks = Y.pool()[:2]
    ptr = np.zeros(3, np.int32)
    ptr[1:] = np.cumsum([len(tr["cams"]) for tr in tracks])
    ocam = np.concatenate([tr["cams"] for tr in tracks]).astype(np.int32)
    oxy = np.ascontiguousarray(np.concatenate([tr["xy"].reshape(-1, 2) for tr in tracks]), np.float64)
    return capi.triangulate_tracks(quat, t, ptr, ocam, oxy, capi.triangulate_options())


def _absolute_pose(capi):
    from tests import pose_yardstick as Y
    ptr, xy, X = Y.arrays(Y.frames_of("defaults")[:2])
    return capi.absolute_pose(ptr, xy, X, capi.absolute_pose_options(**dict(Y.OPTION_SETS["defaults"])))


def _two_view_init(capi):
    from tests import init_yardstick as Y
    idx = next(iter(Y.option_groups().values()))[:2]
    ptr, xa, xb, th = Y.arrays(idx)
    r = capi.two_view_init(ptr, xa, xb, th, capi.two_view_options(**Y.entries()[idx[0]]["opt"]))
    return {k: getattr(r, k) for k in r.FIELDS}


def _verify_pairs(capi):
    from tests import fund_yardstick as Y
    idx = next(iter(Y.option_groups().values()))[:2]
    ptr, xa, xb = Y.arrays(idx)
    return capi.verify_pairs(ptr, xa, xb, capi.verify_pairs_options(**Y.entries()[idx[0]]["opt"]))


def _refine_poses(capi):
    from tests import helpers as H
    probs = [H.make_pose_problem(n, seed=800 + i, model=m) for i, (n, m) in enumerate([(40, 4), (7, 3)])]
    q, t, s = capi.refine_poses([int(p["intr_model"][0]) for p in probs], [p["intr_params"][0] for p in probs],
                                [(p["points"], p["obs_uv"], None) for p in probs], np.array([p["cam_q"][0] for p in probs]),
                                np.array([p["cam_t"][0] for p in probs]))
    fields = ("initial_cost", "final_cost", "n_successful", "n_unsuccessful", "termination", "termination_reason", "lm_steps_attempted", "num_residuals")
    return dict(q=q, t=t, **{f: np.array([getattr(x, f) for x in s]) for f in fields})


def _match_descriptors(capi):
    from tests import match_yardstick as Y
    F, E = Y.frames(), Y.entries()
    # (the catalogue opens with pairs of an empty frame: those return before anything is taken from a pool)
    ks = [k for k in next(iter(Y.option_groups().values())) if len(F[E[k]["a"]]) > 0 and len(F[E[k]["b"]]) > 0][:2]
    ptr, desc, pa, pb = Y.call_arrays(ks)
    return capi.match_descriptors(ptr, desc, pa, pb, capi.match_options(**Y.entries()[ks[0]]["opt"]))


ENTRIES = dict(filter_tracks=_filter_tracks, triangulate_tracks=_triangulate_tracks, absolute_pose=_absolute_pose, two_view_init=_two_view_init,
               verify_pairs=_verify_pairs, refine_poses=_refine_poses, match_descriptors=_match_descriptors)


def outputs(name, capi):
    """one call of the entry on its small input -> its output arrays by name"""
    return {k: np.asarray(v) for k, v in ENTRIES[name](capi).items()}


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_blocks_come_back_and_a_second_call_is_the_first(lib, name):
    from xrsfm_amd import capi
    capi.quiesce()                                  # empties the device cache and the pinned pool: every entry starts from the same state
    r1 = outputs(name, capi)
    c1 = capi.quiesce()
    r2 = outputs(name, capi)
    c2 = capi.quiesce()
    print("%s: cached after the first call %d bytes, after the second %d" % (name, c1, c2))
    assert c1 > 0                                   # the call's device blocks came back to the cache
    assert c2 == c1                                 # ... and nothing was kept
    assert sorted(r1) == sorted(r2) and len(r1) > 0
    for k in r1:
        assert r1[k].dtype == r2[k].dtype and r1[k].shape == r2[k].shape and r1[k].tobytes() == r2[k].tobytes(), (name, k)
