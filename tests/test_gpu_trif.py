"""Frame triangulation on the GPU against (B) of tests/trif_yardstick.py on the catalogue of tests/trif_cases.py, the create
arithmetic of the yardstick being capi.triangulate_tracks on the same lists: every integer output of every case in both modes, created
points bit for bit, untouched tracks bit for bit; two scenes appended in one call, map mode as frame mode frame by frame, the result fed
to capi.merge_tracks, a second call on the result, and the leases of a one-shot call."""
import functools

import numpy as np
import pytest

from tests import trif_cases as TC
from tests import trif_yardstick as Y

pytestmark = pytest.mark.gpu

STATE = ("track_of_key", "track_outlier", "points")


class GpuCreate:
    """the create callback on the GPU: xrsfm_ba_triangulate_tracks on the lists, one call per batch, results kept per list"""

    def __init__(self, c):
        self.q, self.t, self.seen, self.calls = c["cam_q"], c["cam_t"], {}, 0

    def __call__(self, lists):
        from xrsfm_amd import capi
        keys = [(np.asarray(cams, np.int32).tobytes(), np.asarray(xy, np.float64).tobytes()) for cams, xy in lists]
        todo = [i for i, k in enumerate(keys) if k not in self.seen]
        if todo:
            ptr = np.concatenate([[0], np.cumsum([len(lists[i][0]) for i in todo])]).astype(np.int32)
            r = capi.triangulate_tracks(self.q, self.t, ptr, np.concatenate([lists[i][0] for i in todo]), np.concatenate([lists[i][1] for i in todo]))
            self.calls += 1
            for j, i in enumerate(todo):
                self.seen[keys[i]] = dict(status=int(r["status"][j]), point=r["points"][j].copy(), mask=r["inlier_mask"][ptr[j]:ptr[j + 1]].copy(),
                                          num_inliers=int(r["num_inliers"][j]), num_trials=int(r["num_trials"][j]), best_trial=int(r["best_trial"][j]))
        return [self.seen[k] for k in keys]


def call(c, frames, **kw):
    from xrsfm_amd import capi
    r = capi.triangulate_frames(c["key_ptr"], c["key_xyn"], c["registered"], c["cam_q"], c["cam_t"], c["corr_ptr"], c["corr_key"], frames, c["points"], c["track_outlier"],
                                c["track_of_key"], **kw)
    r["stats"] = np.array(list(r["stats"].values()), np.int64)
    return r


def want(c, frames):
    """(B) with the GPU's create arithmetic: every list of the call in one launch, then the program"""
    create = GpuCreate(c)
    lists = [l for l in Y.all_lists(c, frames) if len(l[0]) <= Y.MAX_OBS]
    if lists:
        create(lists)
    r = Y.run_flat(c, frames, create)
    assert create.calls <= 1
    return r


@functools.lru_cache(maxsize=None)
def wanted(name, mode):
    c = TC.case(name)
    return want(c, TC.frames_of(c, mode))


def same_bits(a, b, keys):
    return [k for k in keys if np.ascontiguousarray(a[k]).tobytes() != np.ascontiguousarray(b[k]).tobytes()]


@pytest.mark.parametrize("name,mode", [(n, m) for n in TC.NAMES for m in TC.MODES])
def test_every_output_equals_the_yardstick(lib, name, mode):
    c, w = TC.case(name), wanted(name, mode)
    got = call(c, TC.frames_of(c, mode))
    assert Y.integer_differences(got, w) == []
    T = len(c["points"])
    assert got["points"][:T].tobytes() == c["points"].tobytes() and got["track_outlier"][:T].tobytes() == c["track_outlier"].tobytes()      # untouched tracks
    assert got["points"][T:].tobytes() == w["points"][T:].tobytes()                # created points: the bits of xrsfm_ba_triangulate_tracks on the same lists
    print("%s %s: stats %s, %d tracks created" % (name, mode, got["stats"].tolist(), got["n_tracks"] - T))


def appended(a, b):
    """two cases as one map: b's frames, keys and tracks behind a's"""
    Na, Ta = int(a["key_ptr"][-1]), len(a["points"])
    cat = lambda k: np.concatenate([a[k], b[k]])
    return dict(key_ptr=np.concatenate([a["key_ptr"], b["key_ptr"][1:] + Na]), key_xyn=cat("key_xyn"), registered=cat("registered"), cam_q=cat("cam_q"), cam_t=cat("cam_t"),
                corr_ptr=np.concatenate([a["corr_ptr"], b["corr_ptr"][1:] + a["corr_ptr"][-1]]), corr_key=np.concatenate([a["corr_key"], b["corr_key"] + Na]).astype(np.int32),
                points=cat("points"), track_outlier=cat("track_outlier"),
                track_of_key=np.concatenate([a["track_of_key"], np.where(b["track_of_key"] >= 0, b["track_of_key"] + Ta, -1)]).astype(np.int32))


@pytest.mark.parametrize("mode", TC.MODES)
def test_two_scenes_appended_give_each_scenes_solo_result(lib, mode):
    """scene_a's frames first, then those of `rules`: a's tracks keep their ids, b's old tracks are shifted by a's, b's new ones come
    after a's new ones"""
    a, b = TC.case("scene_a"), TC.case("rules")
    na, Na, Ta, Tb = len(a["key_ptr"]) - 1, int(a["key_ptr"][-1]), len(a["points"]), len(b["points"])
    fa, fb = TC.frames_of(a, mode), TC.frames_of(b, mode)
    ra, rb, r = call(a, fa), call(b, fb), call(appended(a, b), fa + [f + na for f in fb])
    new_a = ra["n_tracks"] - Ta
    # the ids of the joint call from those of the solo calls
    ida = np.where(ra["track_of_key"] >= Ta, ra["track_of_key"] + Tb, ra["track_of_key"])
    idb = np.where(rb["track_of_key"] >= Tb, rb["track_of_key"] + Ta + new_a, np.where(rb["track_of_key"] >= 0, rb["track_of_key"] + Ta, -1))
    assert np.array_equal(r["track_of_key"][:Na], ida) and np.array_equal(r["track_of_key"][Na:], idb)
    assert r["n_tracks"] == ra["n_tracks"] + rb["n_tracks"]
    assert r["points"].tobytes() == np.concatenate([ra["points"][:Ta], rb["points"][:Tb], ra["points"][Ta:], rb["points"][Tb:]]).tobytes()
    for k, cut in (("key_status", Na), ("num_inliers", Na), ("num_trials", Na), ("best_trial", Na), ("corr_have_point3d", Na), ("visible", na), ("measured", na)):
        assert r[k][:cut].tobytes() == ra[k].tobytes() and r[k][cut:].tobytes() == rb[k].tobytes(), k
    assert r["stats"][:7].tolist() == (ra["stats"][:7] + rb["stats"][:7]).tolist() and r["stats"][7] == max(ra["stats"][7], rb["stats"][7])


@pytest.mark.parametrize("name", ("rules", "scene_a"))
def test_map_mode_is_frame_mode_frame_by_frame(lib, name):
    c = TC.case(name)
    whole = call(c, TC.frames_of(c, "map"))
    state, status, total = dict(c), np.zeros(len(c["track_of_key"]), np.uint8), np.zeros(8, np.int64)
    for f in TC.frames_of(c, "map"):
        r = call(state, [f])
        state = dict(state, **{k: r[k] for k in STATE})
        status = np.where(r["key_status"] > 0, r["key_status"], status)
        total[:7] += r["stats"][:7]; total[7] = max(total[7], r["stats"][7])
    assert same_bits(state, whole, STATE) == [] and same_bits(r, whole, ("corr_have_point3d", "visible", "measured")) == []
    # (the steps are cut by the state at a call's start, so only the reference's five counters add up)
    assert total[:5].tolist() == whole["stats"][:5].tolist() and total[5] <= whole["stats"][5]
    # a key point's status is that of the call which visits it; 2 is given by every call that lists its frame while it has no track
    assert np.array_equal(status, whole["key_status"])


@pytest.mark.parametrize("name", ("scene_a", "scene_b"))
def test_merge_tracks_accepts_the_result(lib, name):
    """the state invariants hold after a frame-mode call: xrsfm_ba_merge_tracks in frame mode takes the three arrays (a pinhole camera of
    focal length 1 makes the normalised coordinates its pixels)"""
    from xrsfm_amd import capi
    c = TC.case(name)
    r = call(c, TC.frames_of(c, "frame"))
    n = len(c["registered"])
    m = capi.merge_tracks(c["key_ptr"], c["key_xyn"], c["registered"], c["cam_q"], c["cam_t"], np.zeros(n, np.int32), np.zeros(1, np.int32),
                          np.array([[1.0, 0, 0, 0, 0, 0, 0, 0]]), c["corr_ptr"], c["corr_key"], r["points"], r["track_outlier"], r["track_of_key"],
                          options=capi.merge_options(max_reproj_error=0.01, mode=4, frame=int(c["frame"])))
    assert len(m["points"]) == r["n_tracks"] > len(c["points"]) and m["stats"]["components"] > 0
    f = int(c["frame"])
    assert r["measured"][f] == r["stats"][0] + r["stats"][2] > 0             # frame f carried no track before: one per create (the key point is an inlier) and extend


@pytest.mark.parametrize("name,mode", (("rules", "frame"), ("scene_a", "map")))
def test_a_second_call_does_what_the_rule_says(lib, name, mode):
    """on the result of a call, a second call creates and extends exactly what (B) does on that state"""
    c = TC.case(name)
    frames = TC.frames_of(c, mode)
    r1 = call(c, frames)
    state = dict(c, **{k: r1[k] for k in STATE})
    r2, w2 = call(state, frames), want(state, frames)
    assert Y.integer_differences(r2, w2) == [] and r2["points"].tobytes() == w2["points"].tobytes()
    assert r2["points"][:r1["n_tracks"]].tobytes() == r1["points"].tobytes() and (r2["track_of_key"][r1["track_of_key"] >= 0] == r1["track_of_key"][r1["track_of_key"] >= 0]).all()
    if name == "rules":            # frame 5 again: its creates are done, the refusals are refused again
        assert r2["stats"][:3].tolist() == [0, 2, 0] and r2["n_tracks"] == r1["n_tracks"]     # (the create branch: the diverging rays and the long list)


def test_blocks_come_back_and_a_second_call_is_the_first(lib):
    from xrsfm_amd import capi
    c = TC.case("rules")
    capi.quiesce()
    r1 = call(c, [5])
    c1 = capi.quiesce()
    r2 = call(c, [5])
    c2 = capi.quiesce()
    assert c1 > 0 and c2 == c1
    assert same_bits(r1, r2, sorted(r1)) == []
