"""Track completion and merging on the GPU against tests/merge_yardstick.py on the catalogue of tests/merge_cases.py:
every integer output of every case and mode, the points (unmerged: the input's bits; merged: against the longdouble value, within a bar
the yardstick computes from its own float64 run), components above a limit, independence of what else is in the call (two scenes
appended, the closure of a frame), map mode 3 as mode 1 then mode 2, and the leases of a one-shot call."""
import numpy as np
import pytest

from tests import merge_cases as MC
from tests import merge_yardstick as Y

pytestmark = pytest.mark.gpu

STATE = ("track_of_key", "track_outlier", "points")


def call(c, mode, **kw):
    from xrsfm_amd import capi
    r = capi.merge_tracks(*MC.arrays(c), options=capi.merge_options(max_reproj_error=c["max_re"], mode=mode, frame=c["frame"] if mode == 4 else -1, **kw))
    r["stats"] = np.array(list(r["stats"].values()) + [0], np.int64)
    return r


def same_bits(a, b, keys):
    return [k for k in keys if np.ascontiguousarray(a[k]).tobytes() != np.ascontiguousarray(b[k]).tobytes()]


@pytest.mark.parametrize("name,mode", [(n, m) for n in MC.NAMES for m in Y.MODES])
def test_every_output_equals_the_yardstick(lib, name, mode):
    c = MC.case(name)
    want, long_ = MC.expected(name, mode), MC.expected_long(name, mode)
    got = call(c, mode)
    assert Y.integer_differences(got, want) == []
    bars = Y.point_bars(want, long_)
    moved = [t for t in want["received"] if not np.isnan([float(v) for v in long_["points"][t]]).any()]          # the points a merge has set
    assert want["received"] == long_["received"] and (len(want["received"]) > 0) == (want["stats"][0] > 0)
    still = np.setdiff1d(np.arange(len(c["points"])), want["received"])
    assert got["points"][still].tobytes() == c["points"][still].tobytes()                  # unmerged: the input's bits
    worst = 0.0
    for t in moved:
        dev = max(abs(float(np.longdouble(got["points"][t][k]) - long_["points"][t][k])) for k in range(3))
        worst = max(worst, dev / bars[t])
        assert dev <= bars[t], (t, dev, bars[t])
    print("%s mode %d: %d merged points, smallest bar %.3g, worst deviation / bar %.3g, stats %s" % (name, mode, len(moved), min([bars[t] for t in moved], default=0.0), worst,
                                                                                                   got["stats"].tolist()))


def test_a_component_above_a_limit_is_untouched(lib):
    c = MC.case("limits")
    got = call(c, 3)
    comp, sizes = Y.components(c)
    assert sizes[:4] == [1025, 1024, 513, 512] and got["stats"].tolist()[4:7] == [2, 2, 1024]
    tok = c["track_of_key"]
    for k, over in ((0, True), (1, False), (2, True), (3, False)):
        keys = np.nonzero(comp == k)[0]
        tracks = np.unique(tok[keys])
        assert (got["track_status"][tracks] == 3).all() == over
        if over:
            assert np.array_equal(got["track_of_key"][keys], tok[keys]) and got["points"][tracks].tobytes() == c["points"][tracks].tobytes() and not got["track_outlier"][tracks].any()
        else:
            assert (got["track_status"][tracks] > 0).all() and (got["track_status"][tracks] == 2).sum() > 100
    assert Y.integer_differences(got, MC.expected("limits", 3)) == []                      # the rest of the call is what it is without them


def appended(a, b):
    """two cases as one map: b's frames, keys, tracks and cameras behind a's"""
    na, Na, Ta, Ia = len(a["key_ptr"]) - 1, int(a["key_ptr"][-1]), len(a["points"]), len(a["intr_model"])
    cat = lambda k: np.concatenate([a[k], b[k]])
    return dict(key_ptr=np.concatenate([a["key_ptr"], b["key_ptr"][1:] + Na]), key_xy=cat("key_xy"), registered=cat("registered"), cam_q=cat("cam_q"), cam_t=cat("cam_t"),
                cam_intr=np.concatenate([a["cam_intr"], b["cam_intr"] + Ia]), intr_model=cat("intr_model"), intr_params=cat("intr_params"),
                corr_ptr=np.concatenate([a["corr_ptr"], b["corr_ptr"][1:] + a["corr_ptr"][-1]]), corr_key=np.concatenate([a["corr_key"], b["corr_key"] + Na]).astype(np.int32),
                points=cat("points"), track_outlier=cat("track_outlier"), track_of_key=np.concatenate([a["track_of_key"], np.where(b["track_of_key"] >= 0, b["track_of_key"] + Ta, -1)])
                .astype(np.int32), max_re=a["max_re"], frame=a["frame"]), na, Na, Ta


@pytest.mark.parametrize("mode", (1, 2, 3))
def test_two_scenes_appended_give_each_scenes_solo_result(lib, mode):
    a, b = MC.case("scene_a"), MC.case("rules")
    both, na, Na, Ta = appended(a, b)
    ra, rb, r = call(a, mode), call(b, mode), call(both, mode)
    assert r["track_of_key"][:Na].tobytes() == ra["track_of_key"].tobytes()
    assert np.array_equal(r["track_of_key"][Na:], np.where(rb["track_of_key"] >= 0, rb["track_of_key"] + Ta, -1))
    for k, cut in (("points", Ta), ("track_outlier", Ta), ("track_status", Ta), ("corr_have_point3d", Na), ("visible", na), ("measured", na)):
        assert r[k][:cut].tobytes() == ra[k].tobytes() and r[k][cut:].tobytes() == rb[k].tobytes(), k
    assert r["stats"][:6].tolist() == (ra["stats"][:6] + rb["stats"][:6]).tolist()


@pytest.mark.parametrize("name", ("rules", "live", "scene_a", "scene_b"))
def test_the_closure_of_a_frame_gives_the_whole_maps_result(lib, name):
    from xrsfm_amd import capi
    c = MC.case(name)
    whole = call(c, 4)
    s = capi.merge_closure(c["frame"], c["key_ptr"], c["corr_ptr"], c["corr_key"], c["track_of_key"])
    assert 0 < len(s["keys"]) <= len(c["track_of_key"]) and (not name.startswith("scene") or len(s["keys"]) < len(c["track_of_key"]))
    sub = dict(c, key_ptr=s["key_ptr"], key_xy=c["key_xy"][s["keys"]], corr_ptr=s["corr_ptr"], corr_key=s["corr_key"], points=c["points"][s["tracks"]],
               track_outlier=c["track_outlier"][s["tracks"]], track_of_key=s["track_of_key"])
    part = call(sub, 4)
    tok, points, outlier = c["track_of_key"].copy(), c["points"].copy(), c["track_outlier"].copy()
    tok[s["keys"]] = np.where(part["track_of_key"] >= 0, s["tracks"][np.maximum(part["track_of_key"], 0)], -1)
    points[s["tracks"]], outlier[s["tracks"]] = part["points"], part["track_outlier"]
    assert same_bits(dict(track_of_key=tok, points=points, track_outlier=outlier), whole, STATE) == []
    assert part["stats"].tolist() == whole["stats"].tolist()
    assert np.array_equal(part["corr_have_point3d"], whole["corr_have_point3d"][s["keys"]])


@pytest.mark.parametrize("name", ("rules", "sizes", "scene_a"))
def test_mode_3_is_mode_1_then_mode_2(lib, name):
    c = MC.case(name)
    r1 = call(c, 1)
    r2 = call(dict(c, **{k: r1[k] for k in STATE}), 2)
    r3 = call(c, 3)
    assert same_bits(r2, r3, STATE + ("corr_have_point3d", "visible", "measured")) == []
    assert (r1["stats"][:4] + r2["stats"][:4]).tolist() == r3["stats"][:4].tolist()


def test_blocks_come_back_and_a_second_call_is_the_first(lib):
    from xrsfm_amd import capi
    c = MC.case("live")
    capi.quiesce()
    r1 = call(c, 3)
    c1 = capi.quiesce()
    r2 = call(c, 3)
    c2 = capi.quiesce()
    assert c1 > 0 and c2 == c1
    assert same_bits(r1, r2, sorted(r1)) == []
