"""The track filter's yardstick and catalogue without a GPU (tests/filter_yardstick.py, tests/filter_cases.py): two independent float64
evaluations (the yardstick module's loop restatement and oracle/ba_oracle.py::filter_tracks) pass the checker on every case and setting, no
case outside the exact-threshold group holds a fragile decision, the near-threshold cases sit where they claim, the exact cases give the
hand-written numbers in float64 and in long double bit for bit, the coverage table has no empty row, and every mutated restatement fails the
checker."""
import math

import numpy as np
import pytest

from oracle import ba_oracle as bo
from tests import filter_cases as FC
from tests import filter_yardstick as Y
from tests import helpers as H

LD, F64 = Y.LD, np.float64


# ---------------------------------------------------------------------------------------------------- float64 against the checker
@pytest.mark.parametrize("name,k", FC.RUNS)
def test_both_float64_restatements_pass_the_checker(name, k):
    arr, s, ref = FC.case(name), FC.settings(name)[k], FC.reference(name, k)
    with np.errstate(all="ignore"):
        runs = dict(restatement=Y.restate64(arr, *s), oracle=bo.filter_tracks(H.to_oracle(arr), *s))
    for who, got in runs.items():
        checks = Y.check(ref, got)
        print("%-14s %d %-12s %s" % (name, k, who, "  ".join("%s %.3f" % kv for kv in Y.worst(checks).items())))
        assert Y.failures(checks) == {}, who


def test_the_checker_takes_every_track_by_its_own_bar():
    """a deviation of two bars on one track fails, of half a bar passes; unset values and NaN ask for the same bits"""
    ref = FC.reference("nonfinite", 0)
    good = {k: (np.asarray(ref[k].v, F64) if isinstance(ref[k], Y.V) else ref[k].copy()) for k in Y.CHECKS}
    assert Y.failures(Y.check(ref, good)) == {}
    j = int(np.argmin(np.where(ref["track_angle"].e > 0, ref["track_angle"].e, np.inf)))          # the tightest bar of the case
    for key in ("track_error", "track_angle"):
        for factor, fails in ((0.5, False), (2.0, True)):
            bad = dict(good, **{key: good[key].copy()})
            bad[key][j] += float(factor * ref[key].e[j])
            assert (key in Y.failures(Y.check(ref, bad))) == fails, (key, factor)
    nan = dict(good, track_error=np.where(np.isnan(good["track_error"]), 0.0, good["track_error"]))
    assert "track_error" in Y.failures(Y.check(ref, nan))
    unset = FC.reference("lengths", 0)
    got = {k: (np.asarray(unset[k].v, F64) if isinstance(unset[k], Y.V) else unset[k].copy()) for k in Y.CHECKS}
    got["track_angle"][FC.LENGTHS["single"]] = -1.0 + 2.0 ** -52
    assert list(Y.failures(Y.check(unset, got))) == ["track_angle"]
    for key, index in (("obs_delete", 3), ("track_outlier", 2), ("num_filtered", 1)):
        flipped = dict(good, **{key: good[key].copy()})
        flipped[key][index] += 1
        assert list(Y.failures(Y.check(ref, flipped))) == [key]


# ---------------------------------------------------------------------------------------------------- fragility
@pytest.mark.parametrize("name,k", [r for r in FC.RUNS if FC.group_of(r[0]) != "exact"])
def test_no_decision_is_fragile(name, k):
    ref = FC.reference(name, k)
    assert np.nonzero(ref["fragile_obs"])[0].tolist() == [] and np.nonzero(ref["fragile_track"])[0].tolist() == []


def test_the_bars_are_informative():
    """eps / angle for the angle, a few hundred ulps of a pixel for the error: bar(angle) angle <= 1e-11 on every kept track without a pair
    beyond +-1, bar(error) <= 1e-10, a tenth of the flat tolerance of tests/test_gpu_parity.py; the flat 1e-12 on the angle is exceeded by
    the far points' bars and undercut tenfold by the near ones'"""
    widest, tightest = 0.0, 1.0
    for name, k in FC.RUNS:
        ref = FC.reference(name, k)
        kept = (ref["track_outlier"] != 1) & (ref["facts"]["n"] > 0) & ~ref["facts"]["nan_pair"]
        ang, err = ref["track_angle"][kept & ~ref["facts"]["beyond"]], ref["track_error"][kept]
        assert (ang.e * ang.v <= 1e-11).all() and (err.e <= 1e-10).all(), (name, k)
        some = ang.e[ang.e > 0]
        widest, tightest = max(widest, float(ang.e.max(initial=0))), min(tightest, float(some.min(initial=1)))
    print("bar(angle) from %.1e to %.1e" % (tightest, widest))
    assert tightest < 1e-13 and widest > 1e-12


def test_the_exact_cases_are_the_fragile_ones():
    """the yardstick's own flag sees the thresholds that are met exactly (a positive bar around a value on its threshold)"""
    ref = FC.reference("exact", 0)
    assert ref["fragile_obs"][[0, 1, 4, 5, 8, 9, 10, 11]].all() and FC.reference("exact_angle", 0)["fragile_track"].all()


def test_the_near_cases_sit_four_bars_from_their_thresholds():
    arr, st = FC.case("near"), FC.settings("near")
    i, j, near = FC.NEAR["obs"], FC.NEAR["track"], FC.NEAR
    refs = [FC.reference("near", k) for k in range(5)]
    # max_re on either side of one observation's error
    re = refs[0]["re"][i]
    assert st[2][0] < float(re.v) < st[1][0] and st[1][0] - st[2][0] < 10 * float(re.e) + 1e-15
    for k, deleted in ((1, 0), (2, 1)):
        assert abs(re.v - LD(st[k][0])) >= 4 * re.e > 0 and refs[k]["obs_delete"][i] == deleted
    # min_angle on either side of one track's exit pair
    ang = refs[0]["track_angle"][j]
    assert st[4][1] < float(ang.v) < st[3][1] and st[3][1] - st[4][1] < 10 * float(ang.e) + 1e-15
    assert abs(ang.v - LD(st[3][1])) >= 4 * ang.e > 0 and abs(ang.v - LD(st[4][1])) >= 4 * ang.e
    assert refs[4]["track_angle"].v[j] == ang.v and refs[3]["track_angle"].v[j] != ang.v                  # below: the same exit; above: the pair no longer exits
    # the depths moved to 1e-3 -+ 1e-12 and 1e3 -+ 1e-6
    want = ((1, 1e-3, -1e-12), (0, 1e-3, 1e-12), (0, 1e3, -1e-6), (1, 1e3, 1e-6))
    for (o, pt, target), (deleted, thr, off) in zip(near["moved"], want):
        Z = refs[0]["Z"][o]
        assert arr["obs_pt"][o] == pt and abs(float(Z.v - LD(F64(thr))) - off) < 0.01 * abs(off)
        assert abs(Z.v - LD(F64(thr))) >= 4 * Z.e > 0 and refs[0]["obs_delete"][o] == deleted
        assert not refs[0]["facts"]["by_re"][o]                                                           # the depth alone decides


# ---------------------------------------------------------------------------------------------------- exact thresholds
def _per_observation64(arr):
    out = []
    with np.errstate(all="ignore"):
        for c, j, uv in zip(arr["obs_cam"], arr["obs_pt"], arr["obs_uv"]):
            u, v, Z = Y.project64(*FC._cam_of(arr, c), arr["points"][j])
            out.append((np.sqrt((u - uv[0]) * (u - uv[0]) + (v - uv[1]) * (v - uv[1])), Z))
    return np.array(out)


def test_exact_cases_are_the_hand_written_numbers_bit_for_bit():
    arr = FC.case("exact")
    f64 = _per_observation64(arr)
    for k, want in enumerate(FC.EXACT_EXPECT):
        ref = FC.reference("exact", k)
        assert np.asarray(FC.EXACT_Z, F64).tobytes() == f64[:, 1].tobytes() == np.asarray(ref["Z"].v, F64).tobytes()
        assert (ref["Z"].v == np.asarray(FC.EXACT_Z, LD)).all()
        idx = list(FC.EXACT_RE5)
        assert (f64[idx, 0] == 5.0).all() and (ref["re"].v[idx] == LD(5)).all()
        with np.errstate(all="ignore"):
            runs = (ref, Y.restate64(arr, *FC.settings("exact")[k]), bo.filter_tracks(H.to_oracle(arr), *FC.settings("exact")[k]))
        for got in runs:
            for key, value in want.items():
                assert np.asarray(got[key]).tolist() == value, (k, key)
    assert FC.RE_EXACT == (5.0, 4.999999999999999) and F64(1e-3) == FC.EXACT_Z[0] and FC.EXACT_Z[2] == 0.0009999999999999998 and FC.EXACT_Z[6] == 1000.0000000000001
    assert math.isnan(f64[12, 0]) and math.isnan(f64[13, 0])                 # Z = 0: 0 / 0, and 1 / 0 beside 0 / 0: re compares false, the depth deletes


def test_the_exact_angle_meets_its_threshold_in_float64():
    """the first pair's float64 operand is 1 - 2^-52 and its angle the threshold itself, here; the long-double angle lies below it, and
    the yardstick carries the pair as [0, bar]: it does not exit, whichever value float64 gives"""
    arr = FC.case("exact_angle")
    c = [FC.centre64(arr["cam_q"][i], arr["cam_t"][i]) for i in range(3)]
    stats = dict(den_zero=0, arg_above_1=0, arg_is_1=0, fold=0)
    assert Y._angle64(c[0], c[1], arr["points"][0], (), stats) == FC.ANGLE_EXACT == 2.1073424255447017e-08
    assert 0 < LD(FC.ANGLE_EXACT) - np.arccos(1 - LD(2) ** -52) < LD(2.0) ** -79                         # 0.32 ulp of the threshold
    a, f = Y.tri_angles(*(Y.V(x[None]) for x in (c[0], c[1], arr["points"][0])), np.zeros(1, bool))
    assert f["beyond"][0] and a.v[0] == 0 and FC.ANGLE_EXACT < a.e[0] < 1e-7          # the operand's interval reaches 1: [0, bar], no exit either
    ref = FC.reference("exact_angle", 0)
    assert ref["facts"]["exit_kind"][0] == "later" and ref["track_outlier"][0] == 0 and abs(float(ref["track_angle"].v[0]) - math.atan(0.125)) < 1e-15


# ---------------------------------------------------------------------------------------------------- coverage
WANTED = {
    "scene_kitti": ("by_re_alone", "by_zmin_alone", "by_zmax_alone", "outlier_1", "outlier_2", "exit_first", "exit_later", "exit_none", "len_2", "len_3", "len_5"),
    "scene_models": ("model_0", "model_1", "model_2", "model_3", "model_4", "by_re_alone", "by_zmin_alone", "by_zmax_alone", "outlier_1", "outlier_2"),
    "lengths": ("len_0", "len_1", "len_2", "len_3", "len_5", "len_33", "len_65", "len_130", "pair_one_deleted", "triple_n_minus_2_kept", "triple_n_minus_1_dropped",
                "all_deleted", "fold", "exit_none", "gap_tracks", "last_camera_observed"),
    **{f"points_{n}": ("last_camera_observed",) for n in FC.N_POINTS},
    **{f"cams_{n}": ("last_camera_observed",) for n in FC.N_CAMS},
    "points_129": ("more_than_one_block_of_tracks",), "points_257": ("more_than_one_block_of_tracks",), "cams_257": ("more_than_one_block_of_cameras", "last_camera_observed"),
    "order_base": ("gap_tracks", "outlier_1", "outlier_2"), "order_shuffled": ("unsorted_obs", "gap_tracks"), "order_relabel": ("gap_tracks",),
    "exits": ("exit_first", "exit_later", "exit_below_max", "exit_none"),
    "shared_centre": ("f64_exactly_1", "exit_none", "exit_later"),
    "degenerate": ("den_zero", "fold", "beyond_1", "f64_above_1"),
    "exact": ("by_zmin_alone", "by_zmax_alone", "by_re_alone", "model_0", "f64_exactly_1"),
    "exact_angle": ("exit_later",),
    "near": ("by_zmin_alone", "by_zmax_alone"),
    "nonfinite": ("nan_track",),
}


def test_every_item_of_the_catalogue_occurs():
    table = {name: FC.coverage(name) for name in FC.NAMES}
    print("%-15s %s" % ("", " ".join(r[:7] for r in FC.ROWS)))
    for name in FC.NAMES:
        print("%-15s %s" % (name, " ".join("%7d" % table[name][r] for r in FC.ROWS)))
    for name, rows in WANTED.items():
        for row in rows:
            assert table[name][row] > 0, (name, row)
    assert [r for r in FC.ROWS if not any(table[n][r] for n in FC.NAMES)] == []
    assert sorted(FC.case(f"points_{n}")["points"].shape[0] for n in FC.N_POINTS) == list(FC.N_POINTS)
    assert sorted(FC.case(f"cams_{n}")["cam_q"].shape[0] for n in FC.N_CAMS) == list(FC.N_CAMS)
    assert max(FC.case(n)["points"].shape[0] for n in FC.NAMES) <= 300
    # the hand-built tracks are what their names say, at the mapper's setting
    L, r = FC.LENGTHS, FC.reference("lengths", 0)
    n, nd, out = r["facts"]["n"], r["facts"]["ndel"], r["track_outlier"]
    assert n.tolist() == [0, 1, 2, 2, 3, 3, 3, 3, 5, 33, 65, 130, 0, 2] and nd.tolist() == [0, 0, 0, 1, 0, 1, 2, 3, 0, 0, 0, 0, 0, 0]
    assert out.tolist() == [0, 1, 0, 1, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0] and r["num_filtered"].tolist() == [1 + 2 + 1 + 3 + 3, 0]
    for j in (L["empty"], L["empty_last_but_one"], L["single"], L["pair_one_deleted"], L["triple_n_minus_1"], L["triple_all"]):
        assert r["track_error"].v[j] == -1 and r["track_angle"].v[j] == -1 and r["track_error"].e[j] == 0
    assert r["track_error"].v[L["triple_n_minus_2"]] > 0
    E, r = FC.EXIT, FC.reference("exits", 0)
    kinds, f = r["facts"]["exit_kind"], r["facts"]
    assert [kinds[j] for j in range(5)] == ["first", "later", "none", "later", "later"] and f["below_max"].tolist() == [False, True, False, False, False]
    assert f["pairs"].tolist() == [1, 2, 3, 3, 2] and r["track_outlier"].tolist() == [0, 0, 2, 0, 0]
    S = FC.SHARED
    r0, r1 = FC.reference("shared_centre", 0), FC.reference("shared_centre", 1)
    assert r0["track_outlier"].tolist() == [2, 0] and r1["track_outlier"].tolist() == [0, 0]                  # min_angle = 0: kept, angle 0
    assert r0["track_angle"].v[S["alone"]] == 0 and r0["track_angle"].e[S["alone"]] == 0 and r1["track_angle"].v[S["alone"]] == 0
    assert r0["facts"]["pairs"][S["with_third"]] == 2
    D, r = FC.DEGENERATE, FC.reference("degenerate", 0)
    assert r["facts"]["den_zero"].tolist() == [True, False, False] and r["facts"]["pairs"][D["on_centre"]] == 3 and r["track_outlier"].tolist() == [0, 0, 2]
    assert r["Z"].v[0] == 4 and r["re"].v[0] == 0 and r["facts"]["fold"][D["obtuse"]] and r["facts"]["beyond"][D["above_one"]]
    assert 0 < r["track_angle"].e[D["above_one"]] < 1e-6 and r["track_angle"].v[D["above_one"]] == 0
    # the non-finite track: nothing deleted, error NaN, angle 0, outlier 2 unless min_angle = 0
    j = FC.NAN_TRACK
    for k, outlier in ((0, 2), (1, 0)):
        r = FC.reference("nonfinite", k)
        sel = FC.case("nonfinite")["obs_pt"] == j
        assert sel.sum() == 3 and not r["obs_delete"][sel].any() and np.isnan(r["track_error"].v[j]) and r["track_angle"].v[j] == 0 and r["track_outlier"][j] == outlier


def test_the_order_cases_are_one_problem():
    base = FC.case("order_base")
    for name in ("order_shuffled", "order_relabel"):
        arr = FC.case(name)
        om, pm = FC.ORDER_MAPS[name]
        assert np.array_equal(arr["points"], base["points"][pm], equal_nan=True) and np.array_equal(arr["obs_uv"], base["obs_uv"][om])
        assert np.array_equal(arr["obs_cam"], base["obs_cam"][om]) and np.array_equal(pm[arr["obs_pt"]], base["obs_pt"][om])
        assert sorted(om.tolist()) == list(range(len(om))) and not np.array_equal(om, np.arange(len(om)))
        # the yardstick's outputs are the base's, permuted, bit for bit
        a, b = FC.reference(name, 0), FC.reference("order_base", 0)
        assert np.array_equal(a["obs_delete"], b["obs_delete"][om]) and np.array_equal(a["track_outlier"], b["track_outlier"][pm])
        assert (a["track_angle"].v == b["track_angle"].v[pm]).all() and a["num_filtered"].tolist() == b["num_filtered"].tolist()


# ---------------------------------------------------------------------------------------------------- mutations
CAUGHT_BY = dict(re_ge="exact", zmin_le="exact", zmax_le="exact", ndel_ge_n="lengths", count_ndel="lengths", mean_over_n="lengths", single_focal="scene_models",
                 max_all_pairs="exits", exit_ge="exact_angle", outlier_le="shared_centre", reversed_pairs="exits", no_fold="degenerate", centre_M_t="exits", clamp_z="near",
                 no_scatter="order_shuffled")
FAILS_ON = dict(re_ge={"obs_delete", "track_outlier", "num_filtered", "track_error", "track_angle"}, zmin_le={"obs_delete"}, zmax_le={"obs_delete"},
                ndel_ge_n={"track_outlier"}, count_ndel={"num_filtered"}, mean_over_n={"track_error"}, single_focal={"obs_delete"}, max_all_pairs={"track_angle"},
                exit_ge={"track_angle"}, outlier_le={"track_outlier", "num_filtered"}, reversed_pairs={"track_angle"}, no_fold={"track_angle"}, centre_M_t={"track_angle"},
                clamp_z={"obs_delete"}, no_scatter={"obs_delete"})


@pytest.mark.parametrize("mutation", Y.MUTATIONS)
def test_every_mutated_restatement_fails_the_checker(mutation):
    assert set(CAUGHT_BY) == set(Y.MUTATIONS) == set(FAILS_ON)
    name = CAUGHT_BY[mutation]
    failed = set()
    for k, s in enumerate(FC.settings(name)):
        with np.errstate(all="ignore"):
            failed |= set(Y.failures(Y.check(FC.reference(name, k), Y.restate64(FC.case(name), *s, mut=(mutation,)))))
    print(mutation, name, sorted(failed))
    assert failed >= FAILS_ON[mutation]
