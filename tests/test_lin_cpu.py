"""The linearisation yardstick without a GPU (tests/lin_yardstick.py).

(i) The catalogue contains what it claims, asserted from the packing the library reports (capi.debug_pack / debug_pack_gram /
debug_sgroup): every (C, T, dense | ragged) tile cell, every reduction branch of linearize_item, long items of 2, 3 and 4 tiles, all
camera models, the constant masks, the hand-placed edge observations on the intended side of their threshold, the camera counts around
the grid of k_lin_tail and the partial counts around the group size of segsum_body.
(ii) No case holds a fragile observation (one whose clamp or Huber decision float64 could take either way).
(iii) The plain float64 restatement of the oracle's linearisation (bo.evaluate, bo._Linearization, the scalars of bo.solve) is inside
every bar on every case and both use_scaling settings: the bars, derived from operation counts, are wide enough for a correct float64
implementation.  The largest ratios are printed per family; tests/test_gpu_lin.py quotes them next to the kernels'."""
import numpy as np
import pytest

from tests import helpers as H
from tests import lin_yardstick as Y

_WORST = {}


@pytest.mark.parametrize("name", list(Y.CASES))
def test_float64_restatement_is_inside_every_bar(lib, name):
    arr = Y.case(name)
    for use_scaling in (False, True):
        ref = Y.case_reference(name, use_scaling)
        assert int(ref["fragile"].sum()) == 0, (name, np.nonzero(ref["fragile"])[0])
        w = Y.assert_inside(Y.check_all(ref, Y.float64_restatement(arr, use_scaling)), (name, use_scaling))
        fam = _WORST.setdefault(Y.family_of(name), {})
        for k, v in w.items():
            fam[k] = max(fam.get(k, 0.0), v[0])
        print(f"LIN64 {name} scaling={int(use_scaling)} fragile=0 " + " ".join(f"{k}={v[0]:.3g}" for k, v in w.items()))
    print(f"LIN64 family {Y.family_of(name)} so far: " + " ".join(f"{k}={v:.3g}" for k, v in _WORST[Y.family_of(name)].items()))


def test_shapes_cover_every_cell_and_branch(lib):
    """The 21 catalogue problems hold every (C, T, dense | ragged) cell (tests/test_gpu_hardening.py asserts that of the same
    problems) and, between them, regular tiles (strided_reduce), ragged Gram tiles (sorted LDS runs) and per-observation tiles."""
    assert len(Y.FAMILIES["shapes"]) == len(H.shape_problems()) == 21
    tot = {}
    for n in Y.FAMILIES["shapes"]:
        for k, v in Y.coverage(Y.case(n))["tiles"].items():
            tot[k] = tot.get(k, 0) + v
    assert tot["regular"] >= 50 and tot["gram_ragged"] >= 50 and tot["per_obs"] >= 20 and tot["long"] == 0, tot


def test_long_items(lib):
    tiles = set()
    for n in Y.FAMILIES["long"]:
        cov = Y.coverage(Y.case(n))
        assert cov["tiles"]["long"] > 0
        tiles |= cov["item_tiles"]
        want = [int(x) for x in n[4:].split("_")]
        assert set(want) <= cov["track_lens"] and max(cov["track_lens"]) == max(want)
    assert tiles >= {1, 2, 3, 4}


def test_models_and_consts(lib):
    cov = Y.coverage(Y.case("models"))
    assert cov["models"] == {0, 1, 2, 3, 4} and cov["tiles"]["gram_ragged"] > 0 and cov["tiles"]["per_obs"] > 0 and {1, 2, 3, 4, 5, 6} <= cov["track_lens"]
    b = Y.case("bal9_ragged")
    cov = Y.coverage(b)
    assert cov["models"] == {5} and len(cov["track_lens"] - {0}) > 2
    cc = np.asarray(b["cam_const"])
    assert ((cc & 4) == 0).sum() == 2 and ((cc & 4) != 0).sum() == 12 and (cc & 1).sum() == 1 and (np.asarray(b["point_const"]) != 0).any()
    arr = Y.case("consts")
    cov = Y.coverage(arr)
    assert cov["cam_const"] == {0, 1, 2, 3} and (cov["obs_per_cam"] == 0).sum() == 1
    lens = np.bincount(arr["obs_pt"], minlength=arr["points"].shape[0])
    pc = np.asarray(arr["point_const"]) != 0
    assert (lens == 0).sum() == 2 and (lens == 1).sum() >= 20 and (pc & (lens > 0)).sum() > 50 and (pc & (lens == 1)).any()
    assert int(Y.case_reference("consts", False)["clamped"].sum()) >= 20
    t = Y.case("consts_tfixed")
    assert ((np.asarray(t["cam_const"]) & 2) != 0).all()
    ref = Y.case_reference("consts_tfixed", True)
    assert 0 < float(ref["gradmax_cams"].v) <= 2.0          # a difference of unit quaternions: the quaternion part, nothing else


def test_edge_observations_sit_where_intended(lib):
    LD = Y.LD
    arr, marks = Y.edges()
    assert arr["cam_q"].shape[0] == 6
    ref = Y.reference(arr, False)
    assert int(ref["fragile"].sum()) == 0
    thr = LD(np.float64(Y.MIN_DEPTH))
    for z in Y.EDGE_DEPTHS:
        i = marks[f"depth_{z!r}"]
        rel = float((ref["Z"].v[i] - LD(z)) / LD(z))
        assert abs(rel) < 1e-12, (z, rel)
        assert bool(ref["clamped"][i]) == (z < Y.MIN_DEPTH)
        if abs(z / 1e-2 - 1) < 1e-8:
            d = float((ref["Z"].v[i] - thr) / thr)
            assert 0.9e-9 < abs(d) < 1.1e-9 and (d > 0) == (z > Y.MIN_DEPTH) and float(ref["Z"].e[i] / thr) < 1e-12, (z, d)
    b = LD(np.float64(Y.HUBER_A) * np.float64(Y.HUBER_A))
    for x in Y.EDGE_S:
        i = marks[f"s_{x!r}"]
        d = float((ref["s"].v[i] - b) / b)
        assert 0.9e-9 < abs(d) < 1.1e-9 and (d > 0) == (x > 1) == bool(ref["huber_out"][i]) and float(ref["s"].e[i] / b) < 1e-12, (x, d)
    for x in Y.EDGE_RES:
        i = marks[f"res_{x:g}"]
        assert abs(float(np.sqrt(ref["s"].v[i])) / x - 1) < 1e-9 and bool(ref["huber_out"][i])
    i = marks["zero"]
    assert float(ref["s"].v[i]) == 0.0 and not ref["clamped"][i]
    got = Y.float64_restatement(arr, False)
    assert (got["r"][i] == 0.0).all()
    # the translated copy: the same scene 1e5 away along every axis, five digits of M P + t cancel
    far, fmarks = Y.edges(near=False, shift=1e5)
    near = {f"depth_{z!r}" for z in Y.EDGE_DEPTHS[:2]} | {f"s_{x!r}" for x in Y.EDGE_S}
    assert set(fmarks) == set(marks) - near and len(near) == 4
    assert np.abs(far["points"]).min() > 9e4 and np.abs(far["cam_t"]).max() > 9e4
    rf = Y.reference(far, False)
    assert int(rf["fragile"].sum()) == 0
    # depth bar of an ordinary observation: five digits wider than at the origin
    i0, i1 = marks["res_10000"], fmarks["res_10000"]
    assert float(rf["Z"].e[i1] / ref["Z"].e[i0]) > 1e3


def test_camera_counts_and_partial_lists(lib):
    """k_lin_tail: grid min(1024, cameras), arrivals over 8 ticket counters, the camera loop beyond 1024 cameras; segsum_body:
    G = 21 (6-wide) / 14 (bal9) groups, four loads in flight."""
    assert [Y.case(f"band{n}")["cam_q"].shape[0] for n in Y.BAND] == list(Y.BAND) == [1, 7, 8, 9, 1023, 1024, 1025, 2049]
    for n in Y.BAND:
        arr = Y.case(f"band{n}")
        cov = Y.coverage(arr)
        assert cov["grid"] == min(n, 1024) and (cov["obs_per_cam"] > 0).all()
        assert cov["track_lens"] == ({2} if n > 1 else {1}) and arr["points"].shape[0] <= n + 5
    G6, G9 = 256 // 12, 256 // 18
    assert set(Y.PARTIALS6) >= {0, 1, 2, G6 - 1, G6, G6 + 1, 4 * G6 - 1, 4 * G6, 4 * G6 + 1, 300}
    assert set(Y.PARTIALS9) >= {G9 - 1, G9, G9 + 1, 4 * G9 - 1, 4 * G9, 4 * G9 + 1}
    for name, counts in (("cams_single", Y.PARTIALS6), ("bal9_cams_single", Y.PARTIALS9)):
        cov = Y.coverage(Y.case(name))
        assert cov["obs_per_cam"].tolist() == list(counts) and cov["track_lens"] == {1}
    for name, counts in (("cams_partials", Y.PARTIALS6), ("bal9_cams_partials", Y.PARTIALS9)):
        cov = Y.coverage(Y.case(name))
        k = len(counts)
        assert cov["obs_per_cam"][:k].tolist() == list(counts) and cov["partials"][:k].tolist() == list(counts), cov["partials"][:k]
        assert cov["tiles"]["per_obs"] > 0 and cov["tiles"]["regular"] == cov["tiles"]["gram_ragged"] == 0
    # the single-observation tracks of a 6-wide context fold into stride-1 regular tiles (one partial per camera and tile)
    cov = Y.coverage(Y.case("cams_single"))
    assert cov["tiles"]["regular"] >= 8 and cov["partials"].max() < 10
