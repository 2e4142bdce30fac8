"""xrsfm_ba_extract_features on the GPU against tests/desc_yardstick.py: gradient, orientation, descriptor sums, normalisation and
bytes, each stage on the device's own inputs; the identity with xrsfm_ba_detect_keypoints; the independence from
batching, order, repetition and the workspace split; the capacity error; the budget; images to matches end to end; rotation.

Shapes: those of tests/test_gpu_sift.py, for the reasons given there."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import desc_yardstick as D
from tests import sift_yardstick as Y

pytestmark = pytest.mark.gpu

CASES = (("a44x40", -1), ("b50x33", 0), ("c64x48", -1), ("c64x48", 0), ("e300x260", -1))
BATCH = ("a44x40", "b50x33", "c64x48", "d64x48", "e300x260")
FIELDS = ("keys", "loc", "sign", "level_count", "desc", "desc_float")
_cache = {}


def _opt(fo, **kw):
    from xrsfm_amd import capi
    return capi.sift_options(first_octave=fo, **kw)


def _dopt(upright):
    from xrsfm_amd import capi
    return capi.sift_desc_options(upright=upright)


def _alone(name, fo, upright=0):
    from xrsfm_amd import capi
    key = (name, fo, upright)
    if key not in _cache:
        _cache[key] = capi.extract_features([Y.image(name)], _opt(fo), _dopt(upright))[0]
    return _cache[key]


def _same(a, b, fields=FIELDS):
    return all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in fields)


@pytest.mark.parametrize("name,fo", CASES)
def test_gradient_planes_within_the_operation_count(lib, name, fo):
    """stage A: (grd, rot) of G[1..3] of every octave against longdouble from the levels debug_sift_levels returns"""
    from xrsfm_amd import capi
    for o in range(len(capi.sift_geometry(Y.image(name).shape[1], Y.image(name).shape[0], _opt(fo)))):
        G, _ = capi.debug_sift_levels(Y.image(name), o, _opt(fo))
        wg, wr = D.check_gradient(G[1:4], capi.debug_sift_gradient(Y.image(name), o, _opt(fo)))
        print(name, fo, "octave", o, "worst ratio to the bar: grd %.3f rot %.3f" % (wg, wr))
        assert wg <= 1.0 and wr <= 1.0, (o, wg, wr)


@pytest.mark.parametrize("upright", (0, 1))
@pytest.mark.parametrize("name,fo", CASES)
def test_stages_on_the_devices_own_inputs(lib, name, fo, upright):
    """stages B, C and D through debug_sift_describe, and extract_features = debug_sift_describe + the mirror, byte for byte"""
    from xrsfm_amd import capi
    img = Y.image(name)
    st = capi.debug_sift_describe(img, _opt(fo), _dopt(upright))
    got = _alone(name, fo, upright)
    det = capi.detect_keypoints([img], _opt(fo))[0]
    assert np.array_equal(st["loc"], got["loc"]) and len(st["loc"]) > 0
    assert _same(got, det, ("loc", "sign", "level_count")) and np.array_equal(got["keys"][:, :3].view(np.uint32), det["keys"][:, :3].view(np.uint32))
    planes = [capi.debug_sift_gradient(img, o, _opt(fo)) for o in range(len(capi.sift_geometry(img.shape[1], img.shape[0], _opt(fo))))]
    loc3, off = capi.debug_sift_offsets(img, _opt(fo))
    assert np.array_equal(loc3, st["loc"])
    assert np.array_equal(D.octave_keys(st["loc"], off[:, 1:], fo)[:, :2], st["okeys"][:, :2])          # x, y: additions only
    assert np.abs(D.octave_keys(st["loc"], off[:, 1:], fo)[:, 2] - st["okeys"][:, 2]).max() <= 4 * D.EPS * st["okeys"][:, 2].max()          # one powf, one product
    if upright:
        assert np.all(st["okeys"][:, 3] == 0) and np.all(got["keys"][:, 3] == 0)
    else:
        r = D.check_orientation(planes, st["loc"], st["okeys"])
        print(name, fo, "orientation: fragile", r["fragile"], "compared", r["compared"], "worst ratio to the 16x bar %.3f" % r["worst"], r["mismatch"][:5])
        assert r["mismatch"] == [] and r["worst"] <= 1.0 and r["fragile"] <= 0.05 * len(st["loc"]), r
        assert np.array_equal(got["keys"][:, 3].view(np.uint32), D.mirror(st["okeys"][:, 3]).view(np.uint32))
        assert np.all((got["keys"][:, 3] >= 0) & (got["keys"][:, 3] < np.float32(2 * np.pi)))
    worst, dropped = D.check_descriptor(planes, st["loc"], st["okeys"], st["raw"])
    print(name, fo, "upright", upright, "descriptor sums: worst ratio to the 16x bar %.3f, dropped samples %d" % (worst, dropped))
    assert worst <= 1.0
    n = D.check_normalisation(st["raw"], st["unit"], got["desc_float"], got["desc"])
    print(name, fo, "upright", upright, "normalisation", n, "fragile share %.4f" % (n["fragile"] / n["total"]))
    assert n["unit"] <= 1.0 and n["floats"] <= 1.0 and n["wrong"] == 0 and n["fragile"] <= 0.05 * n["total"], n
    # the bytes are those of the float rows, and without the float rows they are the same bytes
    assert np.array_equal(got["desc"], D.to_bytes(got["desc_float"]))
    assert np.array_equal(capi.extract_features([img], _opt(fo), _dopt(upright), floats=False)[0]["desc"], got["desc"])


def test_alone_in_the_batch_reversed_twice_and_in_chunks_are_bit_identical(lib):
    from xrsfm_amd import capi
    imgs = [Y.image(k) for k in BATCH]
    one = capi.extract_features(imgs, _opt(-1), _dopt(0))
    two = capi.extract_features(imgs, _opt(-1), _dopt(0))
    rev = capi.extract_features(imgs[::-1], _opt(-1), _dopt(0))[::-1]
    det = capi.detect_keypoints(imgs, _opt(-1))
    old = os.environ.get("XRSFM_BA_SIFT_WORKSPACE_MB")
    try:
        os.environ["XRSFM_BA_SIFT_WORKSPACE_MB"] = "0"
        split = capi.extract_features(imgs, _opt(-1), _dopt(0))
        os.environ["XRSFM_BA_SIFT_WORKSPACE_MB"] = "1"          # a budget between: some images share a chunk
        mixed = capi.extract_features(imgs, _opt(-1), _dopt(0))
    finally:
        if old is None:
            del os.environ["XRSFM_BA_SIFT_WORKSPACE_MB"]
        else:
            os.environ["XRSFM_BA_SIFT_WORKSPACE_MB"] = old
    for k, name in enumerate(BATCH):
        for other in (two, rev, split, mixed):
            assert _same(one[k], other[k]), name
        assert _same(one[k], det[k], ("loc", "sign", "level_count")) and np.array_equal(one[k]["keys"][:, :3].view(np.uint32), det[k]["keys"][:, :3].view(np.uint32))
        assert _same(one[k], _alone(name, -1)), name
    assert sum(len(r["loc"]) for r in one) > 1000


def test_small_capacity_is_einval_with_counts_written(lib, capfd):
    from xrsfm_amd import capi
    imgs = [np.ascontiguousarray(Y.image(k)) for k in ("a44x40", "c64x48")]
    want = [_alone("a44x40", -1), _alone("c64x48", -1)]
    n = [len(w["loc"]) for w in want]
    cap = n[0] + n[1] - 1
    w = np.array([a.shape[1] for a in imgs], np.int32); h = np.array([a.shape[0] for a in imgs], np.int32)
    ptr = np.array([0, imgs[0].size, imgs[0].size + imgs[1].size], np.int64)
    pix = np.concatenate([a.ravel() for a in imgs])
    kp = np.full(3, -77, np.int64); keys = np.full((cap, 4), -77, np.float32); loc = np.full((cap, 4), -77, np.int32); sign = np.full(cap, -77, np.int8)
    desc = np.full((cap, 128), 77, np.uint8); fl = np.full((cap, 128), -77, np.float32); lc = np.full((2, 12), -77, np.int32)
    p = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    o, do = _opt(-1), _dopt(0)
    capfd.readouterr()
    code = lib.xrsfm_ba_extract_features(C.byref(o), C.byref(do), 2, p(w, C.c_int32), p(h, C.c_int32), p(ptr, C.c_int64), p(pix, C.c_uint8), cap, p(kp, C.c_int64),
                                         p(keys, C.c_float), p(loc, C.c_int32), p(sign, C.c_int8), p(desc, C.c_uint8), p(fl, C.c_float), p(lc, C.c_int32))
    err = capfd.readouterr().err
    assert code == capi.EINVAL and str(n[0] + n[1]) in err and err.count("\n") == 1
    assert kp.tolist() == [0, n[0], n[0] + n[1]] and np.array_equal(lc[0], want[0]["level_count"]) and np.array_equal(lc[1], want[1]["level_count"])
    assert np.all(keys == -77) and np.all(loc == -77) and np.all(sign == -77) and np.all(desc == 77) and np.all(fl == -77)


def test_budget_cut_returns_the_rows_of_the_full_call(lib):
    from xrsfm_amd import capi
    full = _alone("d64x48", -1)
    got = capi.extract_features([Y.image("d64x48")], _opt(-1, max_num_features=20), _dopt(0))[0]
    take, total = Y.budget(got["level_count"], 3, 20)
    keep = take[3 * full["loc"][:, 0] + full["loc"][:, 1]]
    assert not take.all() and len(got["loc"]) == total == int(keep.sum()) and 0 < total < len(full["loc"])
    for k in ("keys", "loc", "sign", "desc", "desc_float"):
        assert np.array_equal(got[k].view(np.uint8), full[k][keep].view(np.uint8)), k


def test_images_to_matches_end_to_end(lib, tmp_path):
    """Y.translated(8, 8) and Y.translated(12, 12) through extract_features -> feature_frames -> match_descriptors at default options
    -> matched_points.  Among the eligible interior keypoints of the translation test of test_gpu_sift.py, with the margin grown by
    the descriptor's footprint, no match links a keypoint to anything but its shifted counterpart, and the correct matches number at
    least 0.9 of those the host program's descriptors yield through tests/match_yardstick.py on the CPU."""
    from xrsfm_amd import capi
    from tests import desc_cases as K
    imgs = K.e2e_images()
    res = capi.extract_features(imgs, _opt(-1), _dopt(0))
    desc, dptr, xy = capi.feature_frames(res)
    pa, pb = np.array([0], np.int32), np.array([1], np.int32)
    m = capi.match_descriptors(dptr, desc, pa, pb)
    xa, xb = capi.matched_points(m, dptr, xy, pa, pb)[:2]
    correct, wrong = K.count_matches(res[0]["loc"], res[1]["loc"], res[0]["keys"], res[1]["keys"], m["matches"])
    ref, ref_wrong = K.e2e_comparator(tmp_path)
    print("end to end: matches", len(m["matches"]), "among the eligible: correct", correct, "wrong", wrong, "comparator: correct", ref, "wrong", ref_wrong)
    assert len(xa) == len(xb) == len(m["matches"])
    assert ref >= 20 and wrong == 0 and correct >= 0.9 * ref, (correct, wrong, ref)


def test_rotation_by_a_quarter_turn(lib):
    """a 64 x 64 image and its np.rot90, an exact permutation of the pixels: interior keypoints found in both, loc mapped by the
    rotation, have orientations that differ by pi / 2 within the stage-B bar plus the measured deviation that the two gradient planes
    cause; with upright both are 0"""
    from xrsfm_amd import capi
    from tests import desc_cases as K
    a, b = K.rotation_images()
    ra, rb = (capi.debug_sift_describe(x, _opt(0), _dopt(0)) for x in (a, b))
    pairs = K.rotation_pairs(ra["loc"], rb["loc"], 0)
    bar = 16 * D.measured_deviation()["w"] + K.rotation_plane_deviation()
    worst = 0.0
    for i, j in pairs:
        worst = max(worst, K.quarter_turn_error(ra["okeys"][i, 3], rb["okeys"][j, 3]))
    print("rotation: pairs", len(pairs), "worst deviation from a quarter turn %.3e bar %.3e" % (worst, bar))
    assert len(pairs) >= 10 and worst <= bar
    for x in (a, b):
        u = capi.extract_features([x], _opt(0), _dopt(1))[0]
        assert len(u["keys"]) > 0 and np.all(u["keys"][:, 3] == 0)
