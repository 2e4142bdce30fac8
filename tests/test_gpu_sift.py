"""xrsfm_ba_detect_keypoints on the GPU against tests/sift_yardstick.py: the levels of every octave within the bars, the keypoints
(key / no key and sign on every non-fragile pixel, offsets and values within 16 times the float32 restatement's own deviation),
the budget, the independence from batching, order, repetition and the workspace split, the capacity error and translation.

Shapes: 44 x 40 at first_octave -1 (stored widths 88, 44, 24: the down-sample clamp and the stored-width border act, and the widest
filter is wider than the last octave), 50 x 33 at first_octave 0 (width truncated to 48, odd height), 64 x 48 in both modes, and
300 x 260, which has at least two 64 x 32 tiles in each dimension of every kernel in all four octaves (76 x 65 in the last)."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import sift_yardstick as Y

pytestmark = pytest.mark.gpu

CASES = (("a44x40", -1), ("b50x33", 0), ("c64x48", -1), ("c64x48", 0), ("e300x260", -1))
BATCH = ("a44x40", "b50x33", "c64x48", "d64x48", "e300x260")
_cache = {}


def _opt(fo, **kw):
    from xrsfm_amd import capi
    return capi.sift_options(first_octave=fo, **kw)


def _alone(name, fo):
    """detect_keypoints and debug_sift_offsets of one image alone, once"""
    from xrsfm_amd import capi
    if (name, fo) not in _cache:
        r = capi.detect_keypoints([Y.image(name)], _opt(fo))[0]
        loc, off = capi.debug_sift_offsets(Y.image(name), _opt(fo))
        assert np.array_equal(loc, r["loc"]) and np.array_equal(off[:, 0].astype(np.int8), r["sign"])
        r["off"] = off
        _cache[(name, fo)] = r
    return _cache[(name, fo)]


def _same(a, b):
    return all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in ("keys", "loc", "sign", "level_count"))


@pytest.mark.parametrize("name,fo", CASES)
def test_levels_of_every_octave_within_the_bars(lib, name, fo):
    from xrsfm_amd import capi
    ref = Y.catalogue_reference(name, True, fo)
    assert capi.sift_geometry(Y.image(name).shape[1], Y.image(name).shape[0], _opt(fo)) == ref["geometry"]
    for o, ((Gr, Dr), (gb, db)) in enumerate(zip(ref["pyramid"], ref["bars"])):
        G, D = capi.debug_sift_levels(Y.image(name), o, _opt(fo))
        assert G.shape == Gr.shape and D.shape == Dr.shape
        for i in range(6):
            dev = float(np.abs(G[i].astype(np.longdouble) - Gr[i]).max())
            print(name, fo, "octave", o, "G", i, "deviation %.3e bar %.3e" % (dev, gb[i]))
            assert dev <= gb[i], (o, i, dev, gb[i])
        for j in range(5):
            dev = float(np.abs(D[j].astype(np.longdouble) - Dr[j]).max())
            print(name, fo, "octave", o, "D", j, "deviation %.3e bar %.3e" % (dev, db[j]))
            assert dev <= db[j], (o, j, dev, db[j])


def test_keys_against_the_yardstick(lib):
    """key / no key and sign on every non-fragile pixel, level_count, key_ptr, loc and sign exactly where no fragile pixel is
    involved, offsets and (X, Y, S) within 16 times the restatement's own deviation; at most 5 % of the union fragile"""
    union = fragile = compared = 0
    for name, fo in CASES:
        ref, got = Y.catalogue_reference(name, True, fo), _alone(name, fo)
        assert ref["take"][:3 * len(ref["pyramid"])].all()
        mism, u, f = Y.compare(Y.levels_of(got["loc"], got["sign"]), ref)
        print(name, fo, "keypoints", len(got["loc"]), "yardstick", len(ref["loc"]), "union", u, "fragile", f, "mismatches", mism[:5])
        assert mism == [], (name, fo, mism[:5])
        union, fragile = union + u, fragile + f
        for (o, j), r in ref["levels"].items():
            nf = int(r["fragile"].sum())
            assert abs(int(got["level_count"][3 * o + j]) - int(ref["level_count"][3 * o + j])) <= nf
            if nf == 0:
                k = (ref["loc"][:, 0] == o) & (ref["loc"][:, 1] == j)
                kg = (got["loc"][:, 0] == o) & (got["loc"][:, 1] == j)
                assert np.array_equal(got["loc"][kg], ref["loc"][k]) and np.array_equal(got["sign"][kg], ref["sign"][k]), (name, fo, o, j)
        assert np.all(got["level_count"][3 * len(ref["pyramid"]):] == 0) and len(got["loc"]) == int(got["level_count"].sum())
        order = np.lexsort((got["loc"][:, 3], got["loc"][:, 2], got["loc"][:, 1], got["loc"][:, 0]))
        assert np.array_equal(order, np.arange(len(order))) and np.all(got["keys"][:, 3] == 0)
        n, worst = Y.check_values(got["loc"], got["off"][:, 1:], got["keys"], ref)
        print(name, fo, "values compared", n, "worst ratio to the 16x bar %.3f" % worst)
        assert worst <= 1.0, (name, fo, worst)
        compared += n
    assert union >= 1000 and compared >= 1000 and fragile <= 0.05 * union, (union, fragile)


def test_budget_cuts_whole_levels_and_overshoots(lib):
    from xrsfm_amd import capi
    full = _alone("d64x48", -1)
    for budget, name in ((20, "budget20"), (60, "budget60")):
        ref = Y.catalogue_reference(name)
        got = capi.detect_keypoints([Y.image("d64x48")], _opt(-1, max_num_features=budget))[0]
        assert np.array_equal(got["level_count"], full["level_count"])
        take, total = Y.budget(got["level_count"], 3, budget)
        assert take.tolist() == ref["take"].tolist() and not take.all() and total > budget
        keep = take[3 * full["loc"][:, 0] + full["loc"][:, 1]]
        assert len(got["loc"]) == total == int(keep.sum())
        for k in ("keys", "loc", "sign"):
            assert np.array_equal(got[k], full[k][keep])


def test_alone_in_the_batch_reversed_and_twice_are_bit_identical(lib):
    from xrsfm_amd import capi
    for fo in (-1, 0):
        imgs = [Y.image(k) for k in BATCH]
        one = capi.detect_keypoints(imgs, _opt(fo))
        two = capi.detect_keypoints(imgs, _opt(fo))
        rev = capi.detect_keypoints(imgs[::-1], _opt(fo))[::-1]
        for k, name in enumerate(BATCH):
            assert _same(one[k], two[k]) and _same(one[k], rev[k]), (name, fo)
            if (name, fo) in CASES or name == "d64x48":
                assert _same(one[k], _alone(name, fo)), (name, fo)
        assert _same(one[0], capi.detect_keypoints([imgs[0]], _opt(fo))[0])
        assert sum(len(r["loc"]) for r in one) > 200


def test_one_image_per_chunk_is_bit_identical(lib):
    from xrsfm_amd import capi
    imgs = [Y.image(k) for k in BATCH]
    whole = capi.detect_keypoints(imgs, _opt(-1))
    old = os.environ.get("XRSFM_BA_SIFT_WORKSPACE_MB")
    os.environ["XRSFM_BA_SIFT_WORKSPACE_MB"] = "0"
    try:
        split = capi.detect_keypoints(imgs, _opt(-1))
        os.environ["XRSFM_BA_SIFT_WORKSPACE_MB"] = "1"          # a budget between: some images share a chunk
        mixed = capi.detect_keypoints(imgs, _opt(-1))
    finally:
        if old is None:
            del os.environ["XRSFM_BA_SIFT_WORKSPACE_MB"]
        else:
            os.environ["XRSFM_BA_SIFT_WORKSPACE_MB"] = old
    for a, b, c in zip(whole, split, mixed):
        assert _same(a, b) and _same(a, c)


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
    lc = np.full((2, 12), -77, np.int32)
    p = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    o = _opt(-1)
    capfd.readouterr()
    code = lib.xrsfm_ba_detect_keypoints(C.byref(o), 2, p(w, C.c_int32), p(h, C.c_int32), p(ptr, C.c_int64), p(pix, C.c_uint8), cap, p(kp, C.c_int64), p(keys, C.c_float),
                                         p(loc, C.c_int32), p(sign, C.c_int8), p(lc, C.c_int32))
    err = capfd.readouterr().err
    assert code == capi.EINVAL and str(n[0] + n[1]) in err and err.count("\n") == 1
    assert kp.tolist() == [0, n[0], n[0] + n[1]] and np.array_equal(lc[0], want[0]["level_count"]) and np.array_equal(lc[1], want[1]["level_count"])
    assert np.all(keys == -77) and np.all(loc == -77) and np.all(sign == -77)
    code = lib.xrsfm_ba_detect_keypoints(C.byref(o), 2, p(w, C.c_int32), p(h, C.c_int32), p(ptr, C.c_int64), p(pix, C.c_uint8), cap, p(kp, C.c_int64), p(keys, C.c_float),
                                         p(loc, C.c_int32), p(sign, C.c_int8), None)
    assert code == capi.EINVAL


def test_translation_by_a_multiple_of_the_coarsest_pixel(lib):
    """the 64 x 48 content at (8, 8) and at (12, 12) of a 96 x 80 canvas: 8 pixels of the first octave, 1 of the fourth.  A keypoint
    farther from every border, in both, than the summed filter reach appears in both with bit-identical offsets and shifted loc"""
    from xrsfm_amd import capi
    la, oa = capi.debug_sift_offsets(Y.translated(8, 8), _opt(-1))
    lb, ob = capi.debug_sift_offsets(Y.translated(12, 12), _opt(-1))
    geo, reach = Y.geometry(96, 80, -1, 4), Y.filter_reach(-1, 4)
    assert len(geo) == 4
    b_at = {tuple(l): k for k, l in enumerate(lb.tolist())}
    eligible = 0
    for k, (o, j, r, c) in enumerate(la.tolist()):
        s, (w, h) = 8 >> o, geo[o]
        if min(r, c) <= reach[o] or r + s >= h - 1 - reach[o] or c + s >= w - 1 - reach[o]:
            continue
        eligible += 1
        q = b_at.get((o, j, r + s, c + s))
        assert q is not None, (o, j, r, c)
        assert np.array_equal(oa[k].view(np.uint32), ob[q].view(np.uint32)), (o, j, r, c, oa[k], ob[q])
    print("translation: eligible keypoints", eligible, "of", len(la))
    assert eligible >= 4
