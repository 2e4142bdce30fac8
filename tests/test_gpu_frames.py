"""Device-resident frame sets on the GPU.  Every comparison is np.array_equal on the raw bits against the chain of
existing entry points extract_features -> feature_frames -> match_descriptors -> matched_points -> verify_pairs, run in the same
process: the set changes where the data lives, never a bit of it.

Shapes: the catalogue frames of tests/match_yardstick.py (up to 1200 descriptors, several strips), the scenes of
tests/frames_cases.py (the largest 857 key points a frame), the images of tests/test_gpu_desc.py (the largest spans several tiles a
level and more than one work item of 256 key points in a level)."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import frames_cases as FC
from tests import match_yardstick as Y
from tests import sift_yardstick as YS

pytestmark = pytest.mark.gpu

BATCH = ("a44x40", "b50x33", "c64x48", "d64x48", "e300x260")
MATCH_KEYS = ("match_ptr", "matches", "num_row", "num_col")
VERIFY_KEYS = ("status", "F", "inlier_mask", "num_inliers", "num_trials", "best_trial", "accepted")
IMAGE_FIELDS = ("keys", "loc", "sign", "desc", "level_count")


def _capi():
    from xrsfm_amd import capi
    return capi


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same(got, want, keys):
    return [k for k in keys if got[k].shape != want[k].shape or got[k].dtype != want[k].dtype or not np.array_equal(_bits(got[k]), _bits(want[k]))]


class _env:
    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        self.old = os.environ.get(self.name)
        os.environ[self.name] = self.value

    def __exit__(self, *exc):
        if self.old is None:
            del os.environ[self.name]
        else:
            os.environ[self.name] = self.old


def _chain(ptr, keys, desc, pa, pb, mo=None, vo=None, pme=None, psd=None):
    """the existing entry points on host arrays: match_descriptors, matched_points, verify_pairs"""
    capi = _capi()
    r = capi.match_descriptors(ptr, desc, pa, pb, mo)
    if vo is not None:
        xa, xb = capi.matched_points(r, ptr, keys[:, :2], pa, pb)
        r.update(capi.verify_pairs(r["match_ptr"].astype(np.int32), xa, xb, vo, pme, psd))
    return r


# ---------------------------------------------------------------------------------------------------- feature sets (no images)
TAGS = ("shape_129x257", "shape_65x64", "shape_0x17", "shape_257x257", "shape_1x1", "shapeT_129x257", "self_129", "strips_1000x1200", "strips_300x129", "edge_300x131",
        "all255_20x20", "zero_rows_66x70", "tie_row", "tie_col", "clip100", "clip100_T", "ab", "ba")


@pytest.fixture(scope="module")
def catalogue_set(lib):
    capi = _capi()
    ptr, desc, _, _ = Y.call_arrays([])
    rng = np.random.default_rng(2026)
    keys = np.ascontiguousarray(rng.uniform(0, 1280, (len(desc), 4)).astype(np.float32))
    fs = capi.frames_create(ptr, keys, desc)
    yield fs, ptr, keys, desc
    fs.close()


def _entries(tags):
    E = Y.entries()
    ks = [next(k for k, e in enumerate(E) if e["tag"] == t) for t in tags]
    return Y.call_arrays(ks)[2:]


@pytest.mark.parametrize("max_features", (16384, 100))
def test_matching_on_a_set_equals_match_descriptors(catalogue_set, max_features):
    """default options, and max_features below the size of most frames: the clip happens at match time, the set stores every row"""
    capi = _capi()
    fs, ptr, keys, desc = catalogue_set
    pa, pb = _entries(TAGS)
    mo = capi.match_options(max_features=max_features)
    got, want = capi.frames_match(fs, pa, pb, mo), capi.match_descriptors(ptr, desc, pa, pb, mo)
    assert _same(got, want, MATCH_KEYS) == [] and len(want["matches"]) > (500 if max_features > 100 else 100)
    assert "status" not in got
    if max_features == 100:
        assert want["matches"].max() < 100 and np.diff(ptr)[pa].max() > 100


def test_a_created_set_downloads_what_it_was_given(catalogue_set):
    capi = _capi()
    fs, ptr, keys, desc = catalogue_set
    info = capi.frames_info(fs)
    assert info["n_frames"] == len(ptr) - 1 and np.array_equal(info["key_ptr"], ptr) and info["device_bytes"] >= 148 * len(desc)
    rows = capi.frames_download(fs)
    assert np.array_equal(_bits(np.concatenate([r["keys"] for r in rows])), _bits(keys)) and np.array_equal(np.concatenate([r["desc"] for r in rows]), desc)
    assert "loc" not in rows[0]


# ---------------------------------------------------------------------------------------------------- verification
@pytest.fixture(scope="module")
def scene_set(lib):
    capi = _capi()
    ptr, keys, desc = FC.scene_set()
    fs = capi.frames_create(ptr, keys, desc)
    yield fs, ptr, keys, desc
    fs.close()


@pytest.fixture(scope="module")
def scene_chain(scene_set):
    _, ptr, keys, desc = scene_set
    return _chain(ptr, keys, desc, FC.PAIR_A, FC.PAIR_B, _capi().match_options(), _capi().verify_pairs_options(), FC.PAIR_MAX_ERROR, FC.PAIR_SEED)


def test_match_gather_verify_in_one_call_equals_the_chain(scene_set, scene_chain):
    capi = _capi()
    fs = scene_set[0]
    got = capi.frames_match(fs, FC.PAIR_A, FC.PAIR_B, capi.match_options(), capi.verify_pairs_options(), FC.PAIR_MAX_ERROR, FC.PAIR_SEED)
    want = scene_chain
    assert _same(got, want, MATCH_KEYS + VERIFY_KEYS) == []
    n = np.diff(want["match_ptr"])
    print("matches", n.tolist(), "status", want["status"].tolist(), "accepted", want["accepted"].tolist(), "inliers", want["num_inliers"].tolist())
    assert n[:3].tolist() == [24, 40, 12] and n[3] >= 590 and n[5] == n[6] == 0
    assert want["status"][[0, 1, 3]].tolist() == [1, 1, 1] and want["accepted"][[0, 1, 3]].tolist() == [1, 1, 1]
    assert want["status"][2] == 2 and want["status"][5] == 2 and want["status"][6] == 2
    assert want["num_inliers"][0] == 24 and want["num_inliers"][1] == 40
    # verified_matches takes the dict as it takes that of verify_pairs
    kept, rows, new_ptr = capi.verified_matches(got, got["match_ptr"], got["matches"])
    kept2, rows2, new_ptr2 = capi.verified_matches(want, want["match_ptr"], want["matches"])
    assert np.array_equal(kept, kept2) and np.array_equal(rows, rows2) and np.array_equal(new_ptr, new_ptr2) and 0 in kept and 3 in kept and 2 not in kept


def test_two_calls_on_one_set_equal_two_chain_calls(scene_set):
    capi = _capi()
    fs, ptr, keys, desc = scene_set
    for sel in ([0, 2, 4, 7], [1, 3, 5, 8, 6]):
        pa, pb, pme, psd = FC.PAIR_A[sel], FC.PAIR_B[sel], FC.PAIR_MAX_ERROR[sel], FC.PAIR_SEED[sel]
        got = capi.frames_match(fs, pa, pb, capi.match_options(), capi.verify_pairs_options(), pme, psd)
        want = _chain(ptr, keys, desc, pa, pb, capi.match_options(), capi.verify_pairs_options(), pme, psd)
        assert _same(got, want, MATCH_KEYS + VERIFY_KEYS) == [], sel


def _pair_of(r, p):
    a, b = int(r["match_ptr"][p]), int(r["match_ptr"][p + 1])
    out = [r["matches"][a:b], r["inlier_mask"][a:b]] + [r[k][p:p + 1] for k in ("num_row", "num_col", "status", "F", "num_inliers", "num_trials", "best_trial", "accepted")]
    return b"".join(_bits(x).tobytes() for x in out)


def test_a_pair_alone_in_the_batch_reversed_and_in_sub_batches_is_bit_identical(scene_set, scene_chain):
    capi = _capi()
    fs = scene_set[0]
    mo, vo = capi.match_options(), capi.verify_pairs_options()
    n = len(FC.PAIR_A)
    rev = capi.frames_match(fs, FC.PAIR_A[::-1], FC.PAIR_B[::-1], mo, vo, FC.PAIR_MAX_ERROR[::-1], FC.PAIR_SEED[::-1])
    with _env("XRSFM_BA_MATCH_WORKSPACE_MB", "0"):
        split = capi.frames_match(fs, FC.PAIR_A, FC.PAIR_B, mo, vo, FC.PAIR_MAX_ERROR, FC.PAIR_SEED)
        split_m = capi.frames_match(fs, FC.PAIR_A, FC.PAIR_B, mo)
    assert _same(split, scene_chain, MATCH_KEYS + VERIFY_KEYS) == [] and _same(split_m, scene_chain, MATCH_KEYS) == []
    for p in (0, 1, 2, 4, 5, 7, 8):
        alone = capi.frames_match(fs, FC.PAIR_A[p:p + 1], FC.PAIR_B[p:p + 1], mo, vo, FC.PAIR_MAX_ERROR[p:p + 1], FC.PAIR_SEED[p:p + 1])
        assert _pair_of(alone, 0) == _pair_of(scene_chain, p) == _pair_of(rev, n - 1 - p), p


# ---------------------------------------------------------------------------------------------------- image sets
def _sopt(**kw):
    return _capi().sift_options(first_octave=-1, **kw)


def _rows_equal(got, want):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert _same(g, w, IMAGE_FIELDS) == [], k


@pytest.mark.parametrize("upright", (0, 1))
def test_image_set_downloads_what_extract_features_returns(lib, upright):
    capi = _capi()
    imgs = [YS.image(k) for k in BATCH]
    do = capi.sift_desc_options(upright=upright)
    want = capi.extract_features(imgs, _sopt(), do, floats=False)
    with capi.frames_from_images(imgs, _sopt(), do) as fs:
        info = capi.frames_info(fs)
        kp = np.concatenate([[0], np.cumsum([len(w["loc"]) for w in want])])
        assert np.array_equal(info["key_ptr"], kp) and info["device_bytes"] >= 169 * kp[-1] and kp[-1] > 1000
        _rows_equal(capi.frames_download(fs), want)
    assert max(int(w["level_count"].max()) for w in want) > 256          # a level of more than one work item
    if upright == 0:
        with capi.frames_from_images(imgs[::-1], _sopt(), do) as fs:
            _rows_equal(capi.frames_download(fs)[::-1], want)
        for mb in ("0", "1"):                                          # every image a chunk; some images share a chunk: the set grows
            with _env("XRSFM_BA_SIFT_WORKSPACE_MB", mb):
                with capi.frames_from_images(imgs, _sopt(), do) as fs:
                    _rows_equal(capi.frames_download(fs), want)


def test_image_set_under_a_budget_that_cuts_levels(lib):
    capi = _capi()
    img = [YS.image("d64x48")]
    want = capi.extract_features(img, _sopt(max_num_features=20), floats=False)
    full = capi.extract_features(img, _sopt(), floats=False)
    assert 0 < len(want[0]["loc"]) < len(full[0]["loc"])
    with capi.frames_from_images(img, _sopt(max_num_features=20)) as fs:
        _rows_equal(capi.frames_download(fs), want)


def test_images_to_verified_pairs_end_to_end(lib):
    """desc_cases.e2e_images (a pure translation: no assertion about acceptance) through frames_from_images -> frames_match with
    verification, against the chain on host arrays"""
    capi = _capi()
    from tests import desc_cases as K
    imgs = K.e2e_images()
    res = capi.extract_features(imgs, _sopt(), floats=False)
    desc, dptr, xy = capi.feature_frames(res)
    pa, pb = np.array([0, 1], np.int32), np.array([1, 0], np.int32)
    want = _chain(dptr, xy, desc, pa, pb, capi.match_options(), capi.verify_pairs_options())
    with capi.frames_from_images(imgs, _sopt()) as fs:
        got = capi.frames_match(fs, pa, pb, capi.match_options(), capi.verify_pairs_options())
    assert _same(got, want, MATCH_KEYS + VERIFY_KEYS) == [] and len(want["matches"]) >= 20


# ---------------------------------------------------------------------------------------------------- capacity, untouched outputs, lifetime
def test_capacity_one_below_the_need_is_einval_with_untouched_outputs(lib, scene_set, scene_chain, capfd):
    capi = _capi()
    fs = scene_set[0]
    need, n = len(scene_chain["matches"]), len(FC.PAIR_A)
    p = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    mo, vo = capi.match_options(), capi.verify_pairs_options()

    def call(cap, verify=True, verify_out=True):
        o = dict(mp=np.full(n + 1, -77, np.int64), m=np.full((need, 2), -77, np.int32), nr=np.full(n, -77, np.int32), nc=np.full(n, -77, np.int32),
                 st=np.full(n, 77, np.uint8), F=np.full((n, 9), -77.0), mask=np.full(need, 77, np.uint8), ni=np.full(n, -77, np.int32), nt=np.full(n, -77, np.int32),
                 bt=np.full(n, -77, np.int32), acc=np.full(n, 77, np.uint8))
        v = lambda k, t: p(o[k], t) if verify_out else None
        capfd.readouterr()
        code = lib.xrsfm_ba_frames_match(fs.handle, C.byref(mo), C.byref(vo) if verify else None, n, p(FC.PAIR_A, C.c_int32), p(FC.PAIR_B, C.c_int32),
                                         p(FC.PAIR_MAX_ERROR, C.c_double) if verify else None, p(FC.PAIR_SEED, C.c_uint32) if verify else None, cap, p(o["mp"], C.c_int64),
                                         p(o["m"], C.c_int32), p(o["nr"], C.c_int32), p(o["nc"], C.c_int32), v("st", C.c_uint8), v("F", C.c_double), v("mask", C.c_uint8),
                                         v("ni", C.c_int32), v("nt", C.c_int32), v("bt", C.c_int32), v("acc", C.c_uint8))
        return code, capfd.readouterr().err, o, all(np.all(a == (77 if a.dtype == np.uint8 else -77)) for a in o.values())

    for verify in (True, False):
        code, err, _, untouched = call(need - 1, verify, verify)
        assert code == capi.EINVAL and str(need) in err and err.count("\n") == 1 and "xrsfm_ba_frames_match" in err and untouched, (verify, code, err)
    code, err, _, untouched = call(need, False, True)                      # verification outputs without options
    assert code == capi.EINVAL and err.count("\n") == 1 and untouched
    code, err, o, _ = call(need)
    assert code == 0 and err == ""
    assert np.array_equal(o["mp"], scene_chain["match_ptr"]) and np.array_equal(o["m"], scene_chain["matches"]) and np.array_equal(o["mask"], scene_chain["inlier_mask"])
    ok = scene_chain["status"] == 1                                          # (the C call leaves F of the other pairs untouched)
    assert np.array_equal(_bits(o["F"][ok]), _bits(scene_chain["F"][ok])) and np.all(o["F"][~ok] == -77.0)
    for k, name in (("st", "status"), ("ni", "num_inliers"), ("nt", "num_trials"), ("bt", "best_trial"), ("acc", "accepted"), ("nr", "num_row"), ("nc", "num_col")):
        assert np.array_equal(o[k], scene_chain[name]), name


def test_create_destroy_create_again(lib):
    capi = _capi()
    ptr, keys, desc = FC.scene_set()
    pa, pb = FC.PAIR_A[:2], FC.PAIR_B[:2]
    first = None
    for _ in range(2):
        fs = capi.frames_create(ptr, keys, desc)
        info = capi.frames_info(fs)
        assert info["device_bytes"] > 0 and np.array_equal(info["key_ptr"], ptr) and info["n_frames"] == 9
        r = capi.frames_match(fs, pa, pb, capi.match_options(), capi.verify_pairs_options())
        fs.close()
        assert fs.handle is None
        if first is None:
            first = r
        assert _same(r, first, MATCH_KEYS + VERIFY_KEYS) == []
    capi.quiesce()
    with capi.frames_create(ptr, keys, desc) as fs:                       # after the cache has been emptied
        assert _same(capi.frames_match(fs, pa, pb, capi.match_options(), capi.verify_pairs_options()), first, MATCH_KEYS + VERIFY_KEYS) == []
