"""Device-resident frame sets without a GPU: the exports, every EINVAL of every entry before a device is needed with
one line on stderr and untouched outputs, the empty set, ENODEV for real work, ba_frames_rule.h on the host as a stand-alone program
built with the address and undefined-behaviour sanitizers, the premises of the verification scenes of tests/test_gpu_frames.py, and
the register / scratch figures of the two kernels."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import frames_cases as FC
from tests import frames_host_driver as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("xrsfm_ba_frames_create", "xrsfm_ba_frames_from_images", "xrsfm_ba_frames_info", "xrsfm_ba_frames_download", "xrsfm_ba_frames_match",
         "xrsfm_ba_frames_destroy")
SENTINEL = 0x5A5A5A5A
p = lambda a, t: a.ctypes.data_as(C.POINTER(t)) if a is not None else None


def _one_line(err, name):
    return err.count("\n") == 1 and name in err


def test_the_new_symbols_are_declared_and_exported(lib):
    from xrsfm_amd import capi
    hdr = open(os.path.join(ROOT, "include", "xrsfm_ba.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in capi.EXPORTS and getattr(lib, name) is not None, name
    for word in ("immutable", "one thread at a time", "xrsfm_ba_quiesce does not free"):
        assert word in hdr, word


def _empty_frames(lib, n_frames=3):
    """a set of n_frames frames without key points: needs no device"""
    h = C.c_void_p()
    ptr = np.zeros(n_frames + 1, np.int64)
    assert lib.xrsfm_ba_frames_create(n_frames, p(ptr, C.c_int64), None, None, C.byref(h)) == 0 and h.value
    return h


def test_create_refuses_bad_arguments_before_a_device_is_needed(lib, capfd):
    from xrsfm_amd import capi
    keys = np.zeros((4, 4), np.float32); desc = np.zeros((4, 128), np.uint8)
    bad_keys = keys.copy(); bad_keys[2, 1] = np.inf
    ptr = lambda *v: np.array(v, np.int64)
    cases = [(-1, ptr(0), keys, desc), (2, None, keys, desc), (2, ptr(1, 2, 4), keys, desc), (2, ptr(0, 3, 2), keys, desc), (2, ptr(0, 2, 4), None, desc),
             (2, ptr(0, 2, 4), keys, None), (2, ptr(0, 2, 4), bad_keys, desc)]
    for n, kp, k, d in cases:
        h = C.c_void_p(SENTINEL)
        capfd.readouterr()
        code = lib.xrsfm_ba_frames_create(n, p(kp, C.c_int64), p(k, C.c_float), p(d, C.c_uint8), C.byref(h))
        assert code == capi.EINVAL and _one_line(capfd.readouterr().err, "xrsfm_ba_frames_create") and h.value == SENTINEL, (n, kp)
    capfd.readouterr()
    assert lib.xrsfm_ba_frames_create(0, None, None, None, None) == capi.EINVAL and _one_line(capfd.readouterr().err, "xrsfm_ba_frames_create")


def test_from_images_refuses_bad_arguments_before_a_device_is_needed(lib, capfd):
    from xrsfm_amd import capi
    img = np.zeros((20, 24), np.uint8)
    w, h, ptr = np.array([24], np.int32), np.array([20], np.int32), np.array([0, 480], np.int64)
    o, do = capi.sift_options(), capi.sift_desc_options()

    def run(o=o, do=do, n=1, w=w, h=h, ptr=ptr, pix=img, out=True):
        hd = C.c_void_p(SENTINEL)
        capfd.readouterr()
        code = lib.xrsfm_ba_frames_from_images(C.byref(o) if o is not None else None, C.byref(do) if do is not None else None, n, p(w, C.c_int32), p(h, C.c_int32),
                                               p(ptr, C.c_int64), p(pix, C.c_uint8), C.byref(hd) if out else None)
        return code, capfd.readouterr().err, hd.value

    for kw in (dict(o=None), dict(do=None), dict(do=capi.sift_desc_options(upright=2)), dict(n=-1), dict(o=capi.sift_options(first_octave=1)),
               dict(o=capi.sift_options(num_octaves=9)), dict(o=capi.sift_options(peak_threshold=0.0)), dict(o=capi.sift_options(max_num_features=0)),
               dict(w=None), dict(pix=None), dict(ptr=np.array([1, 481], np.int64)), dict(ptr=np.array([0, 479], np.int64)), dict(w=np.array([12], np.int32), ptr=np.array([0, 240], np.int64)),
               dict(o=capi.sift_options(max_image_size=16)), dict(out=False)):
        code, err, hv = run(**kw)
        assert code == capi.EINVAL and _one_line(err, "xrsfm_ba_frames_from_images") and hv == SENTINEL, (kw, code, err)


def test_info_and_download_refuse_bad_arguments(lib, capfd):
    from xrsfm_amd import capi
    n = C.c_int32(-7)
    capfd.readouterr()
    assert lib.xrsfm_ba_frames_info(None, C.byref(n), None, None) == capi.EINVAL and _one_line(capfd.readouterr().err, "xrsfm_ba_frames_info") and n.value == -7
    assert lib.xrsfm_ba_frames_download(None, 0, None, None, None, None, None) == capi.EINVAL and _one_line(capfd.readouterr().err, "xrsfm_ba_frames_download")
    h = _empty_frames(lib)
    try:
        loc = np.full((1, 4), -77, np.int32); sign = np.full(1, -77, np.int8); lc = np.full(12, -77, np.int32)
        for args in ((0, None, None, p(loc, C.c_int32), None, None), (0, None, None, None, p(sign, C.c_int8), None), (0, None, None, None, None, p(lc, C.c_int32)),
                     (-1, None, None, None, None, None)):
            capfd.readouterr()
            assert lib.xrsfm_ba_frames_download(h, *args) == capi.EINVAL and _one_line(capfd.readouterr().err, "xrsfm_ba_frames_download"), args
        assert np.all(loc == -77) and np.all(sign == -77) and np.all(lc == -77)
        assert lib.xrsfm_ba_frames_download(h, 0, None, None, None, None, None) == 0
    finally:
        lib.xrsfm_ba_frames_destroy(h)
    lib.xrsfm_ba_frames_destroy(None)


class _Match:
    """one xrsfm_ba_frames_match call on a set of three frames without key points, every output at a fill value"""

    def __init__(self, n_pairs=2):
        self.pa = np.array([0, 1][:n_pairs], np.int32); self.pb = np.array([1, 2][:n_pairs], np.int32)
        self.n = n_pairs
        self.fill()

    def fill(self):
        n = max(self.n, 1)
        self.out = dict(mp=np.full(n + 1, -77, np.int64), m=np.full((4, 2), -77, np.int32), nr=np.full(n, -77, np.int32), nc=np.full(n, -77, np.int32),
                        st=np.full(n, 77, np.uint8), F=np.full((n, 9), -77.0), mask=np.full(4, 77, np.uint8), ni=np.full(n, -77, np.int32), nt=np.full(n, -77, np.int32),
                        bt=np.full(n, -77, np.int32), acc=np.full(n, 77, np.uint8))

    def untouched(self):
        return all(np.all(v == (77 if v.dtype == np.uint8 else -77)) for v in self.out.values())

    def run(self, lib, h, mo, vo, null=(), n_pairs=None, pa="own", pb="own", pme=None, psd=None, cap=4, verify_out=None):
        self.fill()
        o = {k: (None if k in null else v) for k, v in self.out.items()}
        with_v = (vo is not None) if verify_out is None else verify_out
        v = lambda k, t: p(o[k], t) if with_v else None
        return lib.xrsfm_ba_frames_match(h, C.byref(mo) if mo is not None else None, C.byref(vo) if vo is not None else None, self.n if n_pairs is None else n_pairs,
                                         p(self.pa if isinstance(pa, str) else pa, C.c_int32), p(self.pb if isinstance(pb, str) else pb, C.c_int32), p(pme, C.c_double), p(psd, C.c_uint32),
                                         cap, p(o["mp"], C.c_int64), p(o["m"], C.c_int32), p(o["nr"], C.c_int32), p(o["nc"], C.c_int32), v("st", C.c_uint8),
                                         v("F", C.c_double), v("mask", C.c_uint8), v("ni", C.c_int32), v("nt", C.c_int32), v("bt", C.c_int32), v("acc", C.c_uint8))


def test_match_refuses_bad_arguments_before_a_device_is_needed(lib, capfd):
    from xrsfm_amd import capi
    h = _empty_frames(lib)
    mo, vo = capi.match_options, capi.verify_pairs_options
    c = _Match()
    i32 = lambda *v: np.array(v, np.int32)
    cases = [dict(h=None, mo=mo(), vo=None), dict(mo=None, vo=None), dict(mo=mo(), vo=None, n_pairs=-1), dict(mo=mo(), vo=None, cap=-1),
             dict(mo=mo(max_distance=0.0), vo=None), dict(mo=mo(max_distance=float("nan")), vo=None), dict(mo=mo(max_ratio=1.5), vo=None),
             dict(mo=mo(max_features=0), vo=None), dict(mo=mo(max_features=16385), vo=None),
             dict(mo=mo(), vo=vo(max_error=0.0)), dict(mo=mo(), vo=vo(confidence=1.5)), dict(mo=mo(), vo=vo(min_inlier_ratio=-0.1)),
             dict(mo=mo(), vo=vo(max_num_trials=0)), dict(mo=mo(), vo=vo(max_num_trials=16385)), dict(mo=mo(), vo=vo(min_num_trials=200, max_num_trials=100)),
             dict(mo=mo(), vo=vo(min_matches=6)), dict(mo=mo(), vo=vo(min_num_inliers=-1)), dict(mo=mo(), vo=vo(min_accept_ratio=-1.0)),
             dict(mo=mo(), vo=vo(max_error=float("inf"))),
             dict(mo=mo(), vo=None, verify_out=True),                                  # verification outputs without options
             dict(mo=mo(), vo=None, null=("mp",)), dict(mo=mo(), vo=None, pa=None), dict(mo=mo(), vo=None, pb=None),
             dict(mo=mo(), vo=None, pa=i32(0, 3)), dict(mo=mo(), vo=None, pb=i32(-1, 2)), dict(mo=mo(), vo=None, null=("m",)),
             dict(mo=mo(), vo=vo(), null=("st",)), dict(mo=mo(), vo=vo(), null=("F",)), dict(mo=mo(), vo=vo(), null=("mask",)),
             dict(mo=mo(), vo=vo(), pme=np.array([4.0, 0.0])), dict(mo=mo(), vo=vo(), pme=np.array([np.nan, 1.0]))]
    try:
        for kw in cases:
            kw = dict(kw)
            hh = kw.pop("h", h)
            capfd.readouterr()
            code = c.run(lib, hh, **kw)
            err = capfd.readouterr().err
            assert code == capi.EINVAL and _one_line(err, "xrsfm_ba_frames_match") and c.untouched(), (kw, code, err)
        # a single verification output without options is refused as well
        for k in ("st", "F", "mask", "ni", "nt", "bt", "acc"):
            capfd.readouterr()
            code = c.run(lib, h, mo(), None, verify_out=True, null=tuple(x for x in ("st", "F", "mask", "ni", "nt", "bt", "acc") if x != k))
            assert code == capi.EINVAL and _one_line(capfd.readouterr().err, "xrsfm_ba_frames_match") and c.untouched(), k
    finally:
        lib.xrsfm_ba_frames_destroy(h)


def test_the_empty_set(lib):
    from xrsfm_amd import capi
    with capi.frames_create(np.zeros(1, np.int64), np.zeros((0, 4), np.float32), np.zeros((0, 128), np.uint8)) as fs:
        info = capi.frames_info(fs)
        assert info["n_frames"] == 0 and info["key_ptr"].tolist() == [0] and info["device_bytes"] == 0
        assert capi.frames_download(fs) == []
        for vo in (None, capi.verify_pairs_options()):
            r = capi.frames_match(fs, [], [], capi.match_options(), vo)
            assert r["match_ptr"].tolist() == [0] and r["matches"].shape == (0, 2) and len(r["num_row"]) == 0
            if vo is not None:
                assert len(r["status"]) == 0 and len(r["inlier_mask"]) == 0 and r["F"].shape == (0, 9)
        c = _Match(0)
        assert c.run(lib, fs.handle, capi.match_options(), capi.verify_pairs_options()) == 0 and c.untouched()
    assert fs.handle is None
    fs.close()                                                     # twice is fine
    with pytest.raises(RuntimeError, match="closed"):
        capi.frames_info(fs)
    with capi.frames_from_images([]) as fi:
        assert capi.frames_info(fi)["n_frames"] == 0 and capi.frames_download(fi) == []


def test_real_work_without_a_device_is_enodev(lib):
    import torch
    from xrsfm_amd import capi
    if torch.cuda.is_available() and capi.device_count() > 0:
        pytest.skip("a GPU is present")
    h = C.c_void_p(SENTINEL)
    ptr = np.array([0, 2], np.int64); keys = np.zeros((2, 4), np.float32); desc = np.zeros((2, 128), np.uint8)
    assert lib.xrsfm_ba_frames_create(1, p(ptr, C.c_int64), p(keys, C.c_float), p(desc, C.c_uint8), C.byref(h)) == -2 and h.value == SENTINEL
    with pytest.raises(RuntimeError, match="ENODEV"):
        capi.frames_create(ptr, keys, desc)
    with pytest.raises(RuntimeError, match="ENODEV"):
        capi.frames_from_images([np.zeros((20, 24), np.uint8)])
    hh = _empty_frames(lib)
    try:
        c = _Match()
        assert c.run(lib, hh, capi.match_options(), None) == -2 and c.untouched()
        assert c.run(lib, hh, capi.match_options(), capi.verify_pairs_options()) == -2 and c.untouched()
    finally:
        lib.xrsfm_ba_frames_destroy(hh)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return H.build(tmp_path_factory.mktemp("frames_rule"))


@pytest.mark.parametrize("n", (1, 2, 63, 64, 65, 300))
def test_rank_rule_is_the_argsort_of_the_codes(driver, n):
    """segments in shuffled emission order: the ranks scatter the key points into the order of row * width + col"""
    rng = np.random.default_rng(100 + n)
    width = 52
    cells = rng.permutation(width * 40)[:n]                       # distinct samples of a 52 x 40 level, in the order of emission
    rows, cols = cells // width, cells % width
    rank = np.array(H.run(driver, H.rank_input(rows.tolist(), cols.tolist(), width))[0].split(), np.int64)
    code = rows.astype(np.int64) * width + cols
    assert sorted(rank.tolist()) == list(range(n))
    order = np.empty(n, np.int64); order[rank] = np.arange(n)       # order[r]: the key point that lands at r
    assert np.array_equal(order, np.argsort(code, kind="stable"))


def _check_plan(batches, clip, pa, pb, counts, strip):
    live = [k for k in range(len(pa)) if clip[pa[k]] > 0 and clip[pb[k]] > 0]
    seen = []
    at = 0
    for b in batches:
        assert b["first"] == at and b["last"] > b["first"]             # consecutive, none empty
        at = b["last"]
        rows = cols = parts = items = beg = 0
        for (q, row, col, part, item, strips, g) in b["pairs"]:
            na, nb = clip[pa[q]], clip[pb[q]]
            assert (row, col, part, item, g) == (rows, cols, parts, items, beg) and strips == -(-na // strip)       # each begins where the last ended
            rows += na; cols += nb; parts += strips * nb; items += strips; beg += counts[q]
            seen.append(q)
        assert b["size"] == (len(b["pairs"]), rows, cols, parts, items)
    assert seen == live and at == len(live)
    return batches


def test_plan_covers_every_pair_once(driver):
    clip = [0, 5, 129, 257, 0, 64]
    pa = [1, 2, 2, 0, 3, 5, 4, 3, 1]
    pb = [2, 2, 3, 1, 4, 3, 4, 3, 5]                                # a == b twice, an empty frame on either side and on both
    counts = [min(clip[a], clip[b]) // 2 for a, b in zip(pa, pb)]
    big = _check_plan(H.parse_plan(H.run(driver, H.plan_input(clip, pa, pb, counts, 128, 1 << 40))[0]), clip, pa, pb, counts, 128)
    assert len(big) == 1
    one = _check_plan(H.parse_plan(H.run(driver, H.plan_input(clip, pa, pb, counts, 128, 0))[0]), clip, pa, pb, counts, 128)
    assert all(len(b["pairs"]) == 1 for b in one) and len(one) == 6
    mid = _check_plan(H.parse_plan(H.run(driver, H.plan_input(clip, pa, pb, counts, 128, 20000))[0]), clip, pa, pb, counts, 128)
    assert 1 < len(mid) < 6
    assert H.run(driver, H.plan_input([0, 0], [0], [1], [0], 128, 0))[0].strip() == "live"          # nothing to do


def test_accept_threshold(driver):
    for mn, ratio, n in ((15, 0.25, 24), (15, 0.25, 600), (15, 0.25, 61), (0, 0.999, 1000), (7, 0.0, 5)):
        assert int(H.run(driver, "accept %d %r %d\n" % (mn, ratio, n))[0]) == max(mn, int(ratio * n))


@pytest.mark.parametrize("size", FC.SIZES[:3])
def test_the_scenes_give_what_the_gpu_test_asserts(size):
    """24/9 and 40/17: as many matches as related key points, status 1 with every match an inlier in float64 on the float32-rounded
    points; 12/5: 12 matches, below min_matches"""
    from tests import fund_yardstick as YF
    from tests import match_yardstick as Y
    s = FC.scene(*size)
    m = Y.run_pair(s["desc_a"], s["desc_b"])["matches"]
    assert len(m) == size[0]
    inv = np.argsort(s["perm"])
    assert all(j == inv[i] for i, j in m.tolist())
    xa, xb = s["kp_a"][m[:, 0]].astype(np.float64), s["kp_b"][m[:, 1]].astype(np.float64)
    r = YF.run_pair(xa, xb, dtype=np.float64)
    if size[0] < 15:
        assert r["status"] == 2
    else:
        assert r["status"] == 1 and r["num_inliers"] == size[0] and r["accepted"] == 1


def test_frames_kernels_do_not_spill(tmp_path):
    """k_frames_order and k_frames_gather of the gfx950 code object: no spilled register, no private (scratch) segment"""
    from xrsfm_amd import _build
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = tmp_path / "frames_only.hip"
    src.write_text('#include <hip/hip_runtime.h>\n#include "ba_frames.h"\n')
    asm = tmp_path / "frames.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-I", _build.CSRC, str(src), "-o", str(asm)], check=True, capture_output=True)
    seen = {}
    for blk in asm.read_text().split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        m = re.search(r"k_frames_(order|gather)", name)
        if not m:
            continue
        num = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, blk).group(1))
        fig = dict(vgpr=num("vgpr_count"), sgpr=num("sgpr_count"), lds=num("group_segment_fixed_size"), scratch=num("private_segment_fixed_size"), spill=num("vgpr_spill_count"))
        seen[m.group(1)] = fig
        assert fig["spill"] == 0 and fig["scratch"] == 0 and fig["vgpr"] <= 128, (name, fig)
    print("frame set kernels:", seen)
    assert sorted(seen) == ["gather", "order"]
    assert seen["order"]["lds"] == 256 * 8 + 256 * 4 and seen["gather"]["lds"] == 0
