"""xrsfm_ba_extract_features without a GPU: the interface (exports, struct layouts, every EINVAL with untouched outputs, the empty call,
ENODEV, the capi helpers), the yardstick's own checks (the float32 restatement within every bar and cap, the catalogue and the
hand-built cases cover what DESIGN.md 5n promises), ba_sift_desc_rule.h on the host as a stand-alone program built with the address
and undefined-behaviour sanitizers, the inputs of the end-to-end and rotation tests, and the kernels' register / LDS / scratch
figures."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import desc_cases as K
from tests import desc_host_driver as DH
from tests import desc_yardstick as D
from tests import sift_host_driver as H
from tests import sift_yardstick as Y

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NAMES = ("xrsfm_ba_sift_desc_options_default", "xrsfm_ba_extract_features", "xrsfm_ba_debug_sift_gradient", "xrsfm_ba_debug_sift_describe")


def test_exports_and_struct_layouts(lib, tmp_path):
    from xrsfm_amd import capi
    hdr = open(os.path.join(ROOT, "include", "xrsfm_ba.h")).read()
    for name in NAMES:
        assert name in capi.EXPORTS and getattr(lib, name) is not None and re.search(r"\b%s\s*\(" % name, hdr)
    src = tmp_path / "p.c"
    sf = [f for f, _ in capi.CSiftOptions._fields_]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "xrsfm_ba.h"\nint main(){printf("%zu %zu %zu", sizeof(xrsfm_ba_sift_desc_options), '
                   'offsetof(xrsfm_ba_sift_desc_options, upright), sizeof(xrsfm_ba_sift_options));\n' +
                   "".join('printf(" %%zu", offsetof(xrsfm_ba_sift_options, %s));\n' % f for f in sf) + 'printf("\\n");return 0;}\n')
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "p")], check=True)
    out = [int(x) for x in subprocess.run([str(tmp_path / "p")], capture_output=True, text=True, check=True).stdout.split()]
    assert out == [C.sizeof(capi.CSiftDescOptions), capi.CSiftDescOptions.upright.offset, C.sizeof(capi.CSiftOptions)] + [getattr(capi.CSiftOptions, f).offset for f in sf]
    assert out[:3] == [4, 0, 24]                           # (xrsfm_ba_sift_options keeps its layout)


def test_capi_helpers(lib):
    from xrsfm_amd import capi
    assert capi.sift_desc_options().upright == 0 and capi.sift_desc_options(upright=1).upright == 1
    with pytest.raises(AttributeError):
        capi.sift_desc_options(no_such_field=1)
    assert capi.extract_features([]) == []
    d, p, xy = capi.feature_frames([])
    assert d.shape == (0, 128) and p.tolist() == [0] and xy.shape == (0, 2)
    res = [dict(desc=np.full((2, 128), 3, np.uint8), keys=np.arange(8, dtype=F).reshape(2, 4)), dict(desc=np.zeros((0, 128), np.uint8), keys=np.zeros((0, 4), F)),
           dict(desc=np.full((1, 128), 9, np.uint8), keys=np.full((1, 4), 7, F))]
    d, p, xy = capi.feature_frames(res)
    assert d.dtype == np.uint8 and d.shape == (3, 128) and p.tolist() == [0, 2, 2, 3] and d[2, 0] == 9 and d.flags["C_CONTIGUOUS"]
    assert xy.tolist() == [[0, 1], [4, 5], [7, 7]]
    with pytest.raises(ValueError):
        capi.extract_features([np.zeros((20, 20), F)])
    with pytest.raises(ValueError):
        capi.debug_sift_gradient(np.zeros((40, 44), np.uint8), 3)


class _Call:
    """A small valid call and sentinel-filled outputs for the raw C entry."""
    def __init__(self):
        self.images = [np.ascontiguousarray(Y.image(k)) for k in ("a44x40", "b50x33")]
        self.n = 2
        self.w = np.array([a.shape[1] for a in self.images], np.int32)
        self.h = np.array([a.shape[0] for a in self.images], np.int32)
        self.ptr = np.zeros(3, np.int64)
        self.ptr[1:] = np.cumsum([a.size for a in self.images])
        self.pix = np.concatenate([a.ravel() for a in self.images])
        self.cap = 500
        self.out = dict(kp=np.full(3, -77, np.int64), k=np.full((500, 4), -77, F), l=np.full((500, 4), -77, np.int32), s=np.full(500, -77, np.int8),
                        d=np.full((500, 128), 77, np.uint8), f=np.full((500, 128), -77, F), lc=np.full((2, 12), -77, np.int32))

    def untouched(self):
        return all(np.all(v == (77 if k == "d" else -77)) for k, v in self.out.items())

    def run(self, lib, opt, dopt, null=()):
        p = lambda a, t: a.ctypes.data_as(C.POINTER(t))
        o = self.out
        a = dict(opt=C.byref(opt) if opt is not None else None, dopt=C.byref(dopt) if dopt is not None else None, w=p(self.w, C.c_int32), h=p(self.h, C.c_int32),
                 ptr=p(self.ptr, C.c_int64), pix=p(self.pix, C.c_uint8), kp=p(o["kp"], C.c_int64), k=p(o["k"], C.c_float), l=p(o["l"], C.c_int32), s=p(o["s"], C.c_int8),
                 d=p(o["d"], C.c_uint8), f=p(o["f"], C.c_float), lc=p(o["lc"], C.c_int32))
        for k in null:
            a[k] = None
        return lib.xrsfm_ba_extract_features(a["opt"], a["dopt"], self.n, a["w"], a["h"], a["ptr"], a["pix"], self.cap, a["kp"], a["k"], a["l"], a["s"], a["d"], a["f"], a["lc"])


def _einval_cases():
    def opt(**kw):
        return lambda c, o, d: [setattr(o, k, v) for k, v in kw.items()]

    def dopt(**kw):
        return lambda c, o, d: [setattr(d, k, v) for k, v in kw.items()]

    def field(name, fn):
        return lambda c, o, d: fn(getattr(c, name))
    return {
        "null_opt": "opt", "null_dopt": "dopt", "null_width": ("w",), "null_height": ("h",), "null_pixel_ptr": ("ptr",), "null_pixels": ("pix",), "null_key_ptr": ("kp",),
        "null_keys": ("k",), "null_loc": ("l",), "null_sign": ("s",), "null_desc": ("d",),
        "upright_two": dopt(upright=2), "upright_negative": dopt(upright=-1),
        "negative_images": lambda c, o, d: setattr(c, "n", -1), "negative_capacity": lambda c, o, d: setattr(c, "cap", -1),
        "width_truncates_below_16": field("w", lambda w: w.__setitem__(0, 19)), "height_below_16": field("h", lambda h: h.__setitem__(1, 15)),
        "side_above_max": opt(max_image_size=49), "ptr_not_from_zero": field("ptr", lambda p: p.__setitem__(0, 1)),
        "ptr_disagrees": field("ptr", lambda p: p.__setitem__(1, int(p[1]) - 1)),
        "first_octave_low": opt(first_octave=-2), "octaves_nine": opt(num_octaves=9), "peak_nan": opt(peak_threshold=float("nan")),
        "edge_zero": opt(edge_threshold=0.0), "features_zero": opt(max_num_features=0),
    }


@pytest.mark.parametrize("name", sorted(_einval_cases()))
def test_einval_without_a_device_and_outputs_untouched(lib, name, capfd):
    from xrsfm_amd import capi
    how = _einval_cases()[name]
    c, o, d = _Call(), capi.sift_options(), capi.sift_desc_options()
    if how == "opt":
        code = c.run(lib, None, d)
    elif how == "dopt":
        code = c.run(lib, o, None)
    elif isinstance(how, tuple):
        code = c.run(lib, o, d, null=how)
    else:
        how(c, o, d)
        code = c.run(lib, o, d)
    assert code == capi.EINVAL
    assert c.untouched()
    err = capfd.readouterr().err
    assert err.count("\n") == 1 and "xrsfm_ba_extract_features" in err


def test_no_images_is_success_and_a_valid_call_without_a_device_is_enodev(lib):
    import torch
    from xrsfm_amd import capi
    c = _Call()
    c.n = 0
    assert c.run(lib, capi.sift_options(), capi.sift_desc_options()) == 0 and c.untouched()
    assert c.run(lib, capi.sift_options(), capi.sift_desc_options(), null=("w", "h", "ptr", "pix", "kp", "k", "l", "s", "d", "f", "lc")) == 0
    img = c.images[0]
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    g = np.zeros((3, 80, 88, 2), F)
    o, d = capi.sift_options(), capi.sift_desc_options()
    for bad in (dict(octave=3), dict(octave=-1), dict(grad=None)):          # the test entries check before the device, too
        assert lib.xrsfm_ba_debug_sift_gradient(C.byref(o), 44, 40, img.ctypes.data_as(C.POINTER(C.c_uint8)), bad.get("octave", 0), None if "grad" in bad else p(g)) == capi.EINVAL
    n = C.c_int64(-77)
    assert lib.xrsfm_ba_debug_sift_describe(C.byref(o), None, 44, 40, img.ctypes.data_as(C.POINTER(C.c_uint8)), 0, C.byref(n), None, None, None, None) == capi.EINVAL
    assert lib.xrsfm_ba_debug_sift_describe(C.byref(o), C.byref(d), 44, 40, img.ctypes.data_as(C.POINTER(C.c_uint8)), 5, C.byref(n), None, None, None, None) == capi.EINVAL
    assert n.value == -77 and np.all(g == 0)
    if torch.cuda.is_available() and capi.device_count() > 0:
        return                                             # (with a device the valid call is the subject of tests/test_gpu_desc.py)
    c = _Call()
    assert c.run(lib, o, d) == -2 and c.untouched()
    assert c.run(lib, o, d, null=("f", "lc")) == -2 and c.untouched()
    for call in (lambda: capi.extract_features(c.images), lambda: capi.debug_sift_gradient(img, 0), lambda: capi.debug_sift_describe(img)):
        with pytest.raises(RuntimeError, match="ENODEV"):
            call()


# ---------------------------------------------------------------------------------------------------- the yardstick itself
def test_float32_restatement_is_within_every_bar_and_cap():
    dev = D.measured_deviation()
    print("measured deviation of the float32 restatement:", dev)
    assert dev["keys"] >= 1000 and dev["fragile"] <= 0.05 * dev["keys"] and dev["index_mismatch"] == 0
    assert 1e-8 < dev["vote"] < 1e-5 and 1e-8 < dev["w"] < 1e-4 and 1e-8 < dev["raw"] < 1e-4
    frag = total = 0
    for name in D.NAMES:
        inp = D.catalogue_inputs(name)
        for o, (G, _) in enumerate(Y.catalogue_reference(name, False)["pyramid"]):
            wg, wr = D.check_gradient(G[1:4], inp["planes"][o])
            assert wg <= 1.0 and wr <= 1.0, (name, o, wg, wr)
        st = D.catalogue_stages(name, False)
        okeys = np.concatenate([inp["okeys"], np.array([[s["w32"]] for s in st], F)], 1)
        r = D.check_orientation(inp["planes"], inp["loc"], okeys)
        assert r["mismatch"] == [] and r["worst"] <= 1.0 / 16 + 1e-12 and r["fragile"] <= 0.05 * len(st), (name, r)
        raw = np.stack([s["desc"]["raw"] for s in st]).astype(F)
        worst, _ = D.check_descriptor(inp["planes"], inp["loc"], okeys, raw)
        assert worst <= 1.0 / 16 + 1e-12, (name, worst)
        unit = np.stack([D.normalize(x, F) for x in raw]).astype(F)
        fl = np.stack([D.l1_root(u, F) for u in unit]).astype(F)
        n = D.check_normalisation(raw, unit, fl, D.to_bytes(fl))
        assert n["unit"] <= 1.0 and n["floats"] <= 1.0 and n["wrong"] == 0, (name, n)
        frag, total = frag + n["fragile"], total + n["total"]
    print("rounding-fragile bytes", frag, "of", total)
    assert frag <= 0.05 * total


def test_catalogue_coverage():
    clamped = np.zeros(4, int)
    oclamped = np.zeros(4, int)
    binds = 0
    for name in D.NAMES:
        st = D.catalogue_stages(name, False)
        clamped += np.array([s["desc"]["clamped"] for s in st]).sum(0)
        oclamped += np.array([s["ori"]["clamped"] for s in st]).sum(0)
        raw = np.stack([s["desc"]["raw"] for s in st]).astype(F)
        binds += D.check_normalisation(raw, np.stack([D.normalize(x, F) for x in raw]).astype(F), None, None)["clamp_binds"]
    assert np.all(clamped > 0) and np.all(oclamped > 0) and binds > 0, (clamped, oclamped, binds)          # each of the four borders; a clamp at 0.2 that binds
    a = D.catalogue_inputs("a44x40")
    assert a["planes"][2].shape == (3, 20, 24, 2) and (a["loc"][:, 0] == 2).any()          # the last, 24-wide stored octave of 44 x 40


def _uniform(h, w, grd, rot):
    p = np.zeros((3, h, w, 2), F)
    p[:, 1:-1, 1:-1, 0] = grd
    p[:, 1:-1, 1:-1, 1] = rot
    return p


def _hand_cases():
    """mode-1 inputs of the host program: gradient planes and keys (x, y, sigma, w)"""
    half = _uniform(48, 48, 1.0, 0.3)
    half[:, :, 24:, 1] = 1e-8                              # theta = -1e-8 * 4 / pi + 8 rounds to 8.0f: dropped
    one = np.zeros((3, 48, 48, 2), F)
    one[0, 24, 24] = (1.0, 0.0)                            # a single pixel with a gradient, in the middle of a cell
    return {
        "theta_zero": (_uniform(48, 48, 1.0, 0.5), (24.3, 23.8, 2.0, 0.5)),
        "dropped_8": (half, (24.5, 24.5, 2.0, 0.0)),
        "byte_255": (one, (24.5 - 3.0, 24.5 - 3.0, 2.0, 0.0)),          # cell (2, 2) has its centre at +0.5 spt = +3
        "no_gradient": (np.zeros((3, 48, 48, 2), F), (24.5, 24.5, 2.0, 0.0)),
    }


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("desc_host")
    return H.build(d), DH.build(d), d


def test_hand_built_cases(programs):
    """theta exactly 0, a dropped theta of 8.0f, a byte at 255 and the zero-denominator parabola, through ba_sift_desc_rule.h (a
    stand-alone program under the sanitizers) and both precisions of the yardstick"""
    _, exe, d = programs
    loc = np.zeros((1, 4), np.int32)
    for kind, (plane, key) in _hand_cases().items():
        got = DH.run(exe, d, [plane], loc, np.array([key], F), mode=1)
        y32, yl = D.descriptor(plane[0], np.array(key, F), F), D.descriptor(plane[0], np.array(key, F), D.LD)
        assert got["dropped"][0] == y32["dropped"] == yl["dropped"], kind
        if kind == "theta_zero":
            assert y32["zero_theta"] == y32["samples"] > 100 and y32["dropped"] == 0
            r = got["raw"][0].reshape(16, 8)
            assert np.all(r[:, 0] > 0) and np.all(r[:, 1:] == 0)
        if kind == "dropped_8":
            assert 100 < y32["dropped"] < y32["samples"] and D.theta_of(0.0, F(1e-8))[1] == F(8.0)
            assert np.all(got["raw"][0].reshape(16, 8)[[3, 7, 11, 15]] == 0)          # the right-hand column of cells sees dropped samples only
        if kind == "byte_255":
            assert (got["desc"][0] == 255).any() and got["desc_float"][0].max() > 255.5 / 512
        if kind == "no_gradient":
            v = D.peak(np.zeros(36, F), F)
            assert v[3] == 0 and v[1] == D.RAD * F(0.5) and got["w_hist"][0] == D.RAD * F(0.5) and D.peak(np.zeros(36, D.LD), D.LD)[1] == D.LD(D.RAD) * D.LD(0.5)
            continue                                       # (the descriptor of no gradient at all is 0 / 0: not defined, not tested)
        assert np.abs(got["raw"][0].astype(D.LD) - yl["raw"]).max() <= 16 * D.measured_deviation()["raw"] * yl["raw"].max(), kind
        unit = D.normalize(got["raw"][0], F).astype(F)
        fl = D.l1_root(unit, F).astype(F)
        assert np.array_equal(got["unit"][0], unit) and np.array_equal(got["desc_float"][0], fl) and np.array_equal(got["desc"][0], D.to_bytes(fl)), kind


def test_rule_header_on_the_host_reproduces_the_yardstick(programs):
    """ba_sift_desc_rule.h in a sequential program under the sanitizers, fed by the program around ba_sift_rule.h: every stage on the
    program's own inputs within the bars; against the float32 restatement the arg-max, the dropped samples, the normalised vectors
    and the bytes are equal"""
    sift_exe, exe, d = programs
    keys = fragile = 0
    for name in ("a44x40", "b50x33", "c64x48", "c64x48_o0", "d64x48"):
        o = Y.entry_options(name)
        for upright in (0, 1):
            got, s = DH.run_image(sift_exe, exe, d, Y.image(name), o, upright)
            fo = o["first_octave"]
            want = D.octave_keys(s["loc"], s["off"][:, 1:], fo)
            assert np.array_equal(got["okeys"][:, :2], want[:, :2]), name          # x, y: additions only; sigma: one powf of the library, one product
            assert np.abs(got["okeys"][:, 2] - want[:, 2]).max() <= 4 * D.EPS * want[:, 2].max(), name
            for oc, (G, _) in enumerate(s["levels"]):
                wg, wr = D.check_gradient(G[1:4], got["planes"][oc])
                assert wg <= 1.0 and wr <= 1.0, (name, oc, wg, wr)
            assert np.all(got["okeys"][:, 3] == (0 if upright else got["w_hist"]))
            r = D.check_orientation(got["planes"], s["loc"], np.concatenate([got["okeys"][:, :3], got["w_hist"][:, None]], 1))
            assert r["mismatch"] == [] and r["worst"] <= 1.0, (name, r)
            keys, fragile = keys + len(s["loc"]), fragile + r["fragile"]
            worst, dropped = D.check_descriptor(got["planes"], s["loc"], got["okeys"], got["raw"])
            assert worst <= 1.0 and dropped == int(got["dropped"].sum()), (name, worst)
            for k, (oc, j, _, _) in enumerate(s["loc"].tolist()):
                y = D.orientation(got["planes"][oc][j], got["okeys"][k], F)
                if not D.orient_fragile(D.orientation(got["planes"][oc][j], got["okeys"][k]), 16 * D.measured_deviation()["vote"]):
                    assert int(np.argmax(got["vote"][k])) == y["index"], (name, k)
                unit = D.normalize(got["raw"][k], F).astype(F)
                fl = D.l1_root(unit, F).astype(F)
                assert np.array_equal(got["unit"][k], unit) and np.array_equal(got["desc_float"][k], fl) and np.array_equal(got["desc"][k], D.to_bytes(fl)), (name, k)
            n = D.check_normalisation(got["raw"], got["unit"], got["desc_float"], got["desc"])
            assert n["unit"] <= 1.0 and n["floats"] <= 1.0 and n["wrong"] == 0 and n["fragile"] <= 0.05 * n["total"], (name, n)
    assert keys > 400 and fragile <= 0.05 * keys


def test_inputs_of_the_end_to_end_and_rotation_tests(tmp_path):
    """the comparator yields at least 20 correct matches and no wrong one on the canvas chosen; the rotated pair shares at least 10
    keypoints, and the deviation its gradient planes cause is small against a bin"""
    small = [Y.translated(8, 8), Y.translated(12, 12)]
    assert small[0].shape == (80, 96)                      # (the canvas of test_gpu_sift.py: too small, see tests/desc_cases.py)
    correct, wrong = K.e2e_comparator(tmp_path)
    print("comparator: correct", correct, "wrong", wrong)
    assert correct >= 20 and wrong == 0
    a, b = K.rotation_images()
    assert a.shape == (64, 64) and np.array_equal(np.rot90(a), b)
    ra, rb = (Y.reference(x, False, first_octave=0) for x in (a, b))
    dev = K.rotation_plane_deviation()
    print("rotation: pairs", len(K.rotation_pairs(ra["loc"], rb["loc"])), "16 x deviation %.3e" % dev)
    assert len(K.rotation_pairs(ra["loc"], rb["loc"])) >= 10 and 0 < dev < 0.1 * np.pi / 18


def test_descriptor_kernels_do_not_spill(tmp_path):
    """k_siftd_grad, k_siftd_record, k_siftd_orient and k_siftd_desc of the gfx950 code object: no spilled register, no private
    (scratch) segment; the orientation kernel holds its per-lane histograms and the two smoothing copies in 36 * 256 * 4 + 2 * 16 * 37
    * 4 bytes of LDS, the others none."""
    from xrsfm_amd import _build
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = tmp_path / "siftd_only.hip"
    src.write_text('#include "ba_sift_desc.h"\n')
    asm = tmp_path / "siftd.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-I", _build.CSRC, str(src), "-o", str(asm)], check=True, capture_output=True)
    seen = {}
    for blk in asm.read_text().split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        m = re.search(r"k_siftd_(grad|record|orient|desc)", name)
        if not m:
            continue
        num = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, blk).group(1))
        fig = dict(vgpr=num("vgpr_count"), sgpr=num("sgpr_count"), lds=num("group_segment_fixed_size"), scratch=num("private_segment_fixed_size"), spill=num("vgpr_spill_count"))
        seen[m.group(1)] = fig
        assert fig["spill"] == 0 and fig["scratch"] == 0 and fig["vgpr"] <= 128, (name, fig)
    print("descriptor kernels:", seen)
    assert sorted(seen) == ["desc", "grad", "orient", "record"]
    assert seen["orient"]["lds"] == 4 * (36 * 256 + 2 * 16 * 37) and all(seen[k]["lds"] == 0 for k in ("grad", "record", "desc"))
