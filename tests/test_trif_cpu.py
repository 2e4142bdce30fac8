"""Frame triangulation without a GPU: the two formulations of the yardstick agree on the whole catalogue, the catalogue's
table shows every rule exercised, no case is fragile (no decision of the longdouble run lies within 1e-9 of its threshold), the rule
header as a stand-alone program built with the address and undefined-behaviour sanitizers equals the yardstick, the dot-product rule at
1, 1 + 2^-52 and the threshold's neighbours, every EINVAL before a device is needed with one line on stderr and untouched outputs, real
work without a device is ENODEV, and the new kernels neither spill nor use scratch while k_tri_tracks keeps its figures."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import trif_cases as TC
from tests import trif_host_driver as HD
from tests import trif_yardstick as Y

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("xrsfm_ba_trif_options_default", "xrsfm_ba_triangulate_frames")
CASE_MODES = [(n, m) for n in TC.NAMES for m in TC.MODES]
p = lambda a, t: a.ctypes.data_as(C.POINTER(t)) if a is not None else None


@pytest.fixture(autouse=True)
def the_feature(lib):
    """every test of this file is about xrsfm_ba_triangulate_frames: the yardstick and the catalogue are checked for a library that has it"""
    for name in NAMES:
        assert hasattr(lib, name), name


def _one_line(err, name):
    return err.count("\n") == 1 and name in err


def test_the_new_symbols_are_declared_and_exported(lib):
    from xrsfm_amd import capi
    hdr = open(os.path.join(ROOT, "include", "xrsfm_ba.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in capi.EXPORTS and getattr(lib, name) is not None, name
    for word in ("xrsfm_ba_trif_options", "no output is touched", "Documented deviation"):
        assert word in hdr, word
    o, t = capi.trif_options(), capi.triangulate_options()
    assert o.extend_angle_rad == Y.EXTEND_ANGLE == 8.0 * 0.017453292519943295
    assert [getattr(o.tri, k) for k, _ in capi.CTriOptions._fields_] == [getattr(t, k) for k, _ in capi.CTriOptions._fields_]
    assert C.sizeof(capi.CTrifOptions) == 48 == 8 + C.sizeof(capi.CTriOptions)
    assert capi.trif_options(extend_angle_rad=0.1, max_num_trials=7).tri.max_num_trials == 7
    with pytest.raises(AttributeError):
        capi.trif_options(no_such_field=1)
    assert tuple(capi.TRIF_STATS) == Y.STATS


# ---------------------------------------------------------------------------------------------------- the yardstick and the catalogue
@pytest.mark.parametrize("name,mode", CASE_MODES)
def test_the_two_formulations_agree(name, mode):
    """(A) and (B) in float64: every integer and every bit of every point ((A) knows no steps: the five counters the reference prints)"""
    c, b = TC.case(name), TC.expected(name, mode)
    if name == "rules":
        assert len(c["key_ptr"]) - 1 <= 12 and np.diff(c["key_ptr"]).max() <= 40
    if name.startswith("scene"):
        assert len(c["key_ptr"]) - 1 <= 40 and np.diff(c["key_ptr"]).max() <= 200
    a = TC.literal(name, mode)
    assert Y.integer_differences(a, b, stats=5) == []
    assert np.array_equal(Y.point_bits(a["points"]), Y.point_bits(b["points"]))
    assert Y.capacity(c, TC.frames_of(c, mode)) >= b["n_tracks"]


WANTED = {
    "rules": TC.RULES[:18] + ("list_129",),
    "sizes": ("list_128", "list_129", "status_created", "status_too_many"),
    "chain_3": ("rounds_3",), "chain_64": ("rounds_64",), "chain_65": ("rounds_65",), "chain_200": ("rounds_200",),
    "wide": ("wide_step", "status_created", "status_extended"),
    "scene_a": ("status_created", "status_extended", "status_none_accepted", "holds_frame", "outliers_left", "later_frame_extends_created"),
}


def test_every_rule_is_exercised():
    table = {name: TC.coverage(name) for name in TC.NAMES}
    for name, wanted in WANTED.items():
        for rule in wanted:
            assert table[name][rule], (name, rule)
    assert [r for r in TC.RULES if not any(table[n][r] for n in TC.NAMES)] == []
    for name in TC.NAMES:
        print("%-9s %s" % (name, "".join("x" if table[name][r] else "." for r in TC.RULES)))
    # what the constructed key points of `rules` end as, in frame mode
    c, r = TC.case("rules"), TC.expected("rules", "frame")
    ix, st, tok = c["index"], r["key_status"], r["track_of_key"]
    T = len(c["points"])
    want = dict(create=1, create_outlier=1, lonely=2, unreg_only=2, no_model=4, extend=5, reject=6, second_choice=5, ineligible=6, tie=5, multi=5, zero_ray=6, couple_1=1,
                couple_2=6, long=3, later=0, holder=0)
    assert {k: int(st[ix[k]]) for k in want} == want
    assert tok[ix["wrong"]] == -1 and tok[ix["create_outlier"]] >= T and tok[ix["second_choice"]] == 3 and tok[ix["tie"]] == 4 and tok[ix["multi"]] == 7
    assert r["stats"].tolist()[5:7] == [2, 1] and tok[ix["ineligible"]] == -1 and r["n_tracks"] == T + 3
    m = TC.expected("rules", "map")
    assert m["key_status"][ix["later"]] == 5 and m["track_of_key"][ix["later"]] >= T
    # the chains: every key point ends on the track of its own index, which a one-round resolution does not give
    for L in (3, 64, 65, 200):
        c, r = TC.case("chain_%d" % L), TC.expected("chain_%d" % L, "frame")
        k0 = c["index"]["first"]
        assert r["track_of_key"][k0:k0 + L].tolist() == list(range(L)) and r["stats"][7] == L
    c, r = TC.case("wide"), TC.expected("wide", "frame")
    assert r["track_of_key"][c["index"]["first"]:c["index"]["last"] + 1].tolist() == list(range(140, 180)) and c["index"]["first"] - c["key_ptr"][3] >= 256


@pytest.mark.parametrize("name,mode", CASE_MODES)
def test_no_case_is_fragile(name, mode):
    """apart from the constructed tie, no decision of the longdouble run lies within 1e-9 (relative) of its threshold, and every integer
    of the float64 run is the longdouble run's"""
    a, l = TC.literal(name, mode), TC.literal(name, mode, "longdouble")
    near = [m for m in l["margins"] if not m[2] and m[1] < 1e-9]
    assert near == []
    exact = [m for m in l["margins"] if m[2]]
    assert exact == [] or (name == "rules" and {m[0] for m in exact} == {"order"})
    assert Y.integer_differences(a, l) == []
    assert len(a["margins"]) == len(l["margins"])


# ---------------------------------------------------------------------------------------------------- the rule header, sanitized
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return HD.build(tmp_path_factory.mktemp("trif_rule"))


@pytest.mark.parametrize("name,mode", CASE_MODES)
def test_the_rule_header_equals_the_yardstick(driver, name, mode):
    c, b = TC.case(name), TC.expected(name, mode)
    frames = TC.frames_of(c, mode)
    out = HD.run(driver, HD.case_input(c, frames, expected=b, create=Y.cpu_create_for(c)))
    assert "fault" not in out, out.get("fault")
    for k in ("track_of_key", "track_outlier", "key_status", "stats"):
        assert out[k] == np.asarray(b[k]).astype(np.int64).tolist(), k
    assert out["n_tracks"] == [b["n_tracks"]] and out["point_bits"] == Y.point_bits(b["points"]).reshape(-1).tolist()
    P = Y.plan(c, frames)
    assert out["slot_key"] == P["slot_key"] and out["step_frame"] == [f for f, _ in P["steps"]] and out["step_slot0"] == [0] + [s[-1] + 1 for _, s in P["steps"]]


def test_the_rule_header_refuses_what_the_entry_refuses(driver):
    c = TC.case("rules")
    f = lambda frames=(5,), capacity=None, **kw: " ".join(HD.run(driver, HD.case_input(c, list(frames), capacity=capacity, **kw)).get("fault", []))
    assert "listed twice" in f(frames=(5, 5)) and "not registered" in f(frames=(3,)) and "out of range" in f(frames=(12,))
    assert "track_capacity" in f(capacity=Y.capacity(c, [5]) - 1) and "track_capacity" in f(capacity=len(c["points"]) - 1)
    assert "extend_angle_rad" in f(extend_angle_rad=-0.1)
    tok = c["track_of_key"].copy(); tok[0] = 99
    assert "track index" in f(track_of_key=tok)
    out = c["track_outlier"].copy(); out[0] = 1
    assert "outlier track" in f(track_outlier=out)
    ck = c["corr_key"].copy(); ck[0] = ck[1]
    assert "non-symmetric" in f(corr_key=ck) or "own frame" in f(corr_key=ck)


def test_the_dot_product_rule_at_its_edges(driver):
    """1 is a valid cosine and 1 + 2^-52 is not (its acos is NaN: never best); the bound is the smallest double whose acos is below the
    threshold, so its neighbour below is refused; equal dot products go to the smaller id"""
    th = Y.EXTEND_ANGLE
    bound = Y.dot_bound(th)
    below, above = np.nextafter(bound, -1.0), np.nextafter(bound, 2.0)
    assert math.acos(bound) < th <= math.acos(below) and abs(bound - math.cos(th)) < 1e-15
    dots = [1.0, 1.0 + 2.0 ** -52, np.nextafter(1.0, 0.0), bound, below, above, 0.0, -1.0, np.nextafter(-1.0, -2.0), float("nan"), bound, bound]
    out = HD.run(driver, HD.unit_input(th, dots))
    assert out["bound"] == [int(np.float64(bound).view(np.uint64))]
    assert out["valid"] == [1, 0, 1, 1, 1, 1, 1, 1, 0, 0, 1, 1] == [int(Y.dot_valid(d)) for d in dots]
    assert out["accepts"] == [1, 1, 1, 1, 0, 1, 0, 0, 0, 0, 1, 1] == [int(d >= bound) for d in dots]
    nxt = dots[1:] + dots[:1]
    assert out["better_larger_id"] == [int(Y.better(d, 1, e, 0)) for d, e in zip(dots, nxt)]
    assert out["better_smaller_id"] == [int(Y.better(d, 0, e, 1)) for d, e in zip(dots, nxt)]
    assert out["better_larger_id"][-2] == 0 and out["better_smaller_id"][-2] == 1            # bound against bound: the smaller id
    for th2, want in ((0.0, 2.0), (3.2, -1.0), (math.pi, np.nextafter(-1.0, 0.0))):
        assert HD.run(driver, HD.unit_input(th2, [0.5]))["bound"] == [int(np.float64(want).view(np.uint64))] and Y.dot_bound(th2) == want
    half = Y.dot_bound(math.pi / 2)
    assert math.acos(half) < math.pi / 2 <= math.acos(np.nextafter(half, -1.0))


# ---------------------------------------------------------------------------------------------------- the entry's argument checks
class _Call:
    """one xrsfm_ba_triangulate_frames call on the `rules` case in frame mode, every output at a fill value"""

    def __init__(self):
        from xrsfm_amd import capi
        c = TC.case("rules")
        T, cap = len(c["points"]), Y.capacity(c, [5])
        pts, out = np.zeros((cap, 3)), np.zeros(cap, np.uint8)
        pts[:T] = c["points"]
        self.a = dict(opt=capi.trif_options(), n=len(c["key_ptr"]) - 1, n_list=1, frames=np.array([5], np.int32), T=T, cap=cap, points=pts, track_outlier=out,
                      **{k: np.ascontiguousarray(c[k]).copy() for k in ("key_ptr", "key_xyn", "registered", "cam_q", "cam_t", "corr_ptr", "corr_key", "track_of_key")})

    def run(self, lib, **kw):
        """-> (code, whether the three state arrays and every output are as before the call)"""
        a = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in dict(self.a, **kw).items()}
        n, N = self.a["n"], len(self.a["track_of_key"])
        o = dict(status=np.full(N, 77, np.uint8), ninl=np.full(N, -77, np.int32), ntr=np.full(N, -77, np.int32), best=np.full(N, -77, np.int32), have=np.full(N, -77, np.int32),
                 vis=np.full(n, -77, np.int32), mea=np.full(n, -77, np.int32), stats=np.full(8, -77, np.int64), nout=np.full(1, -77, np.int32))
        before = {k: a[k].copy() for k in ("points", "track_outlier", "track_of_key") if a[k] is not None}
        i32, i64, u8, f64 = C.c_int32, C.c_int64, C.c_uint8, C.c_double
        code = lib.xrsfm_ba_triangulate_frames(C.byref(a["opt"]) if a["opt"] is not None else None, a["n"], p(a["key_ptr"], i64), p(a["key_xyn"], f64), p(a["registered"], u8),
                                               p(a["cam_q"], f64), p(a["cam_t"], f64), p(a["corr_ptr"], i64), p(a["corr_key"], i32), a["n_list"], p(a["frames"], i32), a["T"],
                                               a["cap"], p(a["points"], f64), p(a["track_outlier"], u8), p(a["track_of_key"], i32), p(o["nout"], i32), p(o["status"], u8),
                                               p(o["ninl"], i32), p(o["ntr"], i32), p(o["best"], i32), p(o["have"], i32), p(o["vis"], i32), p(o["mea"], i32), p(o["stats"], i64))
        same = all(np.array_equal(a[k], v, equal_nan=v.dtype.kind == "f") for k, v in before.items())
        return code, same and all(np.all(v == (77 if v.dtype == np.uint8 else -77)) for v in o.values())


def test_triangulate_frames_refuses_bad_arguments_before_a_device_is_needed(lib, capfd):
    from xrsfm_amd import capi
    c = _Call()
    a = c.a
    to = capi.trif_options

    def changed(key, index, value):
        v = a[key].copy()
        v[index] = value
        return {key: v}

    case = TC.case("rules")
    ix, kp = case["index"], case["key_ptr"]
    own = a["corr_key"].copy(); own[a["corr_ptr"][ix["extend"]]] = ix["tie"]                     # the first entry of a key point of frame 5 points into frame 5
    outlier_carried = a["track_outlier"].copy(); outlier_carried[0] = 1
    cases = [dict(opt=None), dict(opt=to(extend_angle_rad=-1e-3)), dict(opt=to(extend_angle_rad=3.3)), dict(opt=to(extend_angle_rad=float("nan"))),
             dict(opt=to(max_error_rad=0.0)), dict(opt=to(confidence=1.5)), dict(opt=to(min_inlier_ratio=-0.1)), dict(opt=to(max_num_trials=0)),
             dict(opt=to(exhaustive_threshold=-1)), dict(opt=to(min_tri_angle_rad=-1.0)), dict(opt=to(max_error_rad=float("inf"))),
             dict(n=-1), dict(T=-1), dict(n_list=-1), dict(cap=-1), dict(cap=a["T"] - 1), dict(cap=a["cap"] - 1),
             dict(key_ptr=None), dict(key_xyn=None), dict(registered=None), dict(cam_q=None), dict(cam_t=None), dict(corr_ptr=None), dict(corr_key=None), dict(frames=None),
             dict(points=None), dict(track_outlier=None), dict(track_of_key=None),
             dict(frames=np.array([12], np.int32)), dict(frames=np.array([-1], np.int32)), dict(frames=np.array([3], np.int32)),
             dict(frames=np.array([5, 5], np.int32), n_list=2), dict(frames=np.array([5], np.int32), **changed("registered", 5, 0)),
             changed("key_ptr", 0, 1), changed("key_ptr", 3, 1), changed("corr_ptr", 0, 1), changed("corr_ptr", 2, 0), changed("corr_key", 0, int(kp[-1])), changed("corr_key", 0, -1),
             changed("track_of_key", 0, a["T"]), changed("track_of_key", 0, -2), dict(track_outlier=outlier_carried), dict(corr_key=own), changed("corr_key", 0, ix["lonely"]),
             changed("cam_q", (1, 2), np.nan), changed("cam_t", (0, 0), np.inf), changed("points", (3, 1), np.nan), changed("key_xyn", (4, 0), -np.inf)]
    for kw in cases:
        capfd.readouterr()
        code, untouched = c.run(lib, **kw)
        err = capfd.readouterr().err
        assert code == capi.EINVAL and _one_line(err, "xrsfm_ba_triangulate_frames") and untouched, (kw, code, err)


def test_nothing_to_do_is_success_without_a_device(lib):
    from xrsfm_amd import capi
    z = lambda t, *s: np.zeros(s or (0,), t)
    r = capi.triangulate_frames(np.zeros(1, np.int64), z(np.float64, 0, 2), z(np.uint8), z(np.float64, 0, 4), z(np.float64, 0, 3), np.zeros(1, np.int64), z(np.int32), [],
                                z(np.float64, 0, 3), z(np.uint8), z(np.int32))
    assert r["n_tracks"] == 0 and r["stats"]["steps"] == 0
    c = TC.case("rules")
    # no frame listed; a frame whose key points without a track have no second observation (every other frame unregistered)
    none = capi.triangulate_frames(*TC.arrays(c, "frame")[:7], [], *TC.arrays(c, "frame")[8:])
    want = Y.run_flat(c, [], None)
    assert Y.integer_differences(none, want) == [] and none["points"].tobytes() == c["points"].tobytes() and set(none["key_status"].tolist()) == {0}
    reg = np.zeros(12, np.uint8); reg[5] = 1
    alone = dict(c, registered=reg)
    r = capi.triangulate_frames(*TC.arrays(alone, "frame"))
    want = Y.run_flat(alone, [5], None)
    assert Y.integer_differences(r, want) == [] and (r["key_status"][c["key_ptr"][5]:c["key_ptr"][6]] == np.where(c["track_of_key"][c["key_ptr"][5]:c["key_ptr"][6]] < 0, 2, 0)).all()
    assert r["best_trial"].tolist() == [-1] * len(r["best_trial"]) and r["measured"].sum() == (c["track_of_key"] >= 0).sum()


def test_real_work_without_a_device_is_enodev(lib):
    import torch
    from xrsfm_amd import capi
    if torch.cuda.is_available() and capi.device_count() > 0:
        pytest.skip("a GPU is present")
    c = _Call()
    code, untouched = c.run(lib)
    assert code == -2 and untouched
    with pytest.raises(RuntimeError, match="ENODEV"):
        capi.triangulate_frames(*TC.arrays(TC.case("rules"), "map"))


# ---------------------------------------------------------------------------------------------------- the code object
def _figures(tmp_path, header, pattern):
    from xrsfm_amd import _build
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src, asm = tmp_path / (header + "_only.hip"), tmp_path / (header + ".s")
    src.write_text('#include <hip/hip_runtime.h>\n#include "%s.h"\n' % header)
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-I", _build.CSRC, str(src), "-o", str(asm)], check=True, capture_output=True)
    seen = {}
    for blk in asm.read_text().split("  - .agpr_count:")[1:]:
        m = re.search(pattern, re.search(r"\.name:\s+(\S+)", blk).group(1))
        if m:
            num = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, blk).group(1))
            seen[m.group(0)] = dict(vgpr=num("vgpr_count"), sgpr=num("sgpr_count"), lds=num("group_segment_fixed_size"), scratch=num("private_segment_fixed_size"),
                                    spill=num("vgpr_spill_count"), sspill=num("sgpr_spill_count"))
    return seen


def test_trif_kernels_do_not_spill_and_k_tri_tracks_is_unchanged(tmp_path):
    """the kernels of ba_trif.h in the gfx950 code object: no spilled register, no private (scratch) segment, at most 64 vector registers
    (eight waves per SIMD), 16 bytes of LDS for the prefix sums of the two one-workgroup kernels and 256 more for the workgroup-wide "or"
    of k_trif_resolve; k_tri_tracks, which ba_trif.h launches as it stands, keeps
    the figures it had before: 210 vector registers, 95 scalar registers, 68 KiB of LDS"""
    seen = _figures(tmp_path, "ba_trif", r"k_trif_(held|classify|select|resolve)")
    print("frame triangulation kernels:", seen)
    assert sorted(seen) == ["k_trif_classify", "k_trif_held", "k_trif_resolve", "k_trif_select"]
    for name, fig in seen.items():
        assert fig["spill"] == 0 and fig["sspill"] == 0 and fig["scratch"] == 0 and fig["vgpr"] <= 64, (name, fig)
    # the table of DESIGN.md 5s
    assert {k: (v["vgpr"], v["sgpr"]) for k, v in seen.items()} == dict(k_trif_held=(3, 16), k_trif_classify=(58, 58), k_trif_select=(40, 63), k_trif_resolve=(30, 87))
    assert {k: v["lds"] for k, v in seen.items()} == dict(k_trif_held=0, k_trif_classify=0, k_trif_select=16, k_trif_resolve=16 + 256)
    tri = _figures(tmp_path, "ba_tri", r"k_tri_tracks")
    assert tri == dict(k_tri_tracks=dict(vgpr=210, sgpr=95, lds=4 * 128 * 17 * 8, scratch=0, spill=0, sspill=0))
    src = open(os.path.join(ROOT, "xrsfm_amd", "csrc", "ba_trif.h")).read()
    assert set(re.findall(r"atomic(?:Add|Min|Max|CAS|Exch)\(a\.(\w+)", src)) == {"counters", "bid"}          # the only atomics: on two int32 arrays
