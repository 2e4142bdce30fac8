"""Track completion and merging without a GPU: the two formulations of the yardstick agree on the whole catalogue, the
catalogue's table shows every rule exercised, no case is fragile (no comparison of the longdouble run lies near the threshold), the rule
header as a stand-alone program built with the address and undefined-behaviour sanitizers equals the yardstick, the numpy helpers equal
their restatements, every EINVAL comes before a device is needed with one line on stderr and untouched outputs, real work without a
device is ENODEV, and the two kernels neither spill nor use scratch."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import merge_cases as MC
from tests import merge_host_driver as HD
from tests import merge_yardstick as Y

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("xrsfm_ba_merge_options_default", "xrsfm_ba_merge_tracks", "xrsfm_ba_debug_merge_components")
CASE_MODES = [(n, m) for n in MC.NAMES for m in Y.MODES]
p = lambda a, t: a.ctypes.data_as(C.POINTER(t)) if a is not None else None


def _one_line(err, name):
    return err.count("\n") == 1 and name in err


def test_the_new_symbols_are_declared_and_exported(lib):
    from xrsfm_amd import capi
    hdr = open(os.path.join(ROOT, "include", "xrsfm_ba.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in capi.EXPORTS and getattr(lib, name) is not None, name
    for word in ("XRSFM_BA_MERGE_CONTINUE 1", "XRSFM_BA_MERGE_MERGE    2", "XRSFM_BA_MERGE_FRAME    4", "XRSFM_BA_MERGE_MAX_KEYS 1024", "XRSFM_BA_MERGE_MAX_TRACKS 512",
                 "no output is touched"):
        assert word in hdr, word
    o = capi.merge_options()
    assert (o.max_reproj_error, o.mode, o.frame) == (8.0, 3, -1)
    assert C.sizeof(capi.CMergeOptions) == 16
    assert (capi.MERGE_MAX_KEYS, capi.MERGE_MAX_TRACKS) == (Y.MAX_KEYS, Y.MAX_TRACKS)


# ---------------------------------------------------------------------------------------------------- the yardstick and the catalogue
@pytest.mark.parametrize("name,mode", CASE_MODES)
def test_the_two_formulations_agree(name, mode):
    """(A) and (B) in float64: every integer and every bit of every point"""
    c, a = MC.case(name), MC.expected(name, mode)
    if name in ("rules", "live"):
        assert len(c["key_ptr"]) - 1 <= 12 and np.diff(c["key_ptr"]).max() <= 40
    if name.startswith("scene"):
        assert len(c["key_ptr"]) - 1 <= 40 and np.diff(c["key_ptr"]).max() <= 200 and set(c["intr_model"].tolist()) == {0, 1, 2, 3, 4}
    b = Y.run_components(c, mode)
    assert Y.integer_differences(a, b) == []
    assert np.array_equal(Y.point_bits(a["points"]), Y.point_bits(b["points"]))


WANTED = {
    "rules": Y.RULES[:6] + Y.RULES[9:20],
    "live": (Y.RULES[0], Y.RULES[3]) + Y.RULES[6:9] + (Y.RULES[16],),
    "sizes": Y.RULES[20:27],
    "limits": Y.RULES[27:31],
    "scene_a": Y.RULES[:4],
}


def test_every_rule_is_exercised():
    table = {name: MC.coverage(name) for name in MC.NAMES}
    for name, wanted in WANTED.items():
        for rule in wanted:
            assert table[name][rule], (name, rule)
    assert [r for r in Y.RULES if not any(table[n][r] for n in MC.NAMES)] == []
    for name in MC.NAMES:
        print("%-8s %s" % (name, "".join("x" if table[name][r] else "." for r in Y.RULES)))
    # merges fail as well as succeed in the scenes, and a scene holds a component above the limits
    for name in ("scene_a", "scene_b"):
        s = MC.expected(name, 3)["stats"]
        assert 0 < s[0] < s[1] and 0 < s[2] < s[3], (name, s)
    assert MC.expected("scene_b", 3)["stats"][5] == 1 and MC.expected("limits", 3)["stats"].tolist()[4:7] == [2, 2, 1024]


@pytest.mark.parametrize("name,mode", CASE_MODES)
def test_no_case_is_fragile(name, mode):
    """apart from the constructed exact and NaN comparisons, nothing the longdouble run compares lies within 1e-6 px of the threshold,
    and every integer of the float64 run is the longdouble run's"""
    a, l = MC.expected(name, mode), MC.expected_long(name, mode)
    near = [m for m in l["margins"] if not m[2] and m[0] < 1e-6]
    assert near == []
    exact = [m for m in l["margins"] if m[2]]
    assert exact == [] or name == "rules"
    assert Y.integer_differences(a, l) == []
    assert len(a["margins"]) == len(l["margins"])


# ---------------------------------------------------------------------------------------------------- the rule header, sanitized
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return HD.build(tmp_path_factory.mktemp("merge_rule"))


@pytest.mark.parametrize("name,mode", CASE_MODES)
def test_the_rule_header_equals_the_yardstick(driver, name, mode):
    c = MC.case(name)
    out = HD.run(driver, HD.case_input(c, mode))
    assert "fault" not in out, out.get("fault")
    b = Y.run_components(c, mode)
    for k in Y.INTEGERS:
        assert out[k] == np.asarray(b[k]).astype(np.int64).tolist(), k
    assert out["point_bits"] == Y.point_bits(b["points"]).reshape(-1).tolist()
    comp, sizes = Y.components(c)
    assert out["comp_of_key"] == comp.tolist()


def test_the_rule_header_refuses_what_the_entry_refuses(driver):
    c = MC.case("live")
    f = lambda **kw: " ".join(HD.run(driver, HD.case_input(dict(c, **{k: v for k, v in kw.items() if k in c}), kw.get("mode", 3), frame=kw.get("frame"), max_re=kw.get("max_re")))
                              .get("fault", []))
    assert f() == ""
    assert "max_reproj_error" in f(max_re=0.0) and "mode" in f(mode=5) and "out of range" in f(mode=4, frame=6)
    reg = c["registered"].copy(); reg[2] = 0
    assert "not registered" in f(mode=4, frame=2, registered=reg)
    tok = c["track_of_key"].copy(); tok[0] = 8
    assert "track index" in f(track_of_key=tok)
    ck = c["corr_key"].copy(); ck[0] = ck[1]
    assert "non-symmetric" in f(corr_key=ck) or "own frame" in f(corr_key=ck)


# ---------------------------------------------------------------------------------------------------- the numpy helpers
def test_correspondence_graph_equals_map_init():
    from xrsfm_amd import capi
    rng = np.random.default_rng(5)
    key_ptr = np.array([0, 5, 9, 9, 16], np.int64)
    pa, pb = np.array([0, 3, 1, 0], np.int32), np.array([1, 0, 3, 3], np.int32)
    counts = [4, 3, 0, 5]
    matches = []
    for a, b, n in zip(pa, pb, counts):
        na, nb = key_ptr[a + 1] - key_ptr[a], key_ptr[b + 1] - key_ptr[b]
        matches += [(int(rng.integers(na)), int(rng.integers(nb))) for _ in range(n)]
    match_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    ptr, key = capi.correspondence_graph(key_ptr, pa, pb, match_ptr, np.array(matches, np.int32))
    lists = [[] for _ in range(16)]            # Map::Init: corrs_vector1.emplace_back(id2, match.id2); corrs_vector2.emplace_back(id1, match.id1)
    for i, (a, b) in enumerate(zip(pa, pb)):
        for ma, mb in matches[match_ptr[i]:match_ptr[i + 1]]:
            lists[key_ptr[a] + ma].append(int(key_ptr[b] + mb))
            lists[key_ptr[b] + mb].append(int(key_ptr[a] + ma))
    assert ptr.tolist() == np.concatenate([[0], np.cumsum([len(v) for v in lists])]).tolist() and key.tolist() == [g for v in lists for g in v]
    assert key.dtype == np.int32 and ptr.dtype == np.int64


@pytest.mark.parametrize("name", ("rules", "live", "scene_a", "scene_b"))
def test_merge_closure_is_closed_under_components(name):
    from xrsfm_amd import capi
    c = MC.case(name)
    comp, _ = Y.components(c)
    kp, tok = c["key_ptr"], c["track_of_key"]
    s = capi.merge_closure(c["frame"], kp, c["corr_ptr"], c["corr_key"], tok)
    seeds = [k for k in range(kp[c["frame"]], kp[c["frame"] + 1]) if tok[k] >= 0]
    want = np.nonzero(np.isin(comp, np.unique(comp[seeds])))[0]
    assert s["keys"].tolist() == want.tolist() and len(want) > 0
    assert s["tracks"].tolist() == sorted({int(t) for t in tok[want] if t >= 0})
    # the sub-map is the map restricted to those keys
    assert np.diff(s["key_ptr"]).tolist() == [int(((want >= kp[f]) & (want < kp[f + 1])).sum()) for f in range(len(kp) - 1)]
    back = s["keys"][s["corr_key"]]
    full = np.concatenate([c["corr_key"][c["corr_ptr"][k]:c["corr_ptr"][k + 1]] for k in want])
    assert back.tolist() == full.tolist() and np.diff(s["corr_ptr"]).tolist() == (c["corr_ptr"][want + 1] - c["corr_ptr"][want]).tolist()
    assert np.where(s["track_of_key"] >= 0, s["tracks"][np.maximum(s["track_of_key"], 0)], -1).tolist() == tok[want].tolist()


def test_the_components_equal_the_yardstick(lib):
    from xrsfm_amd import capi
    for name in MC.QUICK:
        c = MC.case(name)
        comp, n = capi.debug_merge_components(*MC.arrays(c))
        want, sizes = Y.components(c)
        assert n == len(sizes) and np.array_equal(comp, want), name


# ---------------------------------------------------------------------------------------------------- the entry's argument checks
class _Call:
    """one xrsfm_ba_merge_tracks call on the `live` case, every output at a fill value"""

    def __init__(self):
        from xrsfm_amd import capi
        c = MC.case("live")
        self.a = dict(opt=capi.merge_options(), n=len(c["key_ptr"]) - 1, n_intr=1, T=len(c["points"]),
                      **{k: np.ascontiguousarray(c[k]).copy() for k in ("key_ptr", "key_xy", "registered", "cam_q", "cam_t", "cam_intr", "intr_model", "intr_params", "corr_ptr",
                                                                         "corr_key", "points", "track_outlier", "track_of_key")})
        self.fill()

    def fill(self):
        n, N, T = self.a["n"], len(self.a["track_of_key"]), self.a["T"]
        self.out = dict(status=np.full(T, 77, np.uint8), have=np.full(N, -77, np.int32), vis=np.full(n, -77, np.int32), mea=np.full(n, -77, np.int32),
                        stats=np.full(8, -77, np.int64))

    def run(self, lib, **kw):
        """-> (code, whether the three state arrays and every output are as before the call)"""
        self.fill()
        a = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in dict(self.a, **kw).items()}
        before = {k: a[k].copy() for k in ("points", "track_outlier", "track_of_key") if a[k] is not None}
        o = self.out
        i32, i64, u8, f64 = C.c_int32, C.c_int64, C.c_uint8, C.c_double
        code = lib.xrsfm_ba_merge_tracks(C.byref(a["opt"]) if a["opt"] is not None else None, a["n"], p(a["key_ptr"], i64), p(a["key_xy"], f64), p(a["registered"], u8),
                                         p(a["cam_q"], f64), p(a["cam_t"], f64), p(a["cam_intr"], i32), a["n_intr"], p(a["intr_model"], i32), p(a["intr_params"], f64),
                                         p(a["corr_ptr"], i64), p(a["corr_key"], i32), a["T"], p(a["points"], f64), p(a["track_outlier"], u8), p(a["track_of_key"], i32),
                                         p(o["status"], u8), p(o["have"], i32), p(o["vis"], i32), p(o["mea"], i32), p(o["stats"], i64))
        same = all(np.array_equal(a[k], v, equal_nan=v.dtype.kind == "f") for k, v in before.items())
        return code, same and all(np.all(v == (77 if v.dtype == np.uint8 else -77)) for v in o.values())


def test_merge_refuses_bad_arguments_before_a_device_is_needed(lib, capfd):
    from xrsfm_amd import capi
    c = _Call()
    a = c.a
    mo = capi.merge_options

    def changed(key, index, value):
        v = a[key].copy()
        v[index] = value
        return {key: v}

    live = MC.case("live")
    ix = live["index"]
    same_frame = a["track_of_key"].copy(); same_frame[ix["c2"]] = same_frame[ix["a2"]]            # two keys of frame 2 on one track
    own = a["corr_key"].copy(); own[a["corr_ptr"][ix["s2"]]] = ix["a2"]                            # s2's first entry points into frame 2
    cases = [dict(opt=None), dict(opt=mo(max_reproj_error=0.0)), dict(opt=mo(max_reproj_error=-1.0)), dict(opt=mo(max_reproj_error=float("nan"))), dict(opt=mo(mode=0)),
             dict(opt=mo(mode=5)), dict(opt=mo(mode=7)), dict(opt=mo(mode=4, frame=-1)), dict(opt=mo(mode=4, frame=6)), dict(opt=mo(mode=4, frame=2), **changed("registered", 2, 0)),
             dict(n=-1), dict(T=-1), dict(n_intr=-1), dict(key_ptr=None), dict(key_xy=None), dict(registered=None), dict(cam_q=None), dict(cam_t=None), dict(cam_intr=None),
             dict(intr_model=None), dict(intr_params=None), dict(corr_ptr=None), dict(corr_key=None), dict(points=None), dict(track_outlier=None), dict(track_of_key=None),
             changed("key_ptr", 0, 1), changed("key_ptr", 3, 1), changed("corr_ptr", 0, 1), changed("corr_ptr", 2, 0), changed("corr_key", 0, 13), changed("corr_key", 0, -1),
             changed("track_of_key", 0, 8), changed("track_of_key", 0, -2), changed("track_outlier", 0, 1), dict(track_of_key=same_frame), dict(corr_key=own),
             changed("corr_key", 0, ix["z5"]), changed("cam_q", (1, 2), np.nan), changed("cam_t", (0, 0), np.inf), changed("points", (3, 1), np.nan),
             changed("key_xy", (4, 0), -np.inf), changed("intr_params", (0, 7), np.nan), changed("cam_intr", 2, 1), changed("cam_intr", 2, -1), changed("intr_model", 0, 5),
             changed("intr_model", 0, -1)]
    for kw in cases:
        capfd.readouterr()
        code, untouched = c.run(lib, **kw)
        err = capfd.readouterr().err
        assert code == capi.EINVAL and _one_line(err, "xrsfm_ba_merge_tracks") and untouched, (kw, code, err)
    capfd.readouterr()
    assert lib.xrsfm_ba_debug_merge_components(None, 0, *([None] * 6), 0, *([None] * 4), 0, *([None] * 5)) == capi.EINVAL and _one_line(capfd.readouterr().err, "xrsfm_ba_debug_merge_components")


def test_nothing_to_do_is_success_without_a_device(lib):
    from xrsfm_amd import capi
    z = lambda t, *s: np.zeros(s or (0,), t)
    r = capi.merge_tracks(np.zeros(1, np.int64), z(np.float64, 0, 2), z(np.uint8), z(np.float64, 0, 4), z(np.float64, 0, 3), z(np.int32), z(np.int32), z(np.float64, 0, 8),
                          np.zeros(1, np.int64), z(np.int32), z(np.float64, 0, 3), z(np.uint8), z(np.int32))
    assert len(r["track_of_key"]) == 0 and r["stats"]["components"] == 0
    c = MC.case("live")
    a = list(MC.arrays(c))
    # no track at all; frame mode on a frame that carries no track
    none = capi.merge_tracks(*a[:10], z(np.float64, 0, 3), z(np.uint8), np.full(len(c["track_of_key"]), -1, np.int32))
    assert none["visible"].tolist() == [0] * 6 and none["corr_have_point3d"].tolist() == [0] * 13
    tok = c["track_of_key"].copy()
    tok[c["key_ptr"][2]:c["key_ptr"][3]] = -1
    r = capi.merge_tracks(*a[:12], tok, options=capi.merge_options(mode=4, frame=2))
    want = Y.run_components(dict(c, track_of_key=tok), 4)
    assert Y.integer_differences(dict(r, stats=np.array(list(r["stats"].values()) + [0])), want) == [] and want["stats"].tolist() == [0] * 8
    assert np.array_equal(r["points"], c["points"]) and r["measured"].sum() == (tok >= 0).sum() > 0


def test_real_work_without_a_device_is_enodev(lib):
    import torch
    from xrsfm_amd import capi
    if torch.cuda.is_available() and capi.device_count() > 0:
        pytest.skip("a GPU is present")
    c = _Call()
    code, untouched = c.run(lib)
    assert code == -2 and untouched
    with pytest.raises(RuntimeError, match="ENODEV"):
        capi.merge_tracks(*MC.arrays(MC.case("rules")))


# ---------------------------------------------------------------------------------------------------- the code object
def test_merge_kernels_do_not_spill(tmp_path):
    """the kernels of ba_merge.h in the gfx950 code object: no spilled register, no private (scratch) segment; the static LDS of
    k_merge_components is the 20.5 KiB of DESIGN.md 5r: seven one-wave workgroups fit a compute unit's 160 KiB"""
    from xrsfm_amd import _build
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = tmp_path / "merge_only.hip"
    src.write_text('#include <hip/hip_runtime.h>\n#include "ba_merge.h"\n')
    asm = tmp_path / "merge.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-I", _build.CSRC, str(src), "-o", str(asm)], check=True, capture_output=True)
    seen = {}
    for blk in asm.read_text().split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        m = re.search(r"k_merge_(components|counts)", name)
        if not m:
            continue
        num = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, blk).group(1))
        fig = dict(vgpr=num("vgpr_count"), sgpr=num("sgpr_count"), lds=num("group_segment_fixed_size"), scratch=num("private_segment_fixed_size"), spill=num("vgpr_spill_count"),
                   sspill=num("sgpr_spill_count"))
        seen[m.group(1)] = fig
        assert fig["spill"] == 0 and fig["sspill"] == 0 and fig["scratch"] == 0 and fig["vgpr"] <= 128, (name, fig)
    print("track merge kernels:", seen)
    assert sorted(seen) == ["components", "counts"]
    lds = 8 * 3 * 512 + 4 * 1024 + 2 * 1024 + 2 * 512 + 1024 + 512
    assert {k: v["lds"] for k, v in seen.items()} == dict(components=lds, counts=2 * 4 * 4) and lds == 20992 and 7 * lds <= 160 * 1024 < 8 * lds
