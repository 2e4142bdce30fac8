"""Match expansion without a GPU: the two formulations of the yardstick agree on the whole catalogue, the catalogue's
table shows every rule exercised, the host half of the library (the tracks) and ba_expand_rule.h as a stand-alone program built with
the address and undefined-behaviour sanitizers equal the yardstick on every rule, every EINVAL comes before a device is needed with one
line on stderr and untouched outputs, real work without a device is ENODEV, and the new kernels neither spill nor use scratch."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import expand_cases as EC
from tests import expand_host_driver as HD
from tests import expand_yardstick as Y

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("xrsfm_ba_expand_options_default", "xrsfm_ba_expand_candidates", "xrsfm_ba_frames_expand", "xrsfm_ba_debug_expand_tracks", "xrsfm_ba_debug_expand_covis")
p = lambda a, t: a.ctypes.data_as(C.POINTER(t)) if a is not None else None


def _one_line(err, name):
    return err.count("\n") == 1 and name in err


def test_the_new_symbols_are_declared_and_exported(lib):
    from xrsfm_amd import capi
    hdr = open(os.path.join(ROOT, "include", "xrsfm_ba.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in capi.EXPORTS and getattr(lib, name) is not None, name
    for word in ("is not computed", "XRSFM_BA_EXPAND_WINDOW", "no output is touched"):
        assert word in hdr, word
    o = capi.expand_options()
    assert {k: getattr(o, k) for k, _ in o._fields_} == Y.DEFAULTS
    assert C.sizeof(capi.CExpandOptions) == 48


# ---------------------------------------------------------------------------------------------------- the yardstick and the catalogue
@pytest.mark.parametrize("name", EC.NAMES)
def test_the_two_formulations_agree(name):
    c = EC.case(name)
    assert 8 <= c["n"] <= 70 and np.diff(c["key_ptr"]).max() <= 200
    assert Y.same(EC.expected(name), Y.arrays(c)) == []


# the rules each constructed case is there for (tests/expand_cases.py); the ring scenes add breadth and two of the bit-set rules
WANTED = {
    "chain": ("one frame per round, three rounds or more", "a frame ends at exactly min_visible", "a frame ends one below min_visible", "a (frame, patch) seen once",
              "a (frame, patch) seen twice", "a third frame skipped because it is paired", "a key point at x == width", "a frame in its own rank list",
              "a pair proposed from both directions", "a tried pair among the ranked", "a covisibility pair"),
    "tracks": ("AddTrack: a new track", "AddTrack: the first key point joins", "AddTrack: the second key point joins", "AddTrack: a merge",
               "AddTrack: a same-frame conflict in a merge", "AddTrack: insert does not overwrite", "a key point points at an invalid track", "GetMatcheNum differs by direction"),
    "rounds": ("two frames of one round are paired", "the initial pair is stored backwards", "a key point with correspondents in two registered frames", "a second component",
               "a frame without key points", "an initial frame ends below min_visible", "a frame ends at exactly min_visible"),
    "shared": ("exactly max_shared_matches shared", "one above max_shared_matches shared"),
    "star": ("a frame index of 32 or more", "an id twice in a rank list", "may register at exactly mayreg_count_mid", "may register at one below mid and exactly the sum",
             "does not register at one below mid and one below the sum", "a similarity pair at exactly similarity_rank_max", "no similarity pair one rank beyond",
             "a similarity pair", "a tried pair among the ranked"),
    "ring33": ("a frame index of 32 or more", "AddTrack: a merge"),
    "ring65": ("a frame index of 64 or more", "AddTrack: a merge"),
}


def test_every_rule_is_exercised():
    table = {name: EC.coverage(name) for name in EC.NAMES}
    rules = list(table[EC.NAMES[0]])
    for name, wanted in WANTED.items():
        for rule in wanted:
            assert table[name][rule], (name, rule)
    uncovered = [r for r in rules if not any(table[n][r] for n in EC.NAMES)]
    assert uncovered == []
    for name in EC.NAMES:
        print("%-8s %s" % (name, "".join("x" if table[name][r] else "." for r in rules)))
    o = Y.options(EC.case("star"))
    assert o == Y.DEFAULTS and all(Y.options(EC.case(n))["min_visible"] <= 3 for n in EC.NAMES if n != "star")


def test_the_two_stages_and_both_verdicts_of_every_test_occur():
    """over the catalogue a directed candidate fails on shared matches, fails on patches and passes; frames may register and may not"""
    rows = [(EC.case(n), row) for n in EC.NAMES for row in EC.expected(n)["cand"]]
    o = lambda c: Y.options(c)
    assert any(sh > o(c)["max_shared_matches"] for c, (_, _, sh, _) in rows)
    assert any(sh <= o(c)["max_shared_matches"] and cv < o(c)["min_covisible_patches"] for c, (_, _, sh, cv) in rows)
    assert any(sh <= o(c)["max_shared_matches"] and cv >= o(c)["min_covisible_patches"] for c, (_, _, sh, cv) in rows)
    r = EC.expected("star")
    assert sum(r["may_register"]) == 2 and r["may_register"][41] and r["may_register"][42] and not r["may_register"][43]


# ---------------------------------------------------------------------------------------------------- the library's host half
@pytest.mark.parametrize("name", EC.NAMES)
def test_the_tracks_equal_the_yardstick(lib, name):
    from xrsfm_amd import capi
    c, r = EC.case(name), EC.expected(name)
    t = capi.debug_expand_tracks(c["key_ptr"], c["pair_a"], c["pair_b"], c["match_ptr"], c["matches"])
    assert np.array_equal(t["key_track"], np.array(r["key_track"], np.int32))
    tp = t["track_ptr"]
    got = [(list(zip(t["obs_frame"][tp[k]:tp[k + 1]].tolist(), t["obs_key"][tp[k]:tp[k + 1]].tolist())), bool(t["invalid"][k])) for k in range(len(tp) - 1)]
    assert got == [(list(obs), bool(inv)) for obs, inv in r["tracks"]]


# ---------------------------------------------------------------------------------------------------- the rule header, sanitized
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return HD.build(tmp_path_factory.mktemp("expand_rule"))


@pytest.mark.parametrize("name", EC.NAMES)
def test_the_rule_header_equals_the_yardstick(driver, name):
    c, r = EC.case(name), EC.expected(name)
    o = Y.options(c)
    out = HD.run(driver, HD.case_input(c, o))
    assert "fault" not in out
    assert out["patch"] == [q for f in Y.patches_of(c, o) for q in f]
    assert out["key_track"] == r["key_track"]
    tp = out["track_ptr"]
    assert [(list(zip(out["obs_frame"][tp[k]:tp[k + 1]], out["obs_key"][tp[k]:tp[k + 1]])), bool(out["invalid"][k])) for k in range(len(tp) - 1)] == \
        [(list(obs), bool(inv)) for obs, inv in r["tracks"]]
    for k in ("connected", "visible", "registered", "may_register"):
        assert out[k] == [int(x) for x in r[k]], k
    assert out["rounds"] == [r["rounds"]]
    cp = out["code_ptr"]
    codes = [out["codes"][cp[f]:cp[f + 1]] for f in range(c["n"])]
    assert codes == r["codes"]
    assert all(len(codes[f]) <= out["items"][f] // o["min_patch_obs"] for f in range(c["n"]))          # the room the host gives a frame's codes
    assert out["cand"] == [x for row in r["cand"] for x in row]
    assert list(zip(out["out_a"], out["out_b"], out["out_source"])) == r["pairs"]


def test_the_window_split(driver):
    c = EC.case("ring65")
    o = Y.options(c)
    w = lambda lds, forced: HD.run(driver, HD.case_input(c, o, lds, forced))["window"]
    fixed = 4 * 3                                                      # 65 frames: three words of paired bits
    assert w(160 * 1024 - 2048, 0) == [65, 1] and w(160 * 1024 - 2048, 1) == [1, 65] and w(160 * 1024 - 2048, 3) == [3, 22]
    assert w(fixed + 32 * 8, 0) == [8, 9] and w(fixed + 32 * 8 + 31, 0) == [8, 9] and w(fixed + 31, 0) == [0, 0] and w(fixed + 32 * 8, 100) == [8, 9]


def test_the_rule_header_refuses_what_the_entries_refuse(driver):
    c = EC.case("rounds")
    o = Y.options(c)
    for bad, word in ((dict(patch_cols=16), "patch_cols"), (dict(min_patch_obs=3), "min_patch_obs"), (dict(min_visible=0), "min_visible"), (dict(mayreg_rank_mid=2), "ascending"),
                      (dict(max_shared_matches=-1), "negative")):
        assert word in " ".join(HD.run(driver, HD.case_input(c, dict(o, **bad)))["fault"]), bad
    neg = dict(c, keys=c["keys"].copy())
    neg["keys"][4, 0] = -64.0                                          # (int)x / step is -1
    assert HD.run(driver, HD.case_input(neg, o))["fault"] == ["patch"]
    neg["keys"][4, 0] = -63.0                                          # ... and 0 here: the reference's division truncates toward zero
    assert "fault" not in HD.run(driver, HD.case_input(neg, o))
    twice = dict(c, pair_a=np.append(c["pair_a"], 0).astype(np.int32), pair_b=np.append(c["pair_b"], 1).astype(np.int32), match_ptr=np.append(c["match_ptr"], c["match_ptr"][-1]))
    assert HD.run(driver, HD.case_input(twice, o))["fault"] == ["twice"]
    assert HD.run(driver, HD.case_input(dict(c, init=(6, 7)), o))["fault"] == ["init"]


# ---------------------------------------------------------------------------------------------------- the entries' argument checks
class _Call:
    """one xrsfm_ba_expand_candidates call on the `rounds` case, every output at a fill value"""

    def __init__(self):
        from xrsfm_amd import capi
        c = EC.case("rounds")
        self.a = dict(opt=capi.expand_options(min_visible=3), n=c["n"], key_ptr=c["key_ptr"].copy(), keys=c["keys"].copy(), w=np.ascontiguousarray(c["sizes"][:, 0]),
                      h=np.ascontiguousarray(c["sizes"][:, 1]), n_pairs=len(c["pair_a"]), pa=c["pair_a"].copy(), pb=c["pair_b"].copy(), mp=c["match_ptr"].copy(),
                      m=c["matches"].copy(), rp=c["rank_ptr"].copy(), ri=c["rank_ids"].copy(), n_tried=1, ta=np.array([2], np.int32), tb=np.array([6], np.int32), ia=0, ib=1,
                      cap=len(c["rank_ids"]), cand_cap=len(c["rank_ids"]))
        self.fill()

    def fill(self):
        n, cap = self.a["n"], 200
        self.out = dict(n_out=np.full(1, -77, np.int64), oa=np.full(cap, -77, np.int32), ob=np.full(cap, -77, np.int32), src=np.full(cap, 77, np.uint8),
                        con=np.full(n, 77, np.uint8), reg=np.full(n, 77, np.uint8), may=np.full(n, 77, np.uint8), vis=np.full(n, -77, np.int32),
                        n_cand=np.full(1, -77, np.int64), cand=np.full((cap, 4), -77, np.int32), stats=np.full(8, -77, np.int64))

    def untouched(self):
        return all(np.all(v == (77 if v.dtype == np.uint8 else -77)) for v in self.out.values())

    def run(self, lib, null=(), **kw):
        self.fill()
        a = dict(self.a, **kw)
        o = {k: (None if k in null else v) for k, v in self.out.items()}
        i32, i64, u8 = C.c_int32, C.c_int64, C.c_uint8
        return lib.xrsfm_ba_expand_candidates(C.byref(a["opt"]) if a["opt"] is not None else None, a["n"], p(a["key_ptr"], i64), p(a["keys"], C.c_float), p(a["w"], i32),
                                              p(a["h"], i32), a["n_pairs"], p(a["pa"], i32), p(a["pb"], i32), p(a["mp"], i64), p(a["m"], i32), p(a["rp"], i64), p(a["ri"], i32),
                                              a["n_tried"], p(a["ta"], i32), p(a["tb"], i32), a["ia"], a["ib"], a["cap"], p(o["n_out"], i64), p(o["oa"], i32), p(o["ob"], i32),
                                              p(o["src"], u8), p(o["con"], u8), p(o["reg"], u8), p(o["may"], u8), p(o["vis"], i32), a["cand_cap"], p(o["n_cand"], i64),
                                              p(o["cand"], i32), p(o["stats"], i64))


def test_candidates_refuses_bad_arguments_before_a_device_is_needed(lib, capfd):
    from xrsfm_amd import capi
    c = _Call()
    a = c.a
    eo = capi.expand_options

    def changed(key, index, value):
        v = a[key].copy()
        v[index] = value
        return {key: v}

    cases = [dict(opt=None), dict(opt=eo(patch_cols=16)), dict(opt=eo(patch_rows=0)), dict(opt=eo(min_patch_obs=3)), dict(opt=eo(min_visible=0)),
             dict(opt=eo(max_shared_matches=-1)), dict(opt=eo(mayreg_rank_mid=4)), dict(n=-1), dict(n_pairs=-1), dict(n_tried=-1), dict(key_ptr=None),
             changed("key_ptr", 0, 1), changed("key_ptr", 3, 5), dict(w=None), dict(h=None), changed("w", 3, 9), changed("h", 11, 9), dict(keys=None),
             changed("keys", (4, 0), -64.0), changed("keys", (4, 1), np.nan), changed("keys", (4, 0), np.inf), changed("keys", (4, 0), 3e9), dict(pa=None), dict(pb=None),
             dict(mp=None), changed("mp", 0, 1), changed("mp", 2, 2), dict(m=None), changed("pa", 1, 12), changed("pb", 1, -1), changed("pb", 1, 1),
             changed("pb", 1, 0), changed("m", (0, 0), 6), changed("m", (0, 1), -1), dict(rp=None), changed("rp", 1, 100), dict(ri=None), changed("ri", 5, 12),
             dict(ta=None), changed("ta", 0, 12), changed("tb", 0, -1), dict(ia=12), dict(ib=-1), dict(ia=6, ib=7), dict(ia=2, ib=3), dict(cap=-1), dict(cand_cap=-1)]
    for kw in cases:
        capfd.readouterr()
        code = c.run(lib, **kw)
        err = capfd.readouterr().err
        assert code == capi.EINVAL and _one_line(err, "xrsfm_ba_expand_candidates") and c.untouched(), (kw, code, err)
    for null in (("n_out",), ("oa",), ("ob",), ("src",), ("n_cand",)):
        capfd.readouterr()
        code = c.run(lib, null=null)
        assert code == capi.EINVAL and _one_line(capfd.readouterr().err, "xrsfm_ba_expand_candidates") and c.untouched(), null


def test_the_other_entries_refuse_bad_arguments(lib, capfd):
    from xrsfm_amd import capi
    c = EC.case("rounds")
    i32, i64 = C.c_int32, C.c_int64
    o = capi.expand_options(min_visible=3)
    # a NULL frame set
    capfd.readouterr()
    assert lib.xrsfm_ba_frames_expand(None, C.byref(o), *([None] * 2), 0, *([None] * 6), 0, None, None, 0, 1, 0, None, None, None, None, None, None, None, None, 0, None, None,
                                      None) == capi.EINVAL
    assert _one_line(capfd.readouterr().err, "xrsfm_ba_frames_expand")
    # the tracks: a bad index, capacities below the need (the line names it)
    M = len(c["matches"])
    kt = np.full(int(c["key_ptr"][-1]), -77, np.int32); tp = np.full(M + 1, -77, np.int64); inv = np.full(M, 77, np.uint8)
    of, ok = np.full(2 * M, -77, np.int32), np.full(2 * M, -77, np.int32)
    nt, no = np.full(1, -77, np.int64), np.full(1, -77, np.int64)

    def tracks(pa=c["pair_a"], tcap=M, ocap=2 * M):
        capfd.readouterr()
        code = lib.xrsfm_ba_debug_expand_tracks(c["n"], p(c["key_ptr"], i64), len(pa), p(pa, i32), p(c["pair_b"], i32), p(c["match_ptr"], i64), p(c["matches"], i32), p(kt, i32),
                                                tcap, p(nt, i64), p(tp, i64), p(inv, C.c_uint8), ocap, p(no, i64), p(of, i32), p(ok, i32))
        return code, capfd.readouterr().err

    bad = c["pair_a"].copy(); bad[0] = 12
    for kw in (dict(pa=bad), dict(tcap=1), dict(ocap=1), dict(tcap=-1)):
        code, err = tracks(**kw)
        assert code == capi.EINVAL and _one_line(err, "xrsfm_ba_debug_expand_tracks"), kw
        assert all(np.all(v == (77 if v.dtype == np.uint8 else -77)) for v in (kt, tp, inv, of, ok, nt, no))
    _, err = tracks(tcap=1)
    want = capi.debug_expand_tracks(c["key_ptr"], c["pair_a"], c["pair_b"], c["match_ptr"], c["matches"])
    assert "%d tracks" % len(want["invalid"]) in err and "%d observations" % len(want["obs_frame"]) in err
    # the codes: options out of range
    cp = np.full(c["n"] + 1, -77, np.int64); codes = np.full(64, -77, np.int32)
    capfd.readouterr()
    bo = capi.expand_options(patch_cols=16)
    code = lib.xrsfm_ba_debug_expand_covis(C.byref(bo), c["n"], p(c["key_ptr"], i64), p(c["keys"], C.c_float), p(np.ascontiguousarray(c["sizes"][:, 0]), i32),
                                           p(np.ascontiguousarray(c["sizes"][:, 1]), i32), len(c["pair_a"]), p(c["pair_a"], i32), p(c["pair_b"], i32), p(c["match_ptr"], i64),
                                           p(c["matches"], i32), 0, 1, 64, p(cp, i64), p(codes, i32))
    assert code == capi.EINVAL and _one_line(capfd.readouterr().err, "xrsfm_ba_debug_expand_covis") and np.all(cp == -77) and np.all(codes == -77)


def test_no_frames_is_success_with_nothing_out(lib):
    from xrsfm_amd import capi
    z = lambda t: np.zeros(0, t)
    r = capi.expand_candidates(np.zeros(1, np.int64), np.zeros((0, 4), np.float32), np.zeros((0, 2), np.int32), z(np.int32), z(np.int32), np.zeros(1, np.int64),
                               np.zeros((0, 2), np.int32), np.zeros(1, np.int64), z(np.int32), 0, 0)
    assert len(r["pair_a"]) == 0 and len(r["cand"]) == 0 and len(r["connected"]) == 0 and r["stats"]["rounds"] == 0
    t = capi.debug_expand_tracks(np.zeros(1, np.int64), z(np.int32), z(np.int32), np.zeros(1, np.int64), np.zeros((0, 2), np.int32))
    assert len(t["key_track"]) == 0 and t["track_ptr"].tolist() == [0]
    with capi.frames_create(np.zeros(1, np.int64), np.zeros((0, 4), np.float32), np.zeros((0, 128), np.uint8)) as fs:
        r = capi.frames_expand(fs, np.zeros((0, 2), np.int32), z(np.int32), z(np.int32), np.zeros(1, np.int64), np.zeros((0, 2), np.int32), np.zeros(1, np.int64), z(np.int32), 0, 0)
        assert len(r["pair_a"]) == 0


def test_real_work_without_a_device_is_enodev(lib):
    import torch
    from xrsfm_amd import capi
    if torch.cuda.is_available() and capi.device_count() > 0:
        pytest.skip("a GPU is present")
    c = _Call()
    assert c.run(lib) == -2 and c.untouched()
    k = EC.case("rounds")
    with pytest.raises(RuntimeError, match="ENODEV"):
        capi.expand_candidates(k["key_ptr"], k["keys"], k["sizes"], k["pair_a"], k["pair_b"], k["match_ptr"], k["matches"], k["rank_ptr"], k["rank_ids"], 0, 1,
                               options=capi.expand_options(min_visible=3))
    with pytest.raises(RuntimeError, match="ENODEV"):
        capi.debug_expand_covis(k["key_ptr"], k["keys"], k["sizes"], k["pair_a"], k["pair_b"], k["match_ptr"], k["matches"], 0, 1)
    # a set without key points exists without a device; its expansion has work to do (the pairs' rounds) and needs one
    empty = np.zeros(3, np.int64)
    with capi.frames_create(empty, np.zeros((0, 4), np.float32), np.zeros((0, 128), np.uint8)) as fs:
        with pytest.raises(RuntimeError, match="ENODEV"):
            capi.frames_expand(fs, np.array([(640, 480)] * 2, np.int32), [0], [1], np.zeros(2, np.int64), np.zeros((0, 2), np.int32), np.array([0, 1, 2], np.int64), [1, 0], 0, 1)


# ---------------------------------------------------------------------------------------------------- the code object
def test_expand_kernels_do_not_spill(tmp_path):
    """the kernels of ba_expand.h in the gfx950 code object: no spilled register, no private (scratch) segment; the static LDS of each
    (k_expand_covis adds its bit sets as dynamic LDS: 4 bytes per 32 frames and 32 bytes per third frame of a pass)"""
    from xrsfm_amd import _build
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = tmp_path / "expand_only.hip"
    src.write_text('#include <hip/hip_runtime.h>\n#include "ba_expand.h"\n')
    asm = tmp_path / "expand.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-I", _build.CSRC, str(src), "-o", str(asm)], check=True, capture_output=True)
    seen = {}
    for blk in asm.read_text().split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        m = re.search(r"k_expand_(patch|count|fill|select|fire|covis|pairs)", name)
        if not m:
            continue
        num = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, blk).group(1))
        fig = dict(vgpr=num("vgpr_count"), sgpr=num("sgpr_count"), lds=num("group_segment_fixed_size"), scratch=num("private_segment_fixed_size"), spill=num("vgpr_spill_count"),
                   sspill=num("sgpr_spill_count"))
        seen[m.group(1)] = fig
        assert fig["spill"] == 0 and fig["sspill"] == 0 and fig["scratch"] == 0 and fig["vgpr"] <= 64, (name, fig)
    print("match expansion kernels:", seen)
    assert sorted(seen) == ["count", "covis", "fill", "fire", "pairs", "patch", "select"]
    assert {k: v["lds"] for k, v in seen.items()} == dict(patch=0, count=0, fill=0, select=0, fire=0, covis=256 * 4, pairs=0)
    assert 256 * 4 + 160 * 1024 - 2048 <= 160 * 1024                   # static + the most dynamic LDS the host asks for
