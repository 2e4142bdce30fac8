"""Match expansion on the GPU.  Everything the search produces is an integer and every comparison is np.array_equal
against tests/expand_yardstick.py on the catalogue of tests/expand_cases.py (8 - 65 frames, at most 1240 key points a case: the
smallest shapes at which each rule can go wrong, three of them crossing the words of the kernels' bit sets)."""
import os

import numpy as np
import pytest

from tests import expand_cases as EC
from tests import expand_yardstick as Y

pytestmark = pytest.mark.gpu
FIELDS = ("pair_a", "pair_b", "source", "connected", "registered", "may_register", "visible", "cand")


def _capi():
    from xrsfm_amd import capi
    return capi


class _env:
    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        self.old = os.environ.get(self.name)
        if self.value is None:
            os.environ.pop(self.name, None)
        else:
            os.environ[self.name] = self.value

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop(self.name, None)
        else:
            os.environ[self.name] = self.old


def _options(c):
    return _capi().expand_options(**c.get("opt", {}))


def _run(c, **kw):
    return _capi().expand_candidates(c["key_ptr"], c["keys"], c["sizes"], c["pair_a"], c["pair_b"], c["match_ptr"], c["matches"], c["rank_ptr"], c["rank_ids"],
                                     c["init"][0], c["init"][1], c["tried"], _options(c), **kw)


def _want(r):
    """the yardstick's result in the interface's arrays"""
    pairs = np.array(r["pairs"], np.int32).reshape(-1, 3)
    return dict(pair_a=pairs[:, 0].copy(), pair_b=pairs[:, 1].copy(), source=pairs[:, 2].astype(np.uint8), connected=np.array(r["connected"], np.uint8),
                registered=np.array(r["registered"], np.uint8), may_register=np.array(r["may_register"], np.uint8), visible=np.array(r["visible"], np.int32),
                cand=np.array(r["cand"], np.int32).reshape(-1, 4))


def _differ(got, want, fields=FIELDS):
    return [k for k in fields if got[k].dtype != want[k].dtype or got[k].shape != want[k].shape or not np.array_equal(got[k], want[k])]


@pytest.mark.parametrize("name", EC.NAMES)
def test_every_output_equals_the_yardstick(lib, name):
    c, r = EC.case(name), EC.expected(name)
    got = _run(c)
    assert _differ(got, _want(r)) == []
    s = got["stats"]
    valid = sum(1 for _, inv in r["tracks"] if not inv)
    assert (s["rounds"], s["tracks"], s["valid_tracks"], s["corr_entries"], s["passes"]) == (r["rounds"], len(r["tracks"]), valid, 2 * len(c["matches"]), 1)
    assert s["codes_kept"] == sum(len(x) for x in r["codes"])
    slim = _run(c, with_cand=False)                                    # the candidate rows are optional
    assert _differ(slim, _want(r), FIELDS[:-1]) == [] and "cand" not in slim


@pytest.mark.parametrize("name", EC.NAMES)
def test_the_codes_equal_the_yardstick(lib, name):
    c, r = EC.case(name), EC.expected(name)
    cp, codes = _capi().debug_expand_covis(c["key_ptr"], c["keys"], c["sizes"], c["pair_a"], c["pair_b"], c["match_ptr"], c["matches"], c["init"][0], c["init"][1], _options(c))
    assert np.array_equal(cp, np.concatenate([[0], np.cumsum([len(x) for x in r["codes"]])]))
    assert np.array_equal(codes, np.array([x for f in r["codes"] for x in f], np.int32))


def test_min_patch_obs_of_one_compacts_the_first_bit_set(lib):
    c = dict(EC.case("ring33"), opt=dict(EC.case("ring33")["opt"], min_patch_obs=1))
    assert _differ(_run(c), _want(Y.literal(c))) == []


@pytest.mark.parametrize("name", ("chain", "star", "ring65"))
def test_small_windows_give_identical_bits(lib, name):
    """one third frame per pass, three, and all of them: the codes, the counts and the pairs do not move"""
    c = EC.case(name)
    args = (c["key_ptr"], c["keys"], c["sizes"], c["pair_a"], c["pair_b"], c["match_ptr"], c["matches"], c["init"][0], c["init"][1], _options(c))
    with _env("XRSFM_BA_EXPAND_WINDOW", None):
        whole, codes = _run(c), _capi().debug_expand_covis(*args)
    for w in ("1", "3"):
        with _env("XRSFM_BA_EXPAND_WINDOW", w):
            got, cw = _run(c), _capi().debug_expand_covis(*args)
        assert _differ(got, whole) == [] and np.array_equal(cw[0], codes[0]) and np.array_equal(cw[1], codes[1])
        assert got["stats"]["passes"] == -(-c["n"] // int(w)) and got["stats"]["codes_kept"] == whole["stats"]["codes_kept"]
    assert _differ(whole, _want(EC.expected(name))) == []


def test_a_second_call_returns_the_same_bits_and_leaves_the_cache_as_it_was(lib):
    capi = _capi()
    c = EC.case("ring33")
    capi.quiesce()                                                     # empties the device cache and the pinned pool
    first = _run(c)
    c1 = capi.quiesce()
    second = _run(c)
    c2 = capi.quiesce()
    assert _differ(second, first) == [] and second["stats"] == first["stats"]
    assert c1 > 0 and c2 == c1                                         # the call's blocks came back to the cache, and nothing was kept


@pytest.mark.parametrize("name", ("rounds", "ring33"))
def test_a_resident_set_gives_what_host_arrays_give(lib, name):
    """frames_expand reads the key points the set holds: no key point goes up (a set made by frames_create; `rounds` has frames without
    key points)"""
    capi = _capi()
    c = EC.case(name)
    desc = np.zeros((len(c["keys"]), 128), np.uint8)
    with capi.frames_create(c["key_ptr"], c["keys"], desc) as fs:
        got = capi.frames_expand(fs, c["sizes"], c["pair_a"], c["pair_b"], c["match_ptr"], c["matches"], c["rank_ptr"], c["rank_ids"], c["init"][0], c["init"][1], c["tried"],
                                 _options(c))
    assert _differ(got, _run(c)) == [] and _differ(got, _want(EC.expected(name))) == []


def test_a_resident_key_point_outside_its_patches_is_refused(lib):
    capi = _capi()
    c = EC.case("rounds")
    keys = c["keys"].copy()
    keys[4, 0] = -64.0
    with capi.frames_create(c["key_ptr"], keys, np.zeros((len(keys), 128), np.uint8)) as fs:
        with pytest.raises(RuntimeError, match="EINVAL"):
            capi.frames_expand(fs, c["sizes"], c["pair_a"], c["pair_b"], c["match_ptr"], c["matches"], c["rank_ptr"], c["rank_ids"], 0, 1, c["tried"], _options(c))


def test_expansion_and_matching_equals_the_loop_with_the_yardsticks_search(lib):
    """two iterations of ExpansionAndMatching on six views of one scene: the loop with frames_expand and the same loop with the yardstick
    in its place try the same pairs and keep the same matches"""
    capi = _capi()
    ptr, keys, desc, sizes, rp, ri = EC.loop_scene()
    opt = capi.expand_options(**EC.LOOP_OPT)

    def yardstick(frames, sizes, pa, pb, mp, m, rank_ptr, rank_ids, init_a, init_b, tried, options):
        c = dict(n=len(ptr) - 1, key_ptr=ptr, keys=keys, sizes=sizes, pair_a=pa, pair_b=pb, match_ptr=mp, matches=m, rank_ptr=rank_ptr, rank_ids=rank_ids, tried=tried,
                 init=(init_a, init_b), opt=EC.LOOP_OPT)
        pairs = np.array(Y.literal(c)["pairs"], np.int32).reshape(-1, 3)
        return dict(pair_a=pairs[:, 0], pair_b=pairs[:, 1])

    with capi.frames_create(ptr, keys, desc) as fs:
        got = capi.expansion_and_matching(fs, sizes, rp, ri, EC.LOOP_INIT_PAIRS, 0, 1, 2, opt)
        want = capi.expansion_and_matching(fs, sizes, rp, ri, EC.LOOP_INIT_PAIRS, 0, 1, 2, opt, expand=yardstick)
    for k in ("pair_a", "pair_b", "match_ptr", "matches", "tried"):
        assert np.array_equal(got[k], want[k]), k
    assert got["iterations"] == want["iterations"]
    log = got["iterations"]
    print("iterations:", log)
    assert log[0]["accepted"] == len(EC.LOOP_INIT_PAIRS) and log[1]["candidates"] > 0 and log[1]["accepted"] > 0 and len(got["pair_a"]) > len(EC.LOOP_INIT_PAIRS)
