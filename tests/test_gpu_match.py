"""xrsfm_ba_match_descriptors on the GPU against the yardstick (tests/match_yardstick.py), with exact equality
throughout: the whole catalogue, the triples of xrsfm_ba_debug_match_top2, bit-identical outputs across batches, orders, calls and
workspace splits, untouched outputs, and match_descriptors -> matched_points -> verify_pairs -> verified_matches -> two_view_init
recovering the generating relative pose."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import match_yardstick as Y

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("match_ptr", "matches", "num_row", "num_col")


def _capi():
    from xrsfm_amd import capi
    return capi


def _run(ks, opt=None):
    """the entries ks (of one option set) in one call"""
    capi = _capi()
    ptr, desc, pa, pb = Y.call_arrays(ks)
    o = Y.entries()[ks[0]]["opt"] if opt is None else opt
    return capi.match_descriptors(ptr, desc, pa, pb, capi.match_options(**o))


def _pairs(r):
    """a call's result as one tuple of arrays per pair"""
    mp = r["match_ptr"]
    return [(r["matches"][mp[i]:mp[i + 1]], r["num_row"][i], r["num_col"][i]) for i in range(len(mp) - 1)]


def _same(a, b):
    return np.array_equal(a[0], b[0]) and a[1] == b[1] and a[2] == b[2]


@pytest.fixture(scope="module")
def library_results():
    """the catalogue through the library, one call per option set: entry -> (matches, num_row, num_col)"""
    out = {}
    for opt, ks in Y.option_groups().items():
        r = _run(ks)
        want = Y.expected(ks)
        for f in FIELDS:
            assert r[f].dtype == want[f].dtype and np.array_equal(r[f], want[f]), (opt, f)
        out.update(zip(ks, _pairs(r)))
    return out


def test_library_equals_the_yardstick_on_the_whole_catalogue(library_results):
    E = Y.entries()
    assert len(library_results) == len(E)
    for k, got in library_results.items():
        want = Y.reference(k)
        assert _same(got, (want["matches"], want["num_row"], want["num_col"])), E[k]["tag"]
    assert sum(len(g[0]) for g in library_results.values()) == sum(len(Y.reference(k)["matches"]) for k in range(len(E))) >= 1000


def test_top2_triples_equal_the_yardstick():
    """(best, idx, next) of every row and column: the integers the match list cannot show (the idx of a tied best, the next of a
    rejected row), and the orientation of the matrix instruction's result on asymmetric data"""
    capi, F, E = _capi(), Y.frames(), Y.entries()
    seen = set()
    for k, e in enumerate(E):
        if (e["a"], e["b"]) in seen or e["opt"].get("max_features"):
            continue
        seen.add((e["a"], e["b"]))
        want = Y.reference(k)
        rt, ct = capi.debug_match_top2(F[e["a"]], F[e["b"]])
        assert np.array_equal(rt, want["row_top"]) and np.array_equal(ct, want["col_top"]), e["tag"]
    assert len(seen) >= 160
    # asymmetric integers: one-hot rows of different weights, score(i, j) = (i + 1) (2 j + 3) on the diagonal block only
    a, b = np.zeros((40, Y.DIM), np.uint8), np.zeros((70, Y.DIM), np.uint8)
    for i in range(40):
        a[i, i] = i + 1
    for j in range(70):
        b[j, j % 40] = 2 * j + 3
    want = Y.run_pair(a, b)
    rt, ct = capi.debug_match_top2(a, b)
    assert np.array_equal(rt, want["row_top"]) and np.array_equal(ct, want["col_top"])
    assert rt[5].tolist() == [6 * 93, 45, 6 * 13] and ct[45].tolist() == [6 * 93, 5, 0]


def test_a_pair_is_bit_identical_alone_in_batches_reversed_and_again(library_results):
    E = Y.entries()
    main = Y.main_group()
    again, rev, b257 = _pairs(_run(main)), _pairs(_run(main[::-1])), _pairs(_run(Y.batch257()))
    for i, k in enumerate(main):
        assert _same(again[i], library_results[k]) and _same(rev[len(main) - 1 - i], library_results[k]), E[k]["tag"]
    for i, k in enumerate(Y.batch257()):
        assert _same(b257[i], library_results[k]), E[k]["tag"]
    for k in main[5::17]:
        assert _same(_pairs(_run([k]))[0], library_results[k]), E[k]["tag"]


_SPLIT_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import torch  # noqa: F401
from tests import match_yardstick as Y
from xrsfm_amd import capi
ks = Y.main_group()
ptr, desc, pa, pb = Y.call_arrays(ks)
r = capi.match_descriptors(ptr, desc, pa, pb)
np.savez(sys.argv[2], **r)
"""


def test_workspace_split_does_not_change_a_bit(tmp_path):
    """XRSFM_BA_MATCH_WORKSPACE_MB = 1 in a fresh process: descriptors and workspace of the main group need several times the
    budget, so the call runs as many launches (a pair above the budget goes alone)"""
    script, out = tmp_path / "child.py", tmp_path / "r.npz"
    script.write_text(_SPLIT_CHILD)
    env = dict(os.environ, XRSFM_BA_MATCH_WORKSPACE_MB="1")
    subprocess.run([sys.executable, str(script), ROOT, str(out)], check=True, env=env, timeout=120)
    got, want = np.load(out), Y.expected(Y.main_group())
    for f in FIELDS:
        assert np.array_equal(got[f], want[f]), f


def test_untouched_outputs_on_an_error_and_on_a_small_capacity(capfd):
    capi = _capi()
    ks = [k for k, e in enumerate(Y.entries()) if e["tag"] in ("shape_129x257", "shape_65x64", "shape_0x17")]
    ptr, desc, pa, pb = Y.call_arrays(ks)
    want = Y.expected(ks)
    need = int(want["match_ptr"][-1])
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    lp = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))

    def call(cap, o, num=True):
        mp, m = np.full(len(ks) + 1, -77, np.int64), np.full((max(cap, 1), 2), -77, np.int32)
        nr, nc = np.full(len(ks), -77, np.int32), np.full(len(ks), -77, np.int32)
        code = capi.load().xrsfm_ba_match_descriptors(C.byref(o), len(ptr) - 1, lp(ptr), desc.ctypes.data_as(C.POINTER(C.c_uint8)), len(ks), ip(pa), ip(pb), cap,
                                                      lp(mp), ip(m), ip(nr) if num else None, ip(nc) if num else None)
        return code, mp, m, nr, nc
    capfd.readouterr()
    code, mp, m, nr, nc = call(need - 1, capi.match_options())
    err = capfd.readouterr().err
    assert code == capi.EINVAL and all(np.all(x == -77) for x in (mp, m, nr, nc)) and err.count("\n") == 1 and str(need) in err
    code, mp, m, nr, nc = call(need, capi.match_options(max_ratio=1.5))
    assert code == capi.EINVAL and all(np.all(x == -77) for x in (mp, m, nr, nc))
    code, mp, m, nr, nc = call(need, capi.match_options())                         # the exact capacity is enough
    assert code == 0 and np.array_equal(mp, want["match_ptr"]) and np.array_equal(m, want["matches"])
    assert np.array_equal(nr, want["num_row"]) and np.array_equal(nc, want["num_col"])
    code, mp, m, nr, nc = call(need + 3, capi.match_options(), num=False)          # NULL counts; rows past the matches stay
    assert code == 0 and np.array_equal(m[:need], want["matches"]) and np.all(m[need:] == -77) and np.all(nr == -77)


def test_match_verify_and_two_view_init_recover_the_generating_pose():
    """Keypoints projected from 3-D points into two views, descriptors perturbed between the views, 30 % of either frame unrelated:
    match_descriptors, matched_points, verify_pairs, verified_matches, normalisation by the known intrinsics, two_view_init.  The
    relative pose that generated the keypoints is recovered to the tolerance of the end-to-end test of tests/test_gpu_fund.py
    (1e-5); the baseline has no scale, so t is compared at unit length."""
    from tests import fund_yardstick as YF
    from tests import init_yardstick as YI
    capi = _capi()
    rng = np.random.default_rng(77)
    xa, xb, R, t = YF.make_pair(600, 0.0, 0.0, seed=4242, baseline=2.2)
    da = Y.sift_like(rng, 600)
    n_other = 257                                             # 30 % of each frame has no counterpart
    desc_a = np.concatenate([da, Y.sift_like(rng, n_other)])
    desc_b = np.concatenate([Y.perturb(rng, da), Y.sift_like(rng, n_other)])
    kp_a = np.concatenate([xa, rng.uniform(0, 2 * YF.K[0, 2], (n_other, 2))])
    kp_b = np.concatenate([xb, rng.uniform(0, 2 * YF.K[0, 2], (n_other, 2))])
    perm = rng.permutation(len(desc_b))                       # frame b in another order
    desc_b, kp_b = desc_b[perm], kp_b[perm]
    n = len(desc_a)
    r = capi.match_descriptors([0, n, 2 * n], np.concatenate([desc_a, desc_b]), [0], [1])
    inv = np.argsort(perm)
    assert len(r["matches"]) >= 590 and all(j == inv[i] for i, j in r["matches"].tolist() if i < 600)
    ma, mb = capi.matched_points(r, [0, n, 2 * n], np.concatenate([kp_a, kp_b]), [0], [1])
    ptr = r["match_ptr"].astype(np.int32)
    v = capi.verify_pairs(ptr, ma, mb)
    assert v["status"][0] == 1 and v["accepted"][0] == 1 and v["num_inliers"][0] >= 590
    kept, rows, new_ptr = capi.verified_matches(v, ptr, np.concatenate([ma, mb], 1))
    assert kept.tolist() == [0]
    na = (rows[:, 0:2] - YF.K[:2, 2]) / YF.FOCAL
    nb = (rows[:, 2:4] - YF.K[:2, 2]) / YF.FOCAL
    res = capi.two_view_init(new_ptr, na, nb, [10.0 / YF.FOCAL])
    assert res.status[0] == 1 and res.accepted[0] != 0
    Rg = np.asarray(YI.quat_to_mat(np.asarray(res.q[0], np.longdouble)), np.float64)
    tg, tt = res.t[0] / np.linalg.norm(res.t[0]), t / np.linalg.norm(t)
    print("relative pose: max |R - R_true| %.2e, |t - t_true| %.2e" % (np.abs(Rg - R).max(), np.abs(tg - tt).max()))
    assert np.abs(Rg - R).max() < 1e-5 and np.abs(tg - tt).max() < 1e-5
