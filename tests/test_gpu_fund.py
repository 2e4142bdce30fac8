"""xrsfm_ba_verify_pairs on the GPU against the yardstick (tests/fund_yardstick.py): the whole catalogue with the bars
of the CPU tests, bit-identical outputs across batches, orders and calls, per-pair max_error and seed, untouched outputs, NULL
optional outputs, and verify_pairs -> verified_matches -> two_view_init recovering the generating relative pose."""
import ctypes as C

import numpy as np
import pytest

from tests import fund_yardstick as Y
from tests.test_fund_cpu import check_against_yardstick

pytestmark = pytest.mark.gpu
FIELDS = ("status", "F", "inlier_mask", "num_inliers", "num_trials", "best_trial", "accepted")


def _capi():
    from xrsfm_amd import capi
    return capi


def _pair(r, ptr, i):
    """the outputs of pair i of a verify_pairs result, under the yardstick's names"""
    a, b = int(ptr[i]), int(ptr[i + 1])
    return dict(status=r["status"][i], F=r["F"][i], mask=r["inlier_mask"][a:b], num_inliers=r["num_inliers"][i], num_trials=r["num_trials"][i],
                best_trial=r["best_trial"][i], accepted=r["accepted"][i])


def _run(idx, opt=None, **kw):
    capi = _capi()
    ptr, xa, xb = Y.arrays(idx)
    r = capi.verify_pairs(ptr, xa, xb, capi.verify_pairs_options(**(Y.entries()[idx[0]]["opt"] if opt is None else opt)), **kw)
    return [_pair(r, ptr, i) for i in range(len(idx))]


@pytest.fixture(scope="module")
def library_results():
    """the catalogue through the library: one call per option set; catalogue index -> outputs of that pair"""
    out = {}
    for opt, idx in Y.option_groups().items():
        for k, r in zip(idx, _run(idx)):
            out[k] = r
    return out


def test_library_against_the_yardstick_on_the_whole_catalogue(library_results):
    assert Y.fragile_share() <= Y.FRAGILE_CAP
    assert len(library_results) == len(Y.entries())
    assert check_against_yardstick(library_results, "k_verify_pairs") >= 45
    by = {e["tag"]: k for k, e in enumerate(Y.entries())}
    assert library_results[by["too_few"]]["status"] == 2 and library_results[by["too_many"]]["status"] == 3
    assert library_results[by["all_origin"]]["status"] == 0
    for k, r in library_results.items():
        assert np.isfinite(r["F"]).all() and int(r["num_inliers"]) == int(r["mask"].sum())


def _same_bits(a, b):
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in a)


def test_outputs_are_bit_identical_alone_in_batches_reversed_and_again(library_results):
    c = Y.cases()
    E = Y.entries()
    idx = [k for k in c["all"] if len(E[k]["xa"]) <= 1000]
    batch, again, rev, b257 = _run(idx), _run(idx), _run(idx[::-1]), _run(c["b257"])
    first = {}
    for i, k in enumerate(c["b257"]):
        first.setdefault(k, b257[i])
        assert _same_bits(b257[i], first[k]) and _same_bits(b257[i], library_results[k]), E[k]["tag"]
    for i, k in enumerate(idx):
        alone = _run([k])[0] if i % 5 == 0 else None
        for other in (again[i], rev[len(idx) - 1 - i], library_results[k], alone):
            assert other is None or _same_bits(batch[i], other), E[k]["tag"]
    assert _same_bits(_run(c["one"])[0], library_results[c["one"][0]])


def test_per_pair_max_error_and_seed_are_honoured():
    E = Y.entries()
    idx = [k for k, e in enumerate(E) if e["tag"] in ("n63_s0.3", "n64_s0.3", "n65_s0.3", "n255_s0.3", "n256_s0.3", "n257_s0.3", "n100_s0.5", "noisy")]
    assert len(idx) == 8
    base = _run(idx)
    same = _run(idx, pair_max_error=np.full(8, 4.0), pair_seed=np.zeros(8, np.uint32))
    assert all(_same_bits(a, b) for a, b in zip(base, same))
    me = np.array([4.0, 2.0, 8.0, 3.0, 4.0, 6.0, 1.5, 4.0])
    sd = np.array([0, 0, 0, 3, 7, 11, 5489, 0xFFFFFFFF], np.uint32)
    mixed = _run(idx, pair_max_error=me, pair_seed=sd)
    differ = 0
    for i, k in enumerate(idx):
        single = _run([k], opt=dict(max_error=float(me[i]), seed=int(sd[i])))[0]
        assert _same_bits(mixed[i], single), E[k]["tag"]
        differ += not _same_bits(mixed[i], base[i])
    assert _same_bits(mixed[0], base[0]) and differ >= 4
    k = idx[3]
    want = Y.run_pair(E[k]["xa"], E[k]["xb"], Y.Options(max_error=3.0, seed=3))
    assert (mixed[3]["num_trials"], mixed[3]["best_trial"], mixed[3]["num_inliers"]) == (want["num_trials"], want["best_trial"], want["num_inliers"])


def test_untouched_outputs_and_null_optional_outputs():
    capi, E = _capi(), Y.entries()
    idx = [k for k, e in enumerate(E) if e["tag"] in ("too_few", "too_many", "all_origin", "n64_s0")]
    tags = [E[k]["tag"] for k in idx]
    ptr, xa, xb = Y.arrays(idx)
    npair, n = len(idx), len(xa)
    o = capi.verify_pairs_options(max_num_trials=130)
    status = np.full(npair, 9, np.uint8); F = np.full((npair, 9), 1234.5); mask = np.full(n, 9, np.uint8)
    ninl = np.full(npair, -77, np.int32); ntr = np.full(npair, -77, np.int32); best = np.full(npair, -77, np.int32); acc = np.full(npair, 9, np.uint8)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    up = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    call = lambda *opt: capi.load().xrsfm_ba_verify_pairs(C.byref(o), npair, ip(ptr), dp(xa), dp(xb), None, None, up(status), dp(F), up(mask), *opt)
    assert call(ip(ninl), ip(ntr), ip(best), up(acc)) == 0
    assert [int(s) for s in status] == [{"too_few": 2, "too_many": 3, "all_origin": 0}.get(tag, 1) for tag in tags]
    for i, tag in enumerate(tags):
        if tag == "n64_s0":
            assert abs(np.linalg.norm(F[i]) - 1) < 1e-15 and ninl[i] == mask[ptr[i]:ptr[i + 1]].sum() >= 60 and acc[i] == 1 and 0 <= (best[i] & ~Y.LOCAL_BIT) < ntr[i]
        else:
            assert np.all(F[i] == 1234.5) and not mask[ptr[i]:ptr[i + 1]].any() and (ninl[i], ntr[i], best[i], acc[i]) == (0, 0, -1, 0)
    F2 = np.full((npair, 9), 1234.5); mask2 = np.full(n, 9, np.uint8); status2 = np.full(npair, 9, np.uint8)
    F, mask, status, full = F2, mask2, status2, (F.copy(), mask.copy(), status.copy())
    assert call(None, None, None, None) == 0
    assert np.array_equal(F, full[0]) and np.array_equal(mask, full[1]) and np.array_equal(status, full[2])


def test_verify_then_two_view_init_recovers_the_generating_pose():
    """600 matches in pixels, 30 % outliers, noise-free inliers: verify_pairs, verified_matches, normalisation by the known
    intrinsics, two_view_init.  The pair is accepted by both calls and the relative pose that generated the matches is recovered to
    the tolerance of the two-view end-to-end test (1e-5); the baseline has no scale, so t is compared at unit length."""
    from tests import init_yardstick as YI
    capi = _capi()
    xa, xb, R, t = Y.make_pair(600, 0.3, 0.0, seed=4242, baseline=2.2)
    ptr = np.array([0, 600], np.int32)
    v = capi.verify_pairs(ptr, xa, xb)
    assert v["status"][0] == 1 and v["accepted"][0] == 1 and 415 <= v["num_inliers"][0] <= 440
    kept, rows, new_ptr = capi.verified_matches(v, ptr, np.concatenate([xa, xb], 1))
    assert kept.tolist() == [0] and new_ptr.tolist() == [0, int(v["num_inliers"][0])]
    na = (rows[:, 0:2] - Y.K[:2, 2]) / Y.FOCAL
    nb = (rows[:, 2:4] - Y.K[:2, 2]) / Y.FOCAL
    r = capi.two_view_init(new_ptr, na, nb, [10.0 / Y.FOCAL])
    assert r.status[0] == 1 and r.accepted[0] != 0
    Rg = np.asarray(YI.quat_to_mat(np.asarray(r.q[0], np.longdouble)), np.float64)
    tg, tt = r.t[0] / np.linalg.norm(r.t[0]), t / np.linalg.norm(t)
    print("relative pose: max |R - R_true| %.2e, |t - t_true| %.2e" % (np.abs(Rg - R).max(), np.abs(tg - tt).max()))
    assert np.abs(Rg - R).max() < 1e-5 and np.abs(tg - tt).max() < 1e-5
