"""xrsfm_ba_two_view_init on the GPU against the yardstick (tests/init_yardstick.py): the whole catalogue with the
bars of the CPU tests, bit-identical outputs across batches, orders and calls, per-pair seed and threshold, untouched outputs, NULL
optional outputs, and two_view_init followed by xrsfm_ba_solve recovering the generating relative pose."""
import ctypes as C

import numpy as np
import pytest

from tests import init_yardstick as Y
from tests.test_init_cpu import check_against_yardstick

pytestmark = pytest.mark.gpu


def _capi():
    from xrsfm_amd import capi
    return capi


def _run(idx, **kw):
    capi = _capi()
    E = Y.entries()
    ptr, xa, xb, th = Y.arrays(idx)
    return capi.two_view_init(ptr, xa, xb, th, capi.two_view_options(**E[idx[0]]["opt"]), **kw)


@pytest.fixture(scope="module")
def library_results():
    """the catalogue through the library: one call per option set; catalogue index -> outputs of that pair"""
    out = {}
    for opt, idx in Y.option_groups().items():
        r = _run(idx)
        for i, k in enumerate(idx):
            out[k] = r.pair(i)
    return out


def test_library_against_the_yardstick_on_the_whole_catalogue(library_results):
    assert len(library_results) == len(Y.entries())
    assert check_against_yardstick(library_results, "k_init_pairs") >= 55
    E = Y.entries()
    by = {e["tag"]: k for k, e in enumerate(E)}
    assert library_results[by["too_few"]]["status"] == 2 and library_results[by["too_many"]]["status"] == 3
    assert library_results[by["nothing_in_front"]]["status"] == 0 and library_results[by["nothing_in_front"]]["best_trial"] >= 0
    r = library_results[by["overflow"]]
    assert r["status"] == 0 and r["best_trial"] == -1 and r["num_trials"] == 3 and not r["E"].any()


def _same_bits(a, b):
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in _capi().TwoViewResult.FIELDS)


def test_outputs_are_bit_identical_alone_in_a_batch_reversed_and_again(library_results):
    E = Y.entries()
    idx = [k for k, e in enumerate(E) if not e["opt"]][:12]
    assert len(idx) >= 8
    batch, again, rev = _run(idx), _run(idx), _run(idx[::-1])
    for i, k in enumerate(idx):
        alone = _run([k]).pair(0) if i < 4 else None
        for other in (again.pair(i), rev.pair(len(idx) - 1 - i), library_results[k], alone):
            assert other is None or _same_bits(batch.pair(i), other), E[k]["tag"]


def test_per_pair_seed_and_threshold_are_honoured():
    capi, E = _capi(), Y.entries()
    k = next(k for k, e in enumerate(E) if e["tag"] == "seed7")
    e = E[k]
    ptr, xa, xb, _ = Y.arrays([k, k, k])
    r = capi.two_view_init(ptr, xa, xb, [e["th"], e["th"], 2 * e["th"]], capi.two_view_options(), pair_seed=[7, 0, 7])
    want7 = Y.reference("longdouble")[k]
    want0 = Y.solve_pair(e["xa"], e["xb"], e["th"], Y.Options(seed=0))
    wide = Y.solve_pair(e["xa"], e["xb"], 2 * e["th"], Y.Options(seed=7))
    assert not Y.fragile()[k]
    for i, want in enumerate((want7, want0, wide)):
        got = r.pair(i)
        assert (got["best_trial"], got["num_trials"], got["counts"][0]) == (want["best_trial"], want["num_trials"], want["counts"][0])
        assert np.array_equal(got["essential_mask"], want["essential_mask"])
    assert r.best_trial[0] != r.best_trial[1] and r.counts[2, 0] > r.counts[0, 0]


def test_untouched_outputs_and_null_optional_outputs():
    capi, E = _capi(), Y.entries()
    idx = [k for k, e in enumerate(E) if e["tag"] in ("too_few", "nothing_in_front", "too_many", "n64_s0_wide_v0")]
    tags = [E[k]["tag"] for k in idx]
    ptr, xa, xb, th = Y.arrays(idx)
    npair, n = len(idx), len(xa)
    o = capi.two_view_options(max_depth=1e-9)
    status = np.zeros(npair, np.uint8); Em = np.full((npair, 9), 1234.5); q = np.full((npair, 4), 1234.5); t = np.full((npair, 3), 1234.5)
    pts = np.full((n, 3), 1234.5); em = np.full(n, 9, np.uint8); fm = np.full(n, 9, np.uint8); counts = np.full((npair, 8), -77, np.int32)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    up = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))
    code = capi.load().xrsfm_ba_two_view_init(C.byref(o), npair, ptr.ctypes.data_as(C.POINTER(C.c_int32)), dp(xa), dp(xb), dp(th), None, up(status), dp(Em), dp(q),
                                              dp(t), dp(pts), up(em), up(fm), counts.ctypes.data_as(C.POINTER(C.c_int32)), None, None, None)
    assert code == 0
    assert [int(s) for s in status] == [{"too_few": 2, "too_many": 3}.get(tag, 0) for tag in tags]          # (max_depth 1e-9: nothing is in front)
    assert np.all(q == 1234.5) and np.all(t == 1234.5) and np.all(pts == 1234.5) and not fm.any()
    for i, tag in enumerate(tags):
        if tag in ("too_few", "too_many"):
            assert np.all(Em[i] == 1234.5) and not counts[i].any() and not em[ptr[i]:ptr[i + 1]].any()
        else:
            assert abs(np.linalg.norm(Em[i]) - 1) < 1e-15 and counts[i, 0] == em[ptr[i]:ptr[i + 1]].sum() > 0 and not counts[i, 1:].any()


def test_two_view_init_then_solve_recovers_the_generating_pose():
    """300 matches, 20 % outliers, noise-free inliers: two_view_init, then xrsfm_ba_solve over (identity (constant), (q, t), the
    points of front_mask and essential_mask); the relative pose that generated the matches is recovered to the tolerance of the
    absolute-pose end-to-end test (1e-5), gauge-aware: the baseline has no scale, so t is compared at unit length."""
    from xrsfm_amd import capi, parity
    xa, xb, R, t = Y.make_pair(300, 0.2, 0.0, 2.2, seed=4242)
    r = capi.two_view_init([0, 300], xa, xb, [Y.TH])
    assert r.status[0] == 1 and r.accepted[0] & 1
    keep = (r.front_mask & r.essential_mask).astype(bool)
    npt = int(keep.sum())
    assert npt >= 230
    obs_cam = np.tile(np.array([0, 1], np.int32), npt); obs_pt = np.repeat(np.arange(npt, dtype=np.int32), 2)
    uv = np.stack([xa[keep], xb[keep]], 1).reshape(-1, 2) * Y.FX
    prob = capi.ProblemArrays(cam_q=np.array([[0.0, 0.0, 0.0, 1.0], r.q[0]]), cam_t=np.array([[0.0, 0.0, 0.0], r.t[0]]), cam_const=np.array([3, 0], np.uint8),
                              cam_intr=np.zeros(2, np.int32), intr_model=np.full(1, 2, np.int32), intr_params=np.array([[Y.FX, 0, 0, 0, 0, 0, 0, 0.0]]),      # SIMPLE_RADIAL, k = 0
                              points=r.points[keep], point_const=np.zeros(npt, np.uint8), obs_cam=obs_cam, obs_pt=obs_pt, obs_uv=uv)
    capi.solve(prob)
    assert np.array_equal(prob.cam_q[0], [0, 0, 0, 1]) and not prob.cam_t[0].any()
    t_solved = prob.cam_t.copy()
    t_solved[1] /= np.linalg.norm(t_solved[1])
    q_true = np.array([[0.0, 0.0, 0.0, 1.0], np.asarray(Y.quat_of(R), np.float64)]); t_true = np.array([[0.0, 0.0, 0.0], t / np.linalg.norm(t)])
    ang, dt = parity.relative_pose_difference(prob.cam_q, t_solved, q_true, t_true, [(1, 0)])
    print("relative pose after BA: angle %.2e rad, |dt| %.2e" % (ang, dt))
    assert ang < 1e-5 and dt < 1e-5
