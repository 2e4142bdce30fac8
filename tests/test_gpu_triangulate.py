"""xrsfm_ba_triangulate_tracks on the GPU against the extended-precision yardstick (tests/tri_yardstick.py), on every case of the
catalogue: exact discrete outputs on the non-fragile tracks, the model bar on every created point, and the kernel's invariances."""
import ctypes as C

import numpy as np
import pytest

from tests import tri_yardstick as Y

pytestmark = pytest.mark.gpu

_RESULTS = {}


def run_case(name, opt_items=()):
    """one library call per (case, options), shared by the tests"""
    from xrsfm_amd import capi
    key = (name, opt_items)
    if key not in _RESULTS:
        quat, t, ptr, ocam, oxy, idx = Y.case_arrays(name)
        _RESULTS[key] = (capi.triangulate_tracks(quat, t, ptr, ocam, oxy, capi.triangulate_options(**dict(opt_items))), ptr, idx)
    return _RESULTS[key]


def track_outputs(r, ptr, j):
    """everything the call returns for track j, as bytes"""
    return (int(r["status"][j]), r["points"][j].tobytes(), r["inlier_mask"][ptr[j]:ptr[j + 1]].tobytes(), int(r["num_inliers"][j]),
            int(r["num_trials"][j]), int(r["best_trial"][j]))


CAPPED = (("max_num_trials", 7), ("exhaustive_threshold", 0), ("confidence", 0.99))


@pytest.mark.parametrize("name,opt_items", [(n, ()) for n in sorted(Y.cases())] + [("lengths", CAPPED), ("specials_mixed", CAPPED)])
def test_matches_the_yardstick(lib, name, opt_items):
    ext, fr = Y.reference("longdouble", opt_items), Y.fragile(opt_items)
    r, ptr, idx = run_case(name, opt_items)
    assert int(fr[idx].sum()) <= 0.01 * len(idx)
    assert np.all(np.isfinite(r["points"]))
    for j, k in enumerate(idx):
        e, sl = ext[k], slice(ptr[j], ptr[j + 1])
        got = dict(status=int(r["status"][j]), num_inliers=int(r["num_inliers"][j]), num_trials=int(r["num_trials"][j]),
                   best_trial=int(r["best_trial"][j]), mask=r["inlier_mask"][sl])
        if fr[k]:
            assert got["status"] in (0, 1, 2, 3)
            continue
        assert Y.same_discrete(got, e), (name, j, k, Y.pool()[k]["tag"], {q: got[q] for q in Y.DISCRETE}, {q: e[q] for q in Y.DISCRETE})
        if e["status"] == 1:
            assert int(got["mask"].sum()) == got["num_inliers"]
            assert np.allclose(r["points"][j], np.asarray(e["point"], np.float64), rtol=1e-6, atol=1e-9)
        else:
            assert not got["mask"].any() and got["num_inliers"] == 0 and got["num_trials"] == 0 and got["best_trial"] == -1


@pytest.mark.parametrize("name", sorted(Y.cases()))
def test_model_bar(lib, name):
    """h^T M h - lambda_min(M) <= (256 + 16 m) 2^-53 trace(M) for every created point, M from the yardstick in extended precision"""
    quat, t, _ = Y.cameras()
    r, ptr, idx = run_case(name)
    worst, seen, P = 0.0, 0, Y.pool()
    for j, k in enumerate(idx):
        if r["status"][j] != 1:
            continue
        seen += 1
        M, lam, m = Y.bar_matrix(quat, t, P[k]["cams"], P[k]["xy"], int(r["best_trial"][j]))
        excess, bar = Y.bar_check(r["points"][j], M, lam, m)
        worst = max(worst, excess / bar)
        assert excess <= bar, (name, j, k, P[k]["tag"], excess, bar)
    print(name, "created", seen, "largest excess / bar %.3g" % worst)
    assert seen >= 1


def test_outputs_do_not_depend_on_the_batch(lib):
    """a track's outputs are bit-identical whatever else is in the batch, in whatever order, and across two calls"""
    from xrsfm_amd import capi
    seen = {}
    for name in sorted(Y.cases()):
        r, ptr, idx = run_case(name)
        for j, k in enumerate(idx):
            out = track_outputs(r, ptr, j)
            assert seen.setdefault(k, out) == out, (name, j, k)
    quat, t, ptr, ocam, oxy, idx = Y.case_arrays("b257")
    again = capi.triangulate_tracks(quat, t, ptr, ocam, oxy)
    first = run_case("b257")[0]
    assert all(np.array_equal(first[q].view(np.uint8), again[q].view(np.uint8)) for q in first)
    # the same tracks in reverse order
    P = Y.pool()
    rev = idx[::-1]
    rptr = np.zeros(len(rev) + 1, np.int32)
    rptr[1:] = np.cumsum([len(P[k]["cams"]) for k in rev])
    r2 = capi.triangulate_tracks(quat, t, rptr, np.concatenate([P[k]["cams"] for k in rev]), np.concatenate([P[k]["xy"].reshape(-1, 2) for k in rev]))
    for j, k in enumerate(rev):
        assert track_outputs(r2, rptr, j) == seen[k], (j, k)


def test_untouched_points_and_optional_outputs(lib):
    """points of tracks without a model keep the caller's values; the three count arrays may be NULL"""
    from xrsfm_amd import capi
    quat, t, ptr, ocam, oxy, idx = Y.case_arrays("lengths")
    nt = len(idx)
    points = np.full((nt, 3), 1234.5); status = np.full(nt, 9, np.uint8); mask = np.full(len(ocam), 9, np.uint8)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    up = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))
    o = capi.triangulate_options()
    assert lib.xrsfm_ba_triangulate_tracks(C.byref(o), len(quat), dp(quat), dp(t), nt, ip(ptr), ip(ocam), dp(oxy), dp(points), up(status), up(mask),
                                           None, None, None) == 0
    r = run_case("lengths")[0]
    assert np.array_equal(status, r["status"]) and np.array_equal(mask, r["inlier_mask"])
    assert set(status.tolist()) == {0, 1, 2, 3} or set(status.tolist()) == {1, 2, 3}
    made = status == 1
    assert np.array_equal(points[made], r["points"][made]) and np.all(points[~made] == 1234.5)
