"""xrsfm_ba_run_batch / xrsfm_ba_solve_batch (include/xrsfm_ba.h; xrsfm_amd/csrc/ba_lba.h: k_lba_batch): many local-BA-sized problems
as the workgroups of one launch.

The yardstick of every problem is its own single launch (XRSFM_BA_SOLVER_RESIDENT on a fresh context): the state and every summary
field but the times must be equal BIT FOR BIT, whatever the batch holds and in whatever order.  Against the engine
(XRSFM_BA_SOLVER_CHOLESKY) the bounds are those of tests/test_gpu_lba_resident.py (_same_as_engine: 1e-6 px, 1e-5), imported from
there.  Problem builders: tests/helpers.py.
"""
import numpy as np
import pytest

from tests import helpers as H
from tests import test_gpu_lba_resident as R

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -5
FIELDS = ("initial_cost", "final_cost", "num_residuals", "num_effective_params", "n_successful", "n_unsuccessful", "termination",
          "termination_reason", "pcg_iterations", "lm_steps_attempted", "linear_solver_used")          # every field except the times / profile


def _fields(s):
    return tuple(getattr(s, f) for f in FIELDS)


def _opt(**kw):
    from xrsfm_amd import capi
    o = dict(R.LBA_OPT); o.update(kw)
    o.setdefault("linear_solver", capi.SOLVER_RESIDENT)
    return capi.default_options(**o)


def _alone(arr, solver=None, **kw):
    """(q, t, P, summary) of a fresh context of `arr` run alone."""
    from xrsfm_amd import capi
    ctx = capi.Context(H.to_product(arr))
    s = ctx.run(_opt(linear_solver=capi.SOLVER_RESIDENT if solver is None else solver, **kw))
    out = ctx.download() + (s,)
    ctx.close()
    return out


def _same_bits(got, want, what=""):
    assert all(np.array_equal(a, b) for a, b in zip(got[:3], want[:3])), what
    assert _fields(got[3]) == _fields(want[3]), what


def _batch(arrs, **kw):
    """Fresh contexts of `arrs` in one xrsfm_ba_run_batch: (code, [(q, t, P, summary)], codes)."""
    from xrsfm_amd import capi
    ctxs = [capi.Context(H.to_product(a)) for a in arrs]
    code, sums, codes = capi.run_batch(ctxs, _opt(**kw))
    out = [c.download() + (s,) for c, s in zip(ctxs, sums)]
    for c in ctxs:
        c.close()
    return code, out, codes


def _untouched(ctx, arr):
    q, t, P = ctx.download()
    return np.array_equal(q, arr["cam_q"]) and np.array_equal(t, arr["cam_t"]) and np.array_equal(P, arr["points"])


def _with_duplicate(arr):
    """The first track is observed twice by its first camera (tests/test_gpu_lba_resident.py::test_refusals)."""
    arr = dict(arr)
    i = int(np.flatnonzero(arr["obs_pt"] == arr["obs_pt"][0])[0])
    for k in ("obs_cam", "obs_pt"):
        arr[k] = np.concatenate([arr[k], arr[k][i:i + 1]])
    arr["obs_uv"] = np.concatenate([arr["obs_uv"], arr["obs_uv"][i:i + 1] + 0.5])
    return arr


def _unlike():
    from xrsfm_amd import capi
    two = H.make(2, 30, 2, seed=122)                                   # 60 observations: one tile
    rng = np.random.default_rng(3)
    ragged = H.make_tracks(3, [[0, 1, 2] if i % 2 == 0 else [int(rng.integers(3))] for i in range(41)], seed=7)
    seven = H.make(7, 150, 4, seed=127)                                # 600 observations: pass A takes two chunks of 8 tiles
    ten = H.make(10, 120, 4, seed=103)
    ten["cam_const"][:] = 0; ten["cam_const"][2] = 3; ten["cam_const"][5] = 1; ten["cam_const"][6] = 2
    ten["point_const"][::3] = 1
    one = H.make(1, 97, 1, seed=121)
    one["point_const"][:] = 0
    assert capi.debug_pack(H.to_product(two))["tiles"] == 1 and capi.debug_pack(H.to_product(seven))["tiles"] > 8
    return [two, ragged, seven, ten, one]


def test_bit_identity_with_the_single_launch(lib):
    from xrsfm_amd import capi
    arrs = _unlike()
    code, out, codes = _batch(arrs)
    assert code == 0 and not codes.any()
    for i, (arr, got) in enumerate(zip(arrs, out)):
        _same_bits(got, _alone(arr), f"problem {i}")
        assert got[3].linear_solver_used == capi.SOLVER_RESIDENT
        eng = _alone(arr, solver=capi.SOLVER_CHOLESKY)
        R._same_as_engine(arr, eng[3], got[3], eng, got)
    assert len({s.total_time_s for *_, s in out}) == 1 and out[0][3].total_time_s > 0.0


def test_more_problems_than_compute_units(lib):
    arrs = [H.make(3, 60, 3, seed=1000 + i) for i in range(300)]
    code, out, codes = _batch(arrs)
    assert code == 0 and not codes.any()
    for i, (arr, got) in enumerate(zip(arrs, out)):
        _same_bits(got, _alone(arr), f"problem {i}")
    code, rev, codes = _batch(arrs[::-1])
    assert code == 0 and not codes.any()
    for i, (a, b) in enumerate(zip(out, rev[::-1])):
        _same_bits(b, a, f"problem {i} reversed")


def test_unequal_lengths(lib):
    """One problem starts at its optimum of noise-free data and stops at its first test; the others take all five steps."""
    kw = dict(max_iterations=5, function_tolerance=0.0, parameter_tolerance=0.0, gradient_tolerance=1e-6)
    done = H.make(5, 80, 3, seed=31, noise=0.0, outlier_frac=0.0, perturb=(0.0, 0.0, 0.0))
    arrs = [H.make(5, 80, 3, seed=32), done, H.make(7, 150, 4, seed=33), H.make(4, 50, 2, seed=34)]
    code, out, codes = _batch(arrs, **kw)
    assert code == 0 and not codes.any()
    for i, (arr, got) in enumerate(zip(arrs, out)):
        _same_bits(got, _alone(arr, **kw), f"problem {i}")
        s = got[3]
        if i == 1:
            assert (s.termination_reason, s.lm_steps_attempted, s.n_successful) == (1, 0, 0)
        else:
            assert (s.termination_reason, s.lm_steps_attempted) == (5, 5)


def test_per_problem_refusal(lib):
    from xrsfm_amd import capi
    arrs = [H.make(7, 150, 4, seed=151), H.make(3, 60, 3, seed=152), _with_duplicate(H.make(7, 150, 4, seed=153)), H.make(10, 120, 4, seed=154)]
    ctxs = [capi.Context(H.to_product(a)) for a in arrs]
    code, sums, codes = capi.run_batch(ctxs, _opt())
    assert code == EINVAL and list(codes) == [0, 0, EINVAL, 0]
    assert _untouched(ctxs[2], arrs[2])
    assert _fields(sums[2]) == (0,) * len(FIELDS) and sums[2].total_time_s == 0.0
    for i in (0, 1, 3):
        _same_bits(ctxs[i].download() + (sums[i],), _alone(arrs[i]), f"problem {i}")
    for c in ctxs:
        c.close()


ARGUMENT_CASES = ["negative_count", "above_cap", "null_entry", "twice", "cams11", "bal9", "cholesky", "negative_max_iterations"]


@pytest.mark.parametrize("case", ARGUMENT_CASES)
def test_argument_errors(lib, case):
    from xrsfm_amd import capi
    arrs = [H.make(3, 60, 3, seed=161), H.make(7, 150, 4, seed=162)]
    if case == "cams11":
        arrs.insert(1, H.make(11, 200, 4, seed=150))
    if case == "bal9":
        arrs.append(H.make_bal9(8, 200, 4, seed=5))
    ctxs = [capi.Context(H.to_product(a)) for a in arrs]
    batch, kw, n_ctx = list(ctxs), {}, None
    if case == "negative_count":
        n_ctx = -1
    elif case == "above_cap":
        batch, n_ctx = [ctxs[0]], capi.BATCH_MAX + 1
    elif case == "null_entry":
        batch = [ctxs[0], None, ctxs[1]]
    elif case == "twice":
        batch = [ctxs[0], ctxs[1], ctxs[0]]
    elif case == "cholesky":
        kw = dict(linear_solver=capi.SOLVER_CHOLESKY)
    elif case == "negative_max_iterations":
        kw = dict(max_iterations=-1)
    code, _, _ = capi.run_batch(batch, _opt(**kw), n_ctx=n_ctx)
    assert code == EINVAL
    assert all(_untouched(c, a) for c, a in zip(ctxs, arrs))
    for c in ctxs:
        c.close()


def test_an_empty_batch_is_success(lib):
    from xrsfm_amd import capi
    code, sums, codes = capi.run_batch([], _opt())
    assert code == 0 and sums == [] and len(codes) == 0


def test_the_contexts_afterwards(lib):
    from xrsfm_amd import capi
    from tests import cov_yardstick as Y
    arrs = [Y.fix_gauge(H.make(8, 100, 4, seed=171)), H.make(9, 120, 4, seed=172), H.make(3, 60, 3, seed=173)]
    ctxs = [capi.Context(H.to_product(a)) for a in arrs]
    code, _, _ = capi.run_batch(ctxs, _opt())
    assert code == 0
    cov = ctxs[0].covariance([1, 4])
    single = capi.Context(H.to_product(arrs[0]))
    single.run(_opt())
    assert np.array_equal(cov, single.covariance([1, 4]))
    single.close()
    ctxs[1].reset()
    assert _untouched(ctxs[1], arrs[1])
    s = ctxs[1].run(_opt(linear_solver=capi.SOLVER_CHOLESKY))
    _same_bits(ctxs[1].download() + (s,), _alone(arrs[1], solver=capi.SOLVER_CHOLESKY))
    for c in ctxs:
        c.close()


def test_one_shot(lib):
    from xrsfm_amd import capi
    arrs = [H.make(7, 150, 4, seed=181), H.make(3, 60, 3, seed=182), H.make(10, 120, 4, seed=183)]
    code, want, _ = _batch(arrs)
    assert code == 0
    prods = [H.to_product(a) for a in arrs]
    code, sums, codes = capi.solve_batch(prods, _opt())
    assert code == 0 and not codes.any()
    for i, (p, s) in enumerate(zip(prods, sums)):
        _same_bits((p.cam_q, p.cam_t, p.points, s), want[i], f"problem {i}")
    # a refused problem among them keeps its arrays
    arrs[1] = _with_duplicate(arrs[1])
    prods = [H.to_product(a) for a in arrs]
    code, sums, codes = capi.solve_batch(prods, _opt())
    assert code == EINVAL and list(codes) == [0, EINVAL, 0]
    assert all(np.array_equal(getattr(prods[1], k), arrs[1][k]) for k in ("cam_q", "cam_t", "points"))
    for i in (0, 2):
        _same_bits((prods[i].cam_q, prods[i].cam_t, prods[i].points, sums[i]), want[i], f"problem {i}")


def test_profile(lib):
    from xrsfm_amd import capi
    arrs = [H.make(3, 60, 3, seed=191), H.make(7, 150, 4, seed=192), H.make(5, 80, 3, seed=193)]
    ctxs = [capi.Context(H.to_product(a)) for a in arrs]
    code, sums, _ = capi.run_batch(ctxs, _opt(profile=1))
    assert code == 0
    launched = [{k: v for k, v in c.profile().items() if v[1] > 0} for c in ctxs]
    for c in ctxs:
        c.close()
    assert list(launched[0]) == ["k_lba_resident"] and launched[0]["k_lba_resident"][1] == 1
    assert launched[1] == {} and launched[2] == {}
    assert all(s.dom_kernel_launches == 1 and s.dom_kernel_ms == launched[0]["k_lba_resident"][0] > 0.0 for s in sums)
