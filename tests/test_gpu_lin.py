"""k_linearize (linearize_item), its tails (k_lin_tail; k_cam_segsum<12> + k_reduce_multi + k_gradmax_cams), the consumers'
recomputation of r and J (k_materialize_rj, k_debug_materialize), k9_linearize / k9_gradmax_cams and refine_eval against the
extended-precision yardstick of tests/lin_yardstick.py: per observation r, Jc, Jp; per track Hpp, g_p; per camera diag Hcc, g_c; the
cost and the scalars the LM controller decides on (xrsfm_ba_debug_lin_scalars), every one against its own bar counted in float64
operations (see the yardstick's docstring), on the cases whose coverage tests/test_lin_cpu.py asserts from the packing.

Variants (one context each, the environment set before the context exists): default = J-free linearisation and the fused tail;
XRSFM_BA_JFREE=0 = stored J (debug_stored_j() proves it); XRSFM_BA_FUSED=0 = the launch-per-phase tail (read when the context is
created; no entry point reports it, so that variant rests on the environment alone).  bal9 cases run through
debug_wide(radius=None) (k9_linearize's stored blocks, Jacobi scaling always on; it returns no Hpp / g_p).  Both use_scaling settings
on the 6-wide path.

Bit for bit: clamped observations give (12, 12) sqrt(rho') and a zero Jacobian, constant blocks zero columns, cameras and points
without observations zeros (their bars are 0); every array is identical between J-free and stored J, between the fused and the
unfused tail (both add the camera-major partials through segsum_body in list order) and across two calls on one context.

Largest measured ratio of each check to its bar, per case family: kernel on an MI355X (all variants and scaling settings of the
family) / float64 restatement of the oracle (test_lin_cpu.py).  The results are bit-reproducible (fixed-order sums).

  check         shapes          long            models          consts          edges           cams            bal9
  r             0.33 / 0.31     0.27 / 0.30     0.26 / 0.30     0.47 / 0.47     0.47 / 0.47     0.28 / 0.28     0.24 / 0.29
  Jc            0.35 / 0.39     0.35 / 0.34     0.37 / 0.44     0.24 / 0.33     0.23 / 0.38     0.31 / 0.31     0.32 / 0.38
  Jp            0.35 / 0.38     0.32 / 0.34     0.34 / 0.43     0.23 / 0.27     0.23 / 0.38     0.33 / 0.33     0.20 / 0.42
  Hpp           0.20 / 0.21     0.17 / 0.17     0.14 / 0.34     0.16 / 0.18     0.20 / 0.27     0.21 / 0.22     - / -
  gp            0.25 / 0.25     0.18 / 0.16     0.21 / 0.22     0.15 / 0.13     0.13 / 0.13     0.27 / 0.26     - / -
  Hcc_diag      0.15 / 0.14     0.10 / 0.09     0.01 / 0.03     0.07 / 0.07     0.20 / 0.22     0.22 / 0.22     0.21 / 0.25
  gc            0.13 / 0.13     0.11 / 0.11     0.02 / 0.04     0.04 / 0.04     0.06 / 0.11     0.26 / 0.28     0.22 / 0.22
  cost          9e-4 / 9e-4     3e-4 / 3e-4     3e-4 / 3e-4     8e-3 / 7e-3     5e-3 / 7e-3     0.03 / 0.02     4e-3 / 5e-3
  xnorm2_pts    2e-3 / 2e-3     1e-3 / 1e-3     1e-3 / 1e-3     3e-3 / 4e-3     0.04 / 6e-3     0.03 / 0.04     4e-3 / 2e-3
  gradmax_pts   0.03 / 0.03     6e-3 / 9e-3     6e-3 / 6e-3     0.02 / 5e-3     0.04 / 0.04     0.02 / 0.13     5e-3 / 5e-3
  gradmax_cams  1e-4 / 1e-4     3e-4 / 4e-4     1e-4 / 4e-4     7e-6 / 1e-4     3e-8 / 4e-8     6e-3 / 7e-3     1e-4 / 5e-4
  (sum_rho is twice the cost, bit for bit.)  Every exact check (clamped observations, constant blocks, cameras and points without
  observations, the residual of exactly 0, the A/B comparisons): exact on both sides.  bal9: debug_wide returns no Hpp / g_p.
  refine-pose initial cost (all sizes, models and masks): 0.15 of its bar.
  The cost, |x_points|^2 and the max-norms sit far inside their bars: a sum over all observations is charged its full length L,
  and a max-norm the largest bar of any candidate; a discrete error (a point counted twice, a dropped term, the wrong branch)
  moves them by many bars all the same.
"""
import numpy as np
import pytest

from tests import helpers as H
from tests import lin_yardstick as Y

pytestmark = pytest.mark.gpu

# variant -> (environment, debug_stored_j() as it must report)
VARIANTS = {"default": ({}, False), "stored_j": ({"XRSFM_BA_JFREE": "0"}, True), "unfused": ({"XRSFM_BA_FUSED": "0"}, False)}
ARRAYS = ("r", "Jc", "Jp", "Hpp", "gp", "Hcc_diag", "gc")


def _same(a, b, what):
    for k in ARRAYS:
        if k in a:
            assert np.array_equal(a[k], b[k]), (what, k, int(np.argmax(np.abs(a[k] - b[k]))))


def _scalars(ctx, out):
    sc = ctx.debug_lin_scalars()
    assert sc["sum_rho"] * 0.5 == out["cost"]
    return dict(out, **sc)


def _check(name, variant, use_scaling, got):
    w = Y.worst(Y.check_all(Y.case_reference(name, use_scaling), got))
    print(f"LIN {Y.family_of(name)} {name} {variant} scaling={int(use_scaling)} " + " ".join(f"{k}={v[0]:.4g}@{v[1]}" for k, v in w.items()))
    bad = {k: x for k, x in w.items() if not x[0] <= 1.0}
    assert not bad, f"{(name, variant, use_scaling)}: outside the bar (ratio, flat index): {bad}"


@pytest.mark.parametrize("name", [n for n in Y.CASES if not Y.is_wide(n)])
def test_linearisation_matches_yardstick(lib, monkeypatch, name):
    from xrsfm_amd import capi
    arr = Y.case(name)
    res = {}
    for variant, (env, stored) in VARIANTS.items():
        for k in ("XRSFM_BA_JFREE", "XRSFM_BA_FUSED"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        ctx = capi.Context(H.to_product(arr))
        try:
            for use_scaling in (False, True):
                got = _scalars(ctx, ctx.debug_linearize(Y.HUBER_A, use_scaling))
                assert ctx.debug_stored_j() == stored, "the variant under test did not run"
                again = _scalars(ctx, ctx.debug_linearize(Y.HUBER_A, use_scaling))
                _same(got, again, (name, variant, use_scaling, "second call"))
                assert all(got[k] == again[k] for k in Y.SCALARS), (name, variant, use_scaling, "second call")
                _check(name, variant, use_scaling, got)
                res[(variant, use_scaling)] = got
        finally:
            ctx.close()
    for use_scaling in (False, True):
        a, b, c = (res[(v, use_scaling)] for v in ("default", "stored_j", "unfused"))
        _same(a, b, (name, use_scaling, "J-free against stored J"))
        assert all(a[k] == b[k] for k in Y.SCALARS), (name, use_scaling, "J-free against stored J")
        _same(a, c, (name, use_scaling, "fused against unfused tail"))
    if name == "edges":
        i = Y.edges()[1]["zero"]
        assert (res[("default", False)]["r"][i] == 0.0).all()


@pytest.mark.parametrize("name", [n for n in Y.CASES if Y.is_wide(n)])
def test_bal9_linearisation_matches_yardstick(lib, name):
    from xrsfm_amd import capi
    ctx = capi.Context(H.to_product(Y.case(name)))
    try:
        got = _scalars(ctx, ctx.debug_wide(Y.HUBER_A))
        again = _scalars(ctx, ctx.debug_wide(Y.HUBER_A))
        _same(got, again, (name, "second call"))
        assert all(got[k] == again[k] for k in Y.SCALARS), (name, "second call")
        _check(name, "bal9", True, got)
    finally:
        ctx.close()


def test_lin_scalars_need_a_linearisation(lib):
    from xrsfm_amd import capi
    for name in ("band7", "bal9_cams_single"):
        ctx = capi.Context(H.to_product(Y.case(name)))
        try:
            with pytest.raises(RuntimeError, match="-5"):
                ctx.debug_lin_scalars()
        finally:
            ctx.close()


POSE_N = (1, 63, 64, 65, 255, 256, 257, 1500)


@pytest.mark.parametrize("n", POSE_N)
def test_refine_pose_initial_cost_matches_yardstick(lib, n):
    """refine_eval's block-strided sum (k_refine_pose; it shares project / huber with the engine): xrsfm_ba_refine_pose with
    max_iterations = 0 returns the cost at the initial pose, against the cost bar of the yardstick's 1/2 sum rho over the inliers."""
    from xrsfm_amd import capi
    opt = capi.refine_pose_options(max_iterations=0)
    worst = 0.0
    for model in range(5):
        arr = H.make_pose_problem(n=n, seed=40 + model, model=model)
        for mask in (None, (np.arange(n) % 3 != 1).astype(np.uint8)):
            ref = Y.reference(arr, False, a=opt.huber_a, obs_mask=mask)
            assert int(ref["fragile"].sum()) == 0
            q, t, s = capi.refine_pose(model, arr["intr_params"][0], arr["points"], arr["obs_uv"], arr["cam_q"][0], arr["cam_t"][0],
                                       inlier_mask=mask, options=opt)
            assert np.array_equal(q, arr["cam_q"][0]) and np.array_equal(t, arr["cam_t"][0])
            rat = float(Y.ratio(s.initial_cost, ref["cost"]))
            worst = max(worst, rat)
            assert rat <= 1.0, (n, model, mask is not None, rat, s.initial_cost, float(ref["cost"].v))
    print(f"LIN pose n={n} cost={worst:.4g}")
