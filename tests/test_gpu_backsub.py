"""k_backsub<true>, k_backsub<false> and k9_backsub against the extended-precision yardstick of tests/backsub_yardstick.py: one launch
through xrsfm_ba_debug_backsub on the library's own linearisation and camera step, everything put into the caller's order by
xrsfm_ba_debug_backsub_layout, every check with a bar counted in float64 operations (see the yardstick's docstring).

Variants (one context each, the environment set before the context exists; the layout entry's flags prove which kernel ran):
default = k_backsub<true> with recomputed F, E; XRSFM_BA_PREP_FUSED=0 = k_backsub<false> on the stored Hinv; XRSFM_BA_JFREE=0 =
stored J.  Not covered here: the in-run launch forms (the camrec_cand path and the candidate cameras written by the level-scheduled
backward substitution); the whole-solve tests keep covering those.

Largest measured ratio of each check to its bar, per case family: kernel on an MI355X (all variants and radii of the family) /
float64 restatement of the oracle (test_backsub_cpu.py).  The results are bit-reproducible (fixed-order sums).

  check               make            full_tile       long            shapes          bal9
  point_step          0.028 / -       0.014 / -       0.020 / -       0.025 / -       0.011 / -        k_backsub<true>, k9_backsub
  point_step_inverse  0.014 / 0.015   0.012 / 0.012   0.012 / 0.009   0.024 / 0.019   0.004 / 0.014    every variant
  cand_point          0.43  / 0.15    0.20  / 0.15    0.40  / 0.16    0.46  / 0.18    0.17  / 0.17
  part_step2          0.024 / 0.029   0.027 / 0.032   0.024 / 0.017   0.020 / 0.050   0.034 / 0.036
  part_model          0.0032/ 0.0059  0.0009/ 0.0046  0.0020/ 0.0048  0.0071/ 0.0086  0.0020/ 0.0071
  model_total         9e-5  / 5e-4    2e-4  / 1e-4    7e-5  / 1e-5    2e-4  / 4e-4    3e-5  / 3e-4
  cand_q              0.11  / 0.070   0.12  / 0.086   0.088 / 0.090   0.10  / 0.099   0.099 / 0.11
  cand_t              0.90  / 0.36    0.58  / 0.31    0.73  / 0.31    0.55  / 0.35    0.21  / 0.34
  cand_intr           -               -               -               -               0.22  / 0.44
  campart_step2       0.17  / 0.14    0.16  / 0.16    0.13  / 0.13    0.16  / 0.18    0.13  / 0.15
  campart_xnorm2      0.070 / 0.070   0.040 / 0.075   0.054 / 0.068   0.073 / 0.089   0.14  / 0.16
  every "unchanged bit for bit" check: exact on both sides.
  point_step (the condition-independent bar) of the implementations that multiply by a stored inverse, printed and not asserted:
  k_backsub<false> 7.8e5 (ragged at 1e8), 10 (full_tile), 0.87 (long); the float64 restatement 7.4e5 (ragged at 1e8), 88 (ragged
  at 1e4), 13 (full_tile), 0.56 (long), 1.0 (shapes), 4.8 (bal9).
"""
import numpy as np
import pytest

from oracle import ba_oracle as bo
from tests import backsub_yardstick as Y
from tests import helpers as H

pytestmark = pytest.mark.gpu

# variant -> (environment, step_prep, stored_j) as xrsfm_ba_debug_backsub_layout must report them
VARIANTS = {"default": ({}, True, False),
            "hinv": ({"XRSFM_BA_PREP_FUSED": "0"}, False, False),
            "stored_j": ({"XRSFM_BA_JFREE": "0"}, True, True)}


# The camera step comes back non-finite at radius 1e16 (measured on an MI355X) for `ragged` (single-observation tracks, rank-2 point
# blocks) on every variant and for `regular` on the stored-Hinv variant (cofactor inverse): the damped reduced system is not positive
# definite in float64 there, the breakdown a run answers with an invalid step.  The oracle's float64 Cholesky refuses the same
# problems at that radius (test_backsub_cpu.py).  These, and only these, run at 1e8 instead, the radius the oracle accepts for
# `ragged`; the test asserts that 1e16 still breaks down, so that the entry goes when the factorisation learns to take it.
INSTEAD_OF_1E16 = {("ragged", "default"): 1e8, ("ragged", "hinv"): 1e8, ("ragged", "stored_j"): 1e8, ("regular", "hinv"): 1e8}


def _check(name, radius, variant, arr, inp, got, items):
    assert sorted(map(tuple, got["item_tiles"].tolist())) == sorted(map(tuple, items["item_tiles"].tolist()))
    checks = Y.check_all(arr, inp, got)
    w = Y.worst(checks)
    print(f"BACKSUB {name} {radius:g} {variant} " + " ".join(f"{k}={v[0]:.4g}@{v[1]}" for k, v in w.items()))
    Y.assert_inside(checks, (name, radius, variant), explicit_inverse=not got["step_prep"])


def _run_narrow(name, variant):
    from xrsfm_amd import capi
    arr = Y.case(name)
    items = Y.items_from_pack(arr)
    _, want_prep, want_stored = VARIANTS[variant]
    ci, pi = arr["obs_cam"], arr["obs_pt"]
    ctx = capi.Context(H.to_product(arr))
    try:
        raw = ctx.debug_linearize(Y.HUBER_A, False)
        sc_c, sc_p = Y.jacobi_scales(raw["Jc"], raw["Jp"], ci, pi, arr["cam_q"].shape[0], arr["points"].shape[0])
        lin = ctx.debug_linearize(Y.HUBER_A, True)
        for radius in Y.CASES[name][1]:
            y, _ = ctx.debug_cholesky_solve(radius)
            if radius == 1e16 and (name, variant) in INSTEAD_OF_1E16:
                assert not np.isfinite(y).all(), (name, variant, "takes radius 1e16 now: drop it from INSTEAD_OF_1E16")
                radius = INSTEAD_OF_1E16[(name, variant)]
                y, _ = ctx.debug_cholesky_solve(radius)
            assert np.isfinite(y).all(), (name, variant, radius)
            got = ctx.debug_backsub_caller_order()
            assert (got["step_prep"], got["stored_j"]) == (want_prep, want_stored), "the variant under test did not run"
            assert H.rel_err(got["scale_c"], sc_c) < 1e-12 and H.rel_err(got["scale_p"], sc_p) < 1e-12
            inp = dict(r=lin["r"], Jc=lin["Jc"], Jp=lin["Jp"], sc_c=sc_c, sc_p=sc_p, y=y, radius=radius)
            _check(name, radius, variant, arr, inp, got, items)
    finally:
        ctx.close()


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", [n for n in Y.CASES if Y.CASES[n][2]])
def test_backsub_matches_yardstick(lib, monkeypatch, name, variant):
    for k, v in VARIANTS[variant][0].items():
        monkeypatch.setenv(k, v)
    _run_narrow(name, variant)


@pytest.mark.parametrize("name", [n for n in Y.CASES if n.startswith("shape")])
def test_backsub_shape_tiles_match_yardstick(lib, name):
    _run_narrow(name, "default")


@pytest.mark.parametrize("name", ["bal9_ragged_consts", "bal9_long"])
def test_bal9_backsub_matches_yardstick(lib, name):
    """k9_backsub after a debug_wide that solved a step.  debug_wide returns only the scaled linearisation, so the Jacobi scales are
    the library's own (layout entry), pinned to the oracle's at 1e-9 (its Jacobians are pinned at 1e-11)."""
    from xrsfm_amd import capi
    arr = Y.case(name)
    items = Y.items_from_pack(arr)
    pr = H.to_oracle(arr)
    _, _, Fc, Ep = bo.evaluate(pr, pr.cam_q, pr.cam_t, pr.points)
    sc_c, sc_p = Y.jacobi_scales(Fc, Ep, pr.obs_cam, pr.obs_pt, pr.cam_q.shape[0], pr.points.shape[0])
    ctx = capi.Context(H.to_product(arr))
    try:
        ctx.debug_wide(Y.HUBER_A)                      # linearised, no step solved
        with pytest.raises(RuntimeError, match="-5"):
            ctx.debug_backsub()
        for radius in Y.CASES[name][1]:
            out = ctx.debug_wide(Y.HUBER_A, radius)
            got = ctx.debug_backsub_caller_order()
            assert got["step_prep"] and got["stored_j"]
            assert H.rel_err(got["scale_c"], sc_c) < 1e-9 and H.rel_err(got["scale_p"], sc_p) < 1e-9
            inp = dict(r=out["r"], Jc=out["Jc"], Jp=out["Jp"], sc_c=got["scale_c"], sc_p=got["scale_p"], y=out["y"], radius=radius)
            _check(name, radius, "bal9", arr, inp, got, items)
        ctx.debug_wide(Y.HUBER_A)                      # a new linearisation: the solved step is not of it
        with pytest.raises(RuntimeError, match="-5"):
            ctx.debug_backsub()
    finally:
        ctx.close()


def test_layout_entry_states(lib):
    """The layout entry reports pt_orig, the items and the flags at any time; campart, the candidate intrinsics need a debug_backsub
    on the current step and the scales a linearisation (XRSFM_BA_ESTATE, -5, otherwise).  A bal9 context forgets its solved step
    with the next linearisation, like a 6-wide one."""
    from xrsfm_amd import capi
    arr = Y.case("regular")
    ctx = capi.Context(H.to_product(arr))
    try:
        lay = ctx.debug_backsub_layout()
        assert sorted(lay["pt_orig"].tolist()) == sorted(np.unique(arr["obs_pt"]).tolist())
        with pytest.raises(RuntimeError, match="-5"):
            ctx.debug_backsub_layout(after_backsub=True)
        with pytest.raises(RuntimeError, match="-5"):
            ctx.debug_backsub_layout(scales=True)
        ctx.debug_linearize(Y.HUBER_A, True)
        assert (ctx.debug_backsub_layout(scales=True)["scale_p"] > 0).all()
        ctx.debug_cholesky_solve(1e4)
        with pytest.raises(RuntimeError, match="-5"):
            ctx.debug_backsub_layout(after_backsub=True)        # a step, no back-substitution yet
        ctx.debug_backsub()
        assert np.isfinite(ctx.debug_backsub_layout(after_backsub=True)["campart"]).all()
        ctx.debug_cholesky_solve(1e3)                           # a new step invalidates the partials
        with pytest.raises(RuntimeError, match="-5"):
            ctx.debug_backsub_layout(after_backsub=True)
    finally:
        ctx.close()
