"""The assembly of the damped reduced camera system S y = b (k_schur_pairs<GRAM, PREP, NIK>, sgroup_finish, k_chol_segsum /
k_chol_segsum_v, k_tile_fill, point_factor(); the bal9 twins k9_pairs / k9_pairs_gram / k9_chol_segsum / k9_tile_fill; on the PCG path
k_point_prep, k_schur_prep, k_cam_factor, k_schur_matvec) against the extended-precision yardstick of tests/schur_yardstick.py:
every entry of every diagonal block and of every structural off-diagonal block, and every component of b, as
Context.debug_reduced_system(radius, want_y=False) reads them from the tile storage before factoring, against its own bar counted in
float64 operations (the yardstick's docstring).  The yardstick is built from the context's own r, Jc, Jp (debug_linearize /
debug_wide), so the linearisation's error (tests/test_gpu_lin.py) is not mixed in.  The cases and what they cover: test_schur_cpu.py.

Variants (one context each, the environment set before the context exists): default; XRSFM_BA_PREP_FUSED=0 (k_point_prep's stored
cofactor inverse and its factor: held to the inverse-form bar; the step_prep flag of debug_backsub_layout() proves which of the two
ran); XRSFM_BA_JFREE=0 (debug_stored_j() proves it); XRSFM_BA_GRAM4=0; XRSFM_BA_GRAM_MERGE=0; XRSFM_BA_SGROUP=0 / 4;
XRSFM_BA_PAIR_V=0 / 1; XRSFM_BA_PACKED=1 (the plan fact "packed" proves it).  GRAM4, GRAM_MERGE, SGROUP and PAIR_V rest on the
environment alone: no entry point reports what the context made of them, and their own A/B tests (test_gpu_parity.py,
test_gpu_s_prereduce.py) stand on the same footing.  All variants run on shape0 (Gram tiles only), ragged, shape12 (per-pair tiles)
and long; the default alone on the rest (a case that needs a switch to reach its branch sets it).  The checks held to the
inverse-form bar (XRSFM_BA_PREP_FUSED=0, the PCG path) run at the radii 1 and 100, where that bar is informative on every entry, and
then at the case's own radii, where it is not everywhere: which (case, radius) pairs are exempt from the informative-share
condition, and why, is in the yardstick's docstring; test_schur_cpu.py asserts the rest.

Bit for bit: rows and columns of constant camera parameters and of cameras without an observation (zero but for 1e-6 / radius on
the diagonal, b = 0); two calls of debug_reduced_system on one context return identical arrays; the dense S of
debug_cholesky_solve(want_S=True) is exactly 0 in every block no track links and equal to the tile storage elsewhere.  That last
check runs on the default variant of the 6-wide cases of at most 100 cameras only: the entry point returns 6-wide blocks, so bal9 is
not covered by it, and the other variants are not either.

PCG path (6-wide): debug_schur_product(radius, x) against the yardstick's S x and b per camera and component, the inverse-form bar
carried through the product, for a random x and an x that is zero except on one camera.

Largest measured ratio of each check to its bar per case family: kernel on an MI355X (every variant, scaling and radius of the
family; the inverse-form rows are XRSFM_BA_PREP_FUSED=0 and the PCG path) / float64 restatement on the oracle's linearisation
(test_schur_cpu.py: the transcription of point_factor() for the factor form, np.linalg.inv for the inverse form).

  check            shapes          long            make            low_parallax    pair            bal9
  diag, factor     0.099 / 0.15    0.11 / 0.15     0.11 / 0.15     0.17 / 0.17     0.11 / 0.11     0.22 / 0.22
  blk, factor      0.15 / 0.12     0.098 / 0.11    0.16 / 0.11     0.024 / 0.042   0.073 / 0.056   0.061 / 0.066
  b, factor        0.075 / 0.11    0.069 / 0.065   0.043 / 0.071   0.019 / 0.033   0.033 / 0.057   0.032 / 0.055
  diag, inverse    0.15 / 0.15     0.15 / 0.15     0.15 / 0.15     - / 0.17        - / 0.11        - / 0.22
  blk, inverse     0.052 / 0.055   0.053 / 0.083   0.015 / 0.052   - / 0.017       - / 0.019       - / 0.035
  b, inverse       0.070 / 0.086   0.051 / 0.052   0.009 / 0.057   - / 0.021       - / 0.021       - / 0.047
  pcg y = S x      0.033 / 0.039   0.0066 / -      0.067 / 0.067   0.050 / 0.050   - / -           - / -
  pcg b            0.095 / -       0.051 / -       0.0077 / -      0.0059 / -      - / -           - / -
  (diag: the largest ratios, 0.1 to 0.22, are the damping 1e-6 / radius of constant blocks, one rounding against a bar of 4 eps.
  make: the all-variant case of the family is ragged; the restatement's product ratios are those of shape12, consts_models and
  low_parallax.  Every exact check held on every variant: constant rows and columns, blocks no track links, the second call, the
  dense S against the tile storage.)
  informative entries, smallest share over a family (blocks / b), from the kernel's own linearisation: factor form 1.000 / 1.000 in
  every family at every radius; inverse form 1.000 / 1.000 at the radii 1 and 100 (shapes, long, make); at the case's own radii
  above 100, the exempt pairs, 0.9999 / 0.976 (shapes), 0.999 / 0.864 (long), 0.976 / 0.786 (ragged); low_parallax on the PCG path,
  from test_schur_cpu.py: 1.000 / 1.000 at 1 and 100, 0.234 / 0.125 at 1e4 and 1e12.
  All 109 tests: 29 s; the slowest, bal9_long, 3.6 s.

Mutations (scratch copies of the sources, never committed): (1) one Newton step instead of two in fast_rsqrt, (2) the damping clip of
a point block's second diagonal entry taken from the first, (3) V = W C without its third column for tracks of length 2.
Each mutant once on an MI355X against the default variant of every case here (49 tests, before the inverse-form radii were added) and
against the older normwise checks (test_shape_tiles_match_oracle[0], test_cholesky_reduced_system, test_schur_product: 16 tests,
H.rel_err < 1e-11 / 1e-10):
  (1)  new: 3 of 49 fail, off-diagonal blocks at 1.04 (shape11), 1.13 (shape16) and 1.10 (full_tile, radius 1e4) of their bar;
       old: all 16 pass.  A one-step fast_rsqrt is still good to about 1e-14, a thousandth of what the normwise bar allows; the
       new bars catch it, but only just: they are the worst case of every rounding, and a correct kernel uses a tenth of them.
  (2)  new: 48 of 49 fail, by 8e9 (diag), 1e10 (blk), 5e9 (b) on shape0 (pose, the 49th, has no variable point);
       old: 13 of 16 fail (rel_err 1e-7 to 4e-4): the old checks catch this one too.
  (3)  new: shape0, two_cams and low_parallax fail, by 5e12 (diag), 9e12 (blk), 2e12 (b): the cases with regular tiles of two-view
       tracks; old: test_shape_tiles_match_oracle[0] fails (rel_err 0.36), the other 15 pass (no regular tile of two-view tracks).
"""
import numpy as np
import pytest

from tests import helpers as H
from tests import schur_yardstick as Y

pytestmark = pytest.mark.gpu

# variant -> (environment, the bar it is held to)
VARIANTS = {"default": ({}, "factor"), "prep_unfused": ({"XRSFM_BA_PREP_FUSED": "0"}, "inverse"), "stored_j": ({"XRSFM_BA_JFREE": "0"}, "factor"),
            "gram16": ({"XRSFM_BA_GRAM4": "0"}, "factor"), "unmerged": ({"XRSFM_BA_GRAM_MERGE": "0"}, "factor"),
            "sgroup0": ({"XRSFM_BA_SGROUP": "0"}, "factor"), "sgroup4": ({"XRSFM_BA_SGROUP": "4"}, "factor"),
            "pair_v0": ({"XRSFM_BA_PAIR_V": "0"}, "factor"), "pair_v1": ({"XRSFM_BA_PAIR_V": "1"}, "factor"),
            "packed": ({"XRSFM_BA_PACKED": "1"}, "factor")}
RUNS = [(n, v) for n in Y.CASES for v in (VARIANTS if n in Y.ALL_VARIANTS else ("default",))]
_PREP = {}


def _prep(name, scaling, lin):
    """The radius-independent part of the yardstick, shared by the variants of a case while their linearisations are identical."""
    key = (name, scaling)
    hit = _PREP.get(key)
    if hit is None or not all(np.array_equal(hit[0][k], lin[k]) for k in ("r", "Jc", "Jp")):
        hit = _PREP[key] = ({k: lin[k] for k in ("r", "Jc", "Jp")}, Y.prepare(Y.case(name), lin), {})
    return hit[1], hit[2]


def _system(name, scaling, lin, radius):
    prep, cache = _prep(name, scaling, lin)
    if radius not in cache:
        cache[radius] = Y.system(prep, radius)
    return prep, cache[radius]


def _context(monkeypatch, name, variant):
    from xrsfm_amd import capi
    for k in Y.ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    env = dict(Y.CASES[name]["env"], **VARIANTS[variant][0])
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return capi.Context(H.to_product(Y.case(name))), env


@pytest.mark.parametrize("name,variant", RUNS)
def test_reduced_system_matches_yardstick(lib, monkeypatch, name, variant):
    c = Y.CASES[name]
    arr = Y.case(name)
    form = VARIANTS[variant][1]
    ctx, env = _context(monkeypatch, name, variant)
    try:
        for scaling in c["scalings"]:
            lin = ctx.debug_wide(Y.HUBER_A) if c["wide"] else ctx.debug_linearize(Y.HUBER_A, scaling)
            assert c["wide"] or ctx.debug_stored_j() == (env.get("XRSFM_BA_JFREE") == "0"), "the variant under test did not run"
            for i, radius in enumerate(Y.inverse_radii(name) if form == "inverse" else c["radii"]):
                red = ctx.debug_reduced_system(radius, want_y=False)
                if not c["wide"]:
                    assert ctx.debug_backsub_layout()["step_prep"] == (env.get("XRSFM_BA_PREP_FUSED") != "0"), "the variant under test did not run"
                assert red["facts"]["packed"] == (env.get("XRSFM_BA_PACKED") == "1"), "the storage under test did not run"
                prep, s = _system(name, scaling, lin, radius)
                diag, blk, b = Y.blocks_of(red)
                w = Y.worst(Y.check_system(s, diag, blk, b, form))
                share = Y.informative(s, form)
                print(f"SCHUR {Y.family_of(name)} {name} {variant} scaling={int(scaling)} radius={radius:g} {form} "
                      + " ".join(f"{k}={v[0]:.4g}@{v[1]}" for k, v in w.items()) + f" informative={share[0]:.4f}/{share[1]:.4f}")
                bad = {k: x for k, x in w.items() if not x[0] <= 1.0}
                assert not bad, f"{(name, variant, scaling, radius)}: outside the bar (ratio, flat index): {bad}"
                n_bad, n_const = Y.check_constants(arr, s, diag, blk, b)
                assert n_bad == 0, (name, variant, scaling, radius, "constant rows / columns", n_bad, n_const)
                if i == 0:
                    again = ctx.debug_reduced_system(radius, want_y=False)
                    assert np.array_equal(again["b"], red["b"]) and np.array_equal(again["blk_rc"], red["blk_rc"])
                    assert (again["S"] != red["S"]).nnz == 0, (name, variant, "second call")
                    if variant == "default" and not c["wide"] and prep["Nc"] <= 100:
                        _, S = ctx.debug_cholesky_solve(radius, want_S=True)
                        linked = np.eye(prep["Nc"], dtype=bool)
                        linked[s["keys"][:, 0], s["keys"][:, 1]] = True; linked[s["keys"][:, 1], s["keys"][:, 0]] = True
                        blocks = np.abs(S).reshape(prep["Nc"], 6, prep["Nc"], 6).max(axis=(1, 3))
                        assert (blocks[~linked] == 0).all(), (name, "a block no track links is not zero")
                        assert np.array_equal(np.tril(S), np.tril(red["S"].toarray())), (name, "dense S against the tile storage")
    finally:
        ctx.close()


@pytest.mark.parametrize("name", [n for n, c in Y.CASES.items() if c["pcg"]])
def test_schur_product_matches_yardstick(lib, monkeypatch, name):
    c = Y.CASES[name]
    ctx, _ = _context(monkeypatch, name, "default")
    try:
        lin = ctx.debug_linearize(Y.HUBER_A, True)
        for radius in Y.inverse_radii(name):
            prep, s = _system(name, True, lin, radius)
            for which, x in zip(("random", "one_camera"), Y.product_inputs(prep["Nc"], prep["cw"])):
                y, b = ctx.debug_schur_product(radius, x)
                ref, bar = Y.product(prep, s, x)
                ry = Y._ratio(np.abs(y.astype(Y.LD) - ref), bar)
                rb = Y._ratio(np.abs(b.astype(Y.LD) - s["b"]), s["b_bar"]["inverse"])
                print(f"SCHUR {Y.family_of(name)} {name} pcg radius={radius:g} x={which} y={ry.max():.4g}@{int(ry.argmax())} b={rb.max():.4g}@{int(rb.argmax())}")
                assert ry.max() <= 1.0 and rb.max() <= 1.0, (name, radius, which, float(ry.max()), float(rb.max()))
    finally:
        ctx.close()
