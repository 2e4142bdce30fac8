"""No GPU: the yardstick of tests/schur_yardstick.py against two float64 restatements of the reduced-system assembly, and what the
catalogue of tests/test_gpu_schur.py contains.

The linearisation is the oracle's (r, Jc, Jp of lin_yardstick.float64_restatement, Jacobi-scaled), taken as exact like the kernel's own
on the GPU.  On every case, scaling and radius:
  * the oracle's formulas through np.linalg.inv (helpers.reduced_system_oracle restated per block) sit inside the inverse-form bar,
  * a float64 transcription of the default path (point_factor() with a plain 1 / sqrt, V = W C, blocks from V_a V_b^T, b from
    V (C^T g_p)) sits inside the factor-form bar,
  * no entry is fragile, constant rows and columns are exact, and at least 99 % of the entries of the structural blocks and every
    component of b are informative under the factor-form bar;
  * on the cases with a check held to the inverse-form bar (Y.has_inverse_check) the same runs at Y.INV_RADII = 1 and 100 as well, and
    there the informative share is asserted under the inverse-form bar too.  At a case's own radii above 100 that share is printed,
    not asserted: the pairs the yardstick's docstring lists as exempt.
Largest ratios to the bar per case family: the docstring of tests/test_gpu_schur.py, next to the kernels'."""
import numpy as np
import pytest

from tests import backsub_yardstick as BY
from tests import helpers as H
from tests import schur_yardstick as Y


@pytest.mark.parametrize("name", list(Y.CASES))
def test_restatements_inside_every_bar(name):
    c = Y.CASES[name]
    arr = Y.case(name)
    for scaling in c["scalings"]:
        lin = Y.oracle_lin(arr, scaling)
        prep = Y.prepare(arr, lin)
        assert prep["cw"] == (9 if c["wide"] else 6)
        radii = Y.inverse_radii(name) if Y.has_inverse_check(name) and scaling else c["radii"]
        for radius in radii:
            s = Y.system(prep, radius)
            assert s["fragile"] == 0, (name, scaling, radius, "a diagonal entry within its bar of a clip threshold")
            for form, fn in (("inverse", Y.restatement_inverse), ("factor", Y.restatement_factor)):
                diag, blk, b = fn(arr, lin, radius, prep)
                w = Y.assert_inside(Y.check_system(s, diag, blk, b, form), (name, scaling, radius, form))
                bad, n_const = Y.check_constants(arr, s, diag, blk, b)
                assert bad == 0, (name, scaling, radius, form, "constant rows / columns", bad, n_const)
                share = Y.informative(s, form)
                print(f"SCHUR {Y.family_of(name)} {name} scaling={int(scaling)} radius={radius:g} {form} "
                      + " ".join(f"{k}={v[0]:.4g}" for k, v in w.items()) + f" informative={share[0]:.4f}/{share[1]:.4f}")
                if form == "factor" or (Y.has_inverse_check(name) and radius in Y.INV_RADII):
                    assert share[0] >= 0.99 and share[1] == 1.0, (name, scaling, radius, form, share)


def test_product_restatement_inside_its_bar():
    """y = S x of the float64 inverse-form blocks against the product bar, for a random x and an x that is zero except on one camera."""
    for name in ("shape12", "consts_models", "low_parallax"):
        arr = Y.case(name)
        lin = Y.oracle_lin(arr, True)
        prep = Y.prepare(arr, lin)
        for radius in Y.inverse_radii(name):
            s = Y.system(prep, radius)
            diag, blk, b = Y.restatement_inverse(arr, lin, radius, prep)
            for x in Y.product_inputs(prep["Nc"], prep["cw"]):
                y = np.einsum("nij,nj->ni", diag, x)
                for (a, bb), B in blk.items():
                    y[a] += B @ x[bb]; y[bb] += B.T @ x[a]
                ref, bar = Y.product(prep, s, x)
                rat = Y._ratio(np.abs(y.astype(Y.LD) - ref), bar)
                print(f"SCHUR {name} radius={radius:g} product={rat.max():.4g}")
                assert rat.max() <= 1.0, (name, radius, float(rat.max()))


def test_catalogue_coverage(lib, monkeypatch):
    """From the packing, the Gram classification, the same-tuple table and the Cholesky plan the library reports without a GPU."""
    from xrsfm_amd import capi
    gram_C, passes, klasses, item_tiles, runs, cam_const = set(), set(), set(), set(), set(), set()
    pair_tracks, packed = [], {}
    inactive = mixed_const = wide = False
    for name, c in Y.CASES.items():
        arr = Y.case(name)
        prod = H.to_product(arr)
        for k in Y.ENV_KEYS:
            monkeypatch.delenv(k, raising=False)
        for k, v in c["env"].items():
            monkeypatch.setenv(k, v)
        plan = capi.debug_chol_plan(prod)["facts"]
        packed[name] = plan["packed"]
        assert plan["cw"] == (9 if c["wide"] else 6)
        wide |= plan["cw"] == 9
        pa, pb = Y._track_pairs(np.asarray(arr["obs_cam"], np.int64), np.asarray(arr["obs_pt"], np.int64))
        if pa.size:
            pair_tracks.append(np.unique(np.stack([arr["obs_cam"][pa], arr["obs_cam"][pb]], axis=1), axis=0, return_counts=True)[1])
        cov = BY.coverage(arr)
        item_tiles |= cov["n_tiles"]; cam_const |= cov["cam_const"]; inactive |= cov["inactive_cam"]; mixed_const |= cov["const_in_mixed_tile"]
        if c["wide"]:
            g = capi.debug_pack_gram(prod)
            klasses |= {"gram9"} if g["gram_tiles"] else set()
            klasses |= {"pair9"} if g["items_other"] else set()
            continue
        tiles, g = H.tiles_of(arr)
        for C, T, ragged, n_pass, klass in tiles:
            klasses.add(klass)
            if klass == "gram":
                gram_C.add(C); passes.add(min(n_pass, 3))
        if name in ("pair_v0", "pair_v1"):
            assert g["items_other"] > 0, (name, g)
        if c["env"].get("XRSFM_BA_SGROUP") == "4":
            runs |= set(int(v) >> 4 for v in capi.debug_sgroup(prod, 4)["pos_code"])
    counts = np.concatenate(pair_tracks)
    assert gram_C >= set(range(2, 11)), gram_C
    assert passes == {1, 2, 3}, passes
    assert klasses >= {"gram", "pair", "gram9", "pair9"}, klasses
    assert item_tiles >= {1, 2, 3, 4}, item_tiles
    assert runs >= {2, 3, 4}, runs
    assert (counts == 1).any() and (counts > 64).any()
    assert inactive and mixed_const and cam_const == {0, 1, 2, 3} and wide
    assert packed["packed"] and not packed["same_tuple"], packed
