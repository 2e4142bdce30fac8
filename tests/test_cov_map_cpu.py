"""Whole-map covariance without a GPU: the symbol, its declaration and the Python method, the numpy restatement of the tile
recurrence against a dense inverse, the facts of the `deep3` fixture and the agreement of the two dense CPU routes on it."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from tests import cov_map_yardstick as M
from tests import cov_point_yardstick as P
from tests import cov_yardstick as Y

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_and_declaration(lib):
    from xrsfm_amd import capi
    assert getattr(lib, "xrsfm_ba_map_covariance") is not None
    assert "xrsfm_ba_map_covariance" in capi.EXPORTS
    assert hasattr(capi.Context, "map_covariance")
    hdr = open(os.path.join(ROOT, "include", "xrsfm_ba.h")).read()
    assert re.search(r"int\s+xrsfm_ba_map_covariance\s*\(\s*xrsfm_ba_context\s*\*ctx,\s*double huber_a,\s*double \*cam_cov,\s*double \*pt_cov,"
                     r"\s*uint8_t \*cam_status,\s*uint8_t \*pt_status\)", hdr)
    # the selected calls no longer list the whole map as missing: they name the call
    assert "covariance of ALL points" not in hdr
    for first, decl in (("Marginal covariance of selected cameras", "int xrsfm_ba_covariance("), ("Marginal covariance of selected 3-D points", "int xrsfm_ba_point_covariance("),
                        ("Joint covariance of selected cameras AND points", "int xrsfm_ba_joint_covariance(")):
        assert "xrsfm_ba_map_covariance" in hdr[hdr.index(first):hdr.index(decl)]


def test_null_context_needs_no_device(lib):
    lib.xrsfm_ba_map_covariance.argtypes = [C.c_void_p, C.c_double] + [C.c_void_p] * 4
    lib.xrsfm_ba_map_covariance.restype = C.c_int
    assert lib.xrsfm_ba_map_covariance(None, 5.99, None, None, None, None) == -1


def test_library_exports_the_symbol(lib):
    from xrsfm_amd import _build
    out = subprocess.run(["nm", "-D", "--defined-only", _build.LIB], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT xrsfm_ba_map_covariance\b", out)


def test_numpy_recurrence_matches_dense_inverse():
    """A random block-sparse SPD matrix on a fill-closed pattern of 4 levels with columns of two and three off-diagonal tiles (the
    transposed reads Z_mi^T run): every tile of the recurrence equals the tile of the dense inverse."""
    rng = np.random.default_rng(5)
    T, NB = 8, M.NB
    nz = np.eye(T, dtype=bool)
    for i, k in ((2, 0), (6, 0), (7, 0), (2, 1), (6, 1), (5, 3), (6, 4), (5, 4), (7, 2), (7, 5)):
        nz[i, k] = True
    nz = M.fill_closed_pattern(nz)
    assert M.levels_of(nz).max() + 1 >= 3
    assert max(int(nz[k + 1:, k].sum()) for k in range(T)) >= 2
    A = np.zeros((T * NB, T * NB))
    for i in range(T):
        for k in range(i):
            if nz[i, k]:
                A[NB * i:NB * i + NB, NB * k:NB * k + NB] = rng.normal(0, 1.0, (NB, NB))
    A = A + A.T
    A += np.diag(np.abs(A).sum(axis=1) + rng.uniform(1.0, 2.0, T * NB))          # diagonally dominant: SPD, well conditioned
    Lf = np.linalg.cholesky(A)
    for i in range(T):                                                           # the factor stays on the fill-closed pattern
        for k in range(i):
            if not nz[i, k]:
                assert not Lf[NB * i:NB * i + NB, NB * k:NB * k + NB].any()
    Z = M.selected_inverse(Lf, nz)
    inv = np.linalg.inv(A)
    assert set(Z) == {(i, k) for i in range(T) for k in range(i + 1) if nz[i, k]}
    scale = np.abs(inv).max()
    for (i, k), z in Z.items():
        assert np.abs(z - inv[NB * i:NB * i + NB, NB * k:NB * k + NB]).max() <= 1e-12 * scale, (i, k)


def test_deep3_facts_and_routes():
    arr = M.FIXTURES["deep3"][0]()
    lv, n_lv, T, n_nz = M.deep3_facts(arr)
    assert lv and n_lv >= 3 and n_nz >= 2 * T, (lv, n_lv, T, n_nz)
    assert Y.schedule_of(arr) == "level"
    # the smallest: no smaller sequential problem of this family qualifies
    from tests import helpers as H
    for n in range(M.DEEP3_CAMS - 5, M.DEEP3_CAMS):
        assert not M.is_deep3(Y.fix_gauge(H.make(n, 15 * n, M.DEEP3_KOBS, seed=M.DEEP3_SEED))), n
    ec = Y.eps_ref(Y.route_a(arr), Y.route_b(arr))
    ep = P.eps_ref(P.route_a(arr), P.route_b(arr))
    print(f"deep3: T {T}, levels {n_lv}, tiles {n_nz}; eps_ref cameras {ec:.3e}, points {ep:.3e}")
    assert ec < 1e-8 and ep < 1e-8
