"""Joint covariance without a GPU: the symbol, its declaration and its cap, the agreement of the two dense CPU routes that define the
tolerance on every fixture, the joint yardstick against the two marginal yardsticks, and the code object of the new kernels."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import cov_joint_yardstick as Jy
from tests import cov_point_yardstick as P
from tests import cov_yardstick as Y

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_and_declaration(lib):
    from xrsfm_amd import capi
    assert getattr(lib, "xrsfm_ba_joint_covariance") is not None
    assert "xrsfm_ba_joint_covariance" in capi.EXPORTS
    assert hasattr(capi.Context, "joint_covariance")
    hdr = open(os.path.join(ROOT, "include", "xrsfm_ba.h")).read()
    assert re.search(r"int\s+xrsfm_ba_joint_covariance\s*\(\s*xrsfm_ba_context\s*\*ctx,\s*double huber_a,\s*int32_t n_cam_sel,\s*const int32_t \*cam_sel,"
                     r"\s*int32_t n_pt_sel,\s*const int32_t \*pt_sel,\s*double \*cov\)", hdr)
    cap = re.search(r"#define\s+XRSFM_BA_JOINT_COV_MAX_COLS\s+(\d+)", hdr)
    assert cap and int(cap.group(1)) >= 1024
    # the two marginal calls no longer list cross blocks as missing: they name the call that has them
    for first, decl in (("Marginal covariance of selected cameras", "int xrsfm_ba_covariance("), ("Marginal covariance of selected 3-D points", "int xrsfm_ba_point_covariance(")):
        doc = hdr[hdr.index(first):hdr.index(decl)]
        not_built = doc[doc.index("Not built"):]
        assert "cross blocks" not in not_built and "xrsfm_ba_joint_covariance" in doc


def test_argument_errors_need_no_device(lib):
    """NULL context -> EINVAL before anything touches a device."""
    assert lib.xrsfm_ba_joint_covariance(None, 5.99, 0, None, 0, None, None) == -1


def test_library_exports_the_symbol(lib):
    from xrsfm_amd import _build
    out = subprocess.run(["nm", "-D", "--defined-only", _build.LIB], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT xrsfm_ba_joint_covariance\b", out)


@pytest.mark.parametrize("name", sorted(Jy.FIXTURES))
def test_routes_agree_and_match_the_marginal_yardsticks(name):
    """Routes A and B agree below 1e-8 over the full joint matrix of every fixture, so 50 x eps_ref separates a right answer from a
    wrong sign, a missing Hinv_p or a missing scale; the joint route A has the diagonal blocks of the two marginal yardsticks (the
    same dense inverse, cut differently); constant degrees of freedom are zero rows and columns of the expanded matrix."""
    arr = Jy.FIXTURES[name][0]()
    A, B = Jy.route_a(arr), Jy.route_b(arr)
    eps = Jy.eps_ref(A, B)
    print(f"{name}: joint eps_ref {eps:.3e}")
    assert eps < 1e-8
    assert Jy.entry_err(A.M.T, A.M) <= Jy.tolerance(eps)          # (the asymmetry of a dense inverse is part of the reference's own error)
    n_cams = arr["cam_q"].shape[0]
    cams, pts = np.arange(n_cams), Jy.observed_points(arr)[::5]
    S = A.select(cams, pts)
    Ac, Ap = Y.route_a(arr), P.route_a(arr)
    for i, c in enumerate(cams):
        assert Y.rel_blocks(S[None, 6 * i:6 * i + 6, 6 * i:6 * i + 6], Ac[c:c + 1])[0] <= 1e-12
    o = 6 * n_cams
    for i, p in enumerate(pts):
        assert Y.rel_blocks(S[None, o + 3 * i:o + 3 * i + 3, o + 3 * i:o + 3 * i + 3], Ap[p:p + 1])[0] <= 1e-12
    # camera 0 is constant (the gauge): zero rows and columns; the cross blocks of free parameters are not zero
    assert (S[:6, :] == 0).all() and (S[:, :6] == 0).all()
    assert (S[12:18, o:] != 0).all() and (S[12:18, 18:24] != 0).all() and (S[o:o + 3, o + 3:o + 6] != 0).all()
    # the sign of a camera-point block is not a matter of taste: flipping it is far outside the tolerance
    flipped = S.copy()
    flipped[:o, o:] *= -1.0
    flipped[o:, :o] *= -1.0
    assert Jy.entry_err(flipped, S) > 1e3 * Jy.tolerance(eps)


def test_point_under_constant_cameras_has_zero_cross_blocks():
    base = Jy.FIXTURES["ring12"][0]()
    j = int(Jy.observed_points(base)[40])
    arr = Jy.lba_shaped(base, j)
    A, B = Jy.route_a(arr), Jy.route_b(arr)
    eps = Jy.eps_ref(A, B)
    assert eps < 1e-8
    cams = np.nonzero(arr["cam_const"] == 0)[0][:3]
    others = Jy.observed_points(arr)[:5]
    others = others[others != j]
    for G in (A, B):
        S = G.select(cams, np.concatenate([[j], others]))
        o = 6 * cams.shape[0]
        cross = np.abs(np.concatenate([S[o:o + 3, :o].ravel(), S[o:o + 3, o + 3:].ravel()])).max()
        assert cross <= Jy.tolerance(eps) * np.abs(np.diag(S)).max()          # (zero up to the rounding of a dense inverse)
        assert Jy.entry_err(S[o:o + 3, o:o + 3], Jy.point_hinv(arr, j)) <= Jy.tolerance(eps)


def test_joint_kernels_have_no_scratch(tmp_path):
    """The gfx950 code object of k_cov_joint_gram and k_cov_joint_finish: no spilled VGPRs, no private (scratch) segment; the Gram
    kernel keeps the LDS budget of the forward substitution (two 64 x 66 tiles: two workgroups per compute unit); k_lv_fwd_multi
    still has exactly two instantiations."""
    from xrsfm_amd import _build
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    asm = tmp_path / "xba.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-Wno-unused-value",
                    "-Wno-deprecated-declarations", os.path.join(_build.CSRC, "xrsfm_ba.hip"), "-o", str(asm)], check=True, capture_output=True)
    text = asm.read_text()
    want = ("k_lv_fwd_multi", "k_cov_joint_gram", "k_cov_joint_finish")
    seen = {k: 0 for k in want}
    for blk in text.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        for k in want:
            if k in name:
                seen[k] += 1
                spills = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1))
                scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1))
                lds = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", blk).group(1))
                assert spills == 0 and scratch == 0, (name, spills, scratch)
                if k == "k_cov_joint_gram":
                    assert lds == 2 * 64 * 66 * 8, lds
    assert seen == {"k_lv_fwd_multi": 2, "k_cov_joint_gram": 1, "k_cov_joint_finish": 1}, seen
    # the Gram runs on the FP64 matrix instruction and has no floating-point atomic
    body = text[text.index("k_cov_joint_gram"):]
    body = body[:body.index("s_endpgm")]
    assert "v_mfma_f64_16x16x4" in body and "atomic" not in body
