"""Point covariance without a GPU: the symbol, its declaration and its error code, the agreement of the two dense CPU routes that
define the tolerance on every fixture, the identities of special points on the yardstick, and the code object of the new kernels."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import cov_point_yardstick as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_and_declaration(lib):
    from xrsfm_amd import capi
    assert getattr(lib, "xrsfm_ba_point_covariance") is not None
    assert "xrsfm_ba_point_covariance" in capi.EXPORTS
    assert hasattr(capi.Context, "point_covariance")
    hdr = open(os.path.join(ROOT, "include", "xrsfm_ba.h")).read()
    assert re.search(r"int\s+xrsfm_ba_point_covariance\s*\(\s*xrsfm_ba_context\s*\*ctx,\s*double huber_a,\s*int32_t n_sel,\s*const int32_t \*pt_sel,\s*double \*cov\)", hdr)
    # the camera call no longer lists point covariances as missing
    cam_doc = hdr[hdr.index("Marginal covariance of selected cameras"):hdr.index("int xrsfm_ba_covariance(")]
    assert "point covariances" not in cam_doc


def test_argument_errors_need_no_device(lib):
    """NULL context -> EINVAL before anything touches a device."""
    assert lib.xrsfm_ba_point_covariance(None, 5.99, 0, None, None) == -1


def test_library_exports_the_symbol(lib):
    from xrsfm_amd import _build
    out = subprocess.run(["nm", "-D", "--defined-only", _build.LIB], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT xrsfm_ba_point_covariance\b", out)


@pytest.mark.parametrize("name", sorted(P.FIXTURES))
def test_routes_agree(name):
    """Routes A and B agree below 1e-8 per point block on every fixture of the camera tests, so 50 x eps_ref separates a right
    answer from a wrong one, and every observed free point has a positive definite block."""
    arr = P.FIXTURES[name][0]()
    A, B = P.route_a(arr), P.route_b(arr)
    eps = P.eps_ref(A, B)
    print(f"{name}: point eps_ref {eps:.3e}")
    assert eps < 1e-8
    obs = P.observed_points(arr)
    free = obs[arr["point_const"][obs] == 0]
    assert free.size > 0
    assert (A == np.swapaxes(A, 1, 2)).all() or np.abs(A - np.swapaxes(A, 1, 2)).max() <= 1e-12 * np.abs(A).max()
    for j in free:
        assert np.linalg.eigvalsh(0.5 * (A[j] + A[j].T)).min() > 0


def test_constant_point_has_a_zero_block():
    arr = dict(P.FIXTURES["ring12"][0]())
    pc = np.array(arr["point_const"], np.uint8, copy=True)
    j = int(P.observed_points(arr)[5])
    pc[j] = 1
    arr["point_const"] = pc
    A, B = P.route_a(arr), P.route_b(arr)
    assert (A[j] == 0).all() and (B[j] == 0).all()
    assert P.eps_ref(A, B) < 1e-8
    k = int(P.observed_points(arr)[6])
    assert (A[k] != 0).all()


def test_point_seen_by_constant_cameras_only_is_its_own_inverse():
    """Every camera that observes the point constant: W_p = 0 and the block is inv(E^T E), in both routes."""
    base = P.FIXTURES["ring12"][0]()
    j = int(P.observed_points(base)[40])
    arr = P.lba_shaped(base, j)
    assert (arr["cam_const"] == 0).sum() >= 4          # still a problem with free cameras
    A, B = P.route_a(arr), P.route_b(arr)
    eps = P.eps_ref(A, B)
    assert eps < 1e-8
    want = P.point_hinv(arr, j)
    for G in (A, B):
        assert P.rel_blocks(G[j:j + 1], want[None])[0] <= P.tolerance(eps)


def test_point_kernels_have_no_scratch(tmp_path):
    """The gfx950 code object of both instantiations of k_lv_fwd_multi and of the point kernels: no spilled VGPRs, no private
    (scratch) segment; the forward substitution keeps its LDS budget (two workgroups per compute unit)."""
    from xrsfm_amd import _build
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    asm = tmp_path / "xba.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-Wno-unused-value",
                    "-Wno-deprecated-declarations", os.path.join(_build.CSRC, "xrsfm_ba.hip"), "-o", str(asm)], check=True, capture_output=True)
    text = asm.read_text()
    want = ("k_lv_fwd_multi", "k_cov_pt_rhs", "k_cov_pt_scatter", "k_cov_pt_gram", "k_cov_pt_gather")
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
                if k == "k_lv_fwd_multi":
                    assert lds == 2 * 64 * 66 * 8, lds
    assert seen["k_lv_fwd_multi"] == 2 and all(v >= 1 for v in seen.values()), seen
