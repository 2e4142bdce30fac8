"""Camera covariance without a GPU: the symbol and its error code, the fixtures of the GPU test (their plans and the agreement
of the two dense CPU routes that define the tolerance), and the code object of the new kernels."""
import os
import re
import shutil
import subprocess

import pytest

from tests import cov_yardstick as Y

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_and_error_code(lib):
    from xrsfm_amd import capi
    assert getattr(lib, "xrsfm_ba_covariance") is not None
    assert "xrsfm_ba_covariance" in capi.EXPORTS
    hdr = open(os.path.join(ROOT, "include", "xrsfm_ba.h")).read()
    assert re.search(r"#define\s+XRSFM_BA_ESINGULAR\s+\(-8\)", hdr)
    assert capi.ESINGULAR == -8 and "ESINGULAR" in capi.ERRORS[-8]
    assert re.search(r"int\s+xrsfm_ba_covariance\s*\(\s*xrsfm_ba_context\s*\*ctx,\s*double huber_a,\s*int32_t n_sel,\s*const int32_t \*cam_sel,\s*double \*cov\)", hdr)


def test_argument_errors_need_no_device(lib):
    """NULL context -> EINVAL before anything touches a device."""
    assert lib.xrsfm_ba_covariance(None, 5.99, 0, None, None) == -1


@pytest.mark.parametrize("name", sorted(Y.FIXTURES))
def test_fixture_is_usable(lib, name):
    """Routes A and B (two correct float64 computations) agree below 1e-8 per camera block, so that 50 x eps_ref separates a
    right answer from a wrong one; the plan puts the fixture on the schedule the GPU test wants it on; the problem is small
    enough for the dense inverse."""
    make, want = Y.FIXTURES[name]
    arr = make()
    assert arr["cam_q"].shape[0] <= 40 and arr["points"].shape[0] <= 2000
    if want is not None:
        assert Y.schedule_of(arr) == want
    A, B = Y.route_a(arr), Y.route_b(arr)
    eps = Y.eps_ref(A, B)
    print(f"{name}: eps_ref {eps:.3e}")
    assert eps < 1e-8
    free = arr["cam_const"] == 0
    assert (A[free].reshape(free.sum(), -1) != 0).all()


def test_const_q_fixture_has_zero_rotation_rows():
    arr = Y.FIXTURES["const_q"][0]()
    A = Y.route_a(arr)
    c = Y.CONST_Q_CAM
    assert arr["cam_const"][c] == 1
    assert (A[c, :3, :] == 0).all() and (A[c, :, :3] == 0).all() and (A[c, 3:, 3:] != 0).all()


def test_cov_kernels_have_no_scratch(tmp_path):
    """The gfx950 code object of k_lv_fwd_multi, k_cov_gram and k_cov_prep: no spilled VGPRs, no private (scratch) segment —
    read from the code-object notes like tests/test_capi_cpu.py reads them; the compile is also the check that
    hipcc --offload-arch=gfx950 builds the library's device code."""
    from xrsfm_amd import _build
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    asm = tmp_path / "xba.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-Wno-unused-value",
                    "-Wno-deprecated-declarations", os.path.join(_build.CSRC, "xrsfm_ba.hip"), "-o", str(asm)], check=True, capture_output=True)
    text = asm.read_text()
    seen = set()
    for blk in text.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        for k in ("k_lv_fwd_multi", "k_cov_gram", "k_cov_prep"):
            if k in name:
                seen.add(k)
                spills = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1))
                scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1))
                lds = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", blk).group(1))
                assert spills == 0 and scratch == 0, (name, spills, scratch)
                if k == "k_lv_fwd_multi":
                    assert lds <= 80 * 1024, lds          # two workgroups per compute unit (160 KB of LDS)
    assert seen == {"k_lv_fwd_multi", "k_cov_gram", "k_cov_prep"}


def test_library_builds_for_gfx950(lib):
    from xrsfm_amd import _build
    assert os.path.exists(_build.LIB)
    out = subprocess.run(["nm", "-D", "--defined-only", _build.LIB], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT xrsfm_ba_covariance\b", out)
