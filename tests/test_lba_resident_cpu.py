"""CPU-side checks of the resident LBA solver (xrsfm_amd/csrc/ba_lba.h): the kernel's resource budget in the gfx950 code
object and the constant in the Python binding."""
import os
import re
import shutil
import subprocess


def test_lba_kernel_has_no_scratch_and_fits_one_cu(tmp_path):
    """k_lba_resident: no spilled VGPRs, no private (scratch) segment, a group segment of at most 160 KiB (one workgroup on one
    compute unit) — read from the code-object notes like tests/test_cov_cpu.py::test_cov_kernels_have_no_scratch reads them."""
    from xrsfm_amd import _build
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    asm = tmp_path / "xba.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-Wno-unused-value",
                    "-Wno-deprecated-declarations", os.path.join(_build.CSRC, "xrsfm_ba.hip"), "-o", str(asm)], check=True, capture_output=True)
    text = asm.read_text()
    seen = 0
    for blk in text.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        if "k_lba_resident" not in name:
            continue
        seen += 1
        spills = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1))
        scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1))
        lds = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", blk).group(1))
        assert spills == 0 and scratch == 0, (name, spills, scratch)
        assert 0 < lds <= 160 * 1024, lds
    assert seen == 1


def test_capi_exposes_the_constant():
    from xrsfm_amd import capi
    assert capi.SOLVER_RESIDENT == 3
    assert {capi.SOLVER_PCG, capi.SOLVER_CHOLESKY, capi.SOLVER_AUTO} == {0, 1, 2}
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "xrsfm_ba.h")).read()
    assert re.search(r"#define XRSFM_BA_SOLVER_RESIDENT 3\b", header)
