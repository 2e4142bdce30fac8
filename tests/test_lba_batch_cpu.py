"""CPU-side checks of the batched resident solve (xrsfm_ba_run_batch / xrsfm_ba_solve_batch; xrsfm_amd/csrc/ba_lba.h: k_lba_batch):
the symbols, the empty batch without a device, the batch kernel's resource budget in the gfx950 code object next to the single
launch's, and the Python mirrors."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_are_exported_and_declared(lib):
    from xrsfm_amd import capi
    header = open(os.path.join(ROOT, "include", "xrsfm_ba.h")).read()
    for name in ("xrsfm_ba_run_batch", "xrsfm_ba_solve_batch"):
        assert getattr(lib, name) is not None and name in capi.EXPORTS
        assert re.search(r"^int " + name + r"\(", header, re.M), name
    assert re.search(r"#define XRSFM_BA_BATCH_MAX 4096\b", header) and capi.BATCH_MAX == 4096


def test_an_empty_batch_needs_no_device(lib):
    """n_ctx == 0 is checked first: success with every pointer NULL, with or without a HIP device."""
    assert lib.xrsfm_ba_run_batch(0, None, None, None, None) == 0
    assert lib.xrsfm_ba_solve_batch(None, 0, None, None, None) == 0


def test_counts_outside_the_range_are_refused_without_a_device(lib):
    from xrsfm_amd import capi
    opt = capi.default_options(linear_solver=capi.SOLVER_RESIDENT)
    arr = (C.c_void_p * 1)(None)
    sums = (capi.CSummary * 1)()
    assert lib.xrsfm_ba_run_batch(-1, arr, C.byref(opt), sums, None) == -1
    assert lib.xrsfm_ba_run_batch(capi.BATCH_MAX + 1, arr, C.byref(opt), sums, None) == -1      # (the cap is checked before any entry is read)
    assert lib.xrsfm_ba_run_batch(1, arr, C.byref(opt), sums, None) == -1                       # a NULL entry
    assert lib.xrsfm_ba_run_batch(1, None, C.byref(opt), sums, None) == -1


@pytest.fixture(scope="module")
def notes(tmp_path_factory):
    """Per kernel of the gfx950 code object whose name holds k_lba_: the metadata note's figures (the source
    tests/test_lba_resident_cpu.py reads)."""
    from xrsfm_amd import _build
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    asm = tmp_path_factory.mktemp("lba_batch") / "xba.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-Wno-unused-value",
                    "-Wno-deprecated-declarations", os.path.join(_build.CSRC, "xrsfm_ba.hip"), "-o", str(asm)], check=True, capture_output=True)
    out = {}
    for blk in asm.read_text().split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        if "k_lba_" not in name:
            continue
        short = re.search(r"k_lba_[a-z_]*[a-z]", name).group(0)
        out[short] = {k: int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1))
                      for k in ("vgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size", "vgpr_count", "max_flat_workgroup_size")}
    return out


def test_batch_kernel_budget_equals_the_single_launch(notes):
    assert set(notes) == {"k_lba_resident", "k_lba_batch"}
    one, many = notes["k_lba_resident"], notes["k_lba_batch"]
    assert many["group_segment_fixed_size"] == one["group_segment_fixed_size"]
    assert many["vgpr_spill_count"] == 0 and many["private_segment_fixed_size"] == 0
    assert many["max_flat_workgroup_size"] == one["max_flat_workgroup_size"] == 512


def test_single_launch_budget_is_the_parent_commits(notes):
    """profiles/lba_resident.md, "Kernel budget": 256 VGPRs, 0 spilled, no private segment, 161 392 B of LDS."""
    one = notes["k_lba_resident"]
    assert (one["vgpr_count"], one["vgpr_spill_count"], one["private_segment_fixed_size"], one["group_segment_fixed_size"]) == (256, 0, 0, 161392)


def test_capi_mirrors_marshal_a_list_of_contexts(lib, monkeypatch):
    """run_batch hands the library the contexts' handles in order as one pointer array (a None entry as NULL), one summary and one
    code per context; solve_batch one xrsfm_ba_problem per problem.  Checked on a stand-in for the library: no device needed."""
    from xrsfm_amd import capi
    seen = {}

    class Fake:
        def xrsfm_ba_run_batch(self, n, arr, opt, sums, codes):
            seen["run"] = (n, [arr[i] for i in range(n)])
            sums[1].n_successful = 7
            C.cast(codes, C.POINTER(C.c_int32))[1] = -1
            return -1

        def xrsfm_ba_solve_batch(self, opt, n, probs, sums, codes):
            seen["solve"] = (n, [probs[i].n_cams for i in range(n)], [probs[i].n_obs for i in range(n)])
            return 0

    monkeypatch.setattr(capi, "load", lambda path=None: Fake())

    class Ctx:
        def __init__(self, h):
            self._h = C.c_void_p(h)

    code, sums, codes = capi.run_batch([Ctx(0x10), None, Ctx(0x30)], capi.COptions())
    assert seen["run"] == (3, [0x10, None, 0x30])
    assert code == -1 and len(sums) == 3 and sums[1].n_successful == 7 and list(codes) == [0, -1, 0]
    probs = [H.to_product(H.make(3, 20, 2, seed=1)), H.to_product(H.make(5, 30, 3, seed=2))]
    code, sums, codes = capi.solve_batch(probs, capi.COptions())
    assert code == 0 and len(sums) == 2 and codes.dtype == np.int32 and len(codes) == 2
    assert seen["solve"] == (2, [3, 5], [p.n_obs for p in probs])
