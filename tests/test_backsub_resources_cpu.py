"""Register budget of the back-substitution kernels, read from the compiler's resource remarks (no GPU needed).

k_backsub<PREP, YP> (the items of one tile, the common path) is allocated for 5 waves per SIMD: at most 96 VGPRs, and it must get
there without a private segment — a spilled register is a scratch round trip inside the kernel the fifth wave is meant to speed up.
k_backsub_long<PREP> (tracks longer than a tile) keeps its own budget; it only has to stay out of scratch memory too.
The device code is compiled with the flags of xrsfm_amd/_build.py plus --cuda-device-only -c -Rpass-analysis=kernel-resource-usage."""
import os
import re
import shutil
import subprocess

import pytest


def _remarks(tmp_path):
    from xrsfm_amd import _build
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-unused-value", "-Wno-deprecated-declarations",
                        "--cuda-device-only", "-c", "-Rpass-analysis=kernel-resource-usage", os.path.join(_build.CSRC, "xrsfm_ba.hip"),
                        "-o", str(tmp_path / "xba.o")], check=True, capture_output=True, text=True)
    kernels, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+(.*?)\s+\[-Rpass-analysis=kernel-resource-usage\]", line)
        if not m:
            continue
        key, _, val = m.group(1).partition(":")
        if key == "Function Name":
            cur = kernels.setdefault(val.strip(), {})
        elif cur is not None:
            cur[key.strip()] = val.strip()
    return kernels


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    return _remarks(tmp_path_factory.mktemp("backsub_resources"))


def _of(remarks, mangled_prefix):
    return {n: r for n, r in remarks.items() if n.startswith(mangled_prefix)}


def test_common_path_fits_five_waves(remarks):
    # _ZN3xba9k_backsubILb<PREP>ELb<YP>EEEv...: both point-factor forms, with and without the debug entry's yp store
    got = _of(remarks, "_ZN3xba9k_backsubILb")
    assert sorted(n[len("_ZN3xba9k_backsubI"):len("_ZN3xba9k_backsubI") + 8] for n in got) == ["Lb0ELb0E", "Lb0ELb1E", "Lb1ELb0E", "Lb1ELb1E"]
    for name, r in got.items():
        print("RESOURCES", name, r)
        assert int(r["VGPRs"]) <= 96, (name, r)
        assert int(r["Occupancy [waves/SIMD]"]) == 5, (name, r)
        assert int(r["ScratchSize [bytes/lane]"]) == 0, (name, r)
        assert int(r["VGPRs Spill"]) == 0, (name, r)
        assert int(r["LDS Size [bytes/block]"]) * 5 <= 160 * 1024, (name, r)       # 5 workgroups of 4 waves per compute unit


def test_long_track_kernel_has_no_scratch(remarks):
    got = _of(remarks, "_ZN3xba14k_backsub_longILb")
    assert len(got) == 2
    for name, r in got.items():
        print("RESOURCES", name, r)
        assert int(r["ScratchSize [bytes/lane]"]) == 0 and int(r["VGPRs Spill"]) == 0, (name, r)


def test_parent_kernel_is_still_built(remarks):
    """XRSFM_BA_BACKSUB_LEAN=0 needs it (the A/B reference of tests/test_gpu_backsub_lean.py): 4 waves, no scratch."""
    got = _of(remarks, "_ZN3xba16k_backsub_parentILb")
    assert len(got) == 2
    for name, r in got.items():
        assert int(r["Occupancy [waves/SIMD]"]) == 4 and int(r["ScratchSize [bytes/lane]"]) == 0, (name, r)
