"""Register budget of the streaming kernels that stage a tile's camera records in LDS, read from the compiler's resource remarks
(no GPU needed; k_backsub has tests/test_backsub_resources_cpu.py).

The merged k_schur_pairs launch carries the staged route next to the gather route under a wave-uniform branch (k_linearize was
measured with one and ships without: profiles/r10_cam_stage.md); no instantiation, and not k_linearize, may cost a private
segment or a spilled register, and each kernel stays at the occupancy it ships with — 4 waves per SIMD
for k_linearize and the Gram launches of up to 8 cameras, 3 for the 9-10-camera Gram launch and the per-pair launch.
The device code is compiled with the flags of xrsfm_amd/_build.py plus --cuda-device-only -c -Rpass-analysis=kernel-resource-usage."""
import os
import re
import shutil
import subprocess

import pytest


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    from xrsfm_amd import _build
    tmp = tmp_path_factory.mktemp("cam_stage_resources")
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-unused-value", "-Wno-deprecated-declarations",
                        "--cuda-device-only", "-c", "-Rpass-analysis=kernel-resource-usage", os.path.join(_build.CSRC, "xrsfm_ba.hip"),
                        "-o", str(tmp / "xba.o")], check=True, capture_output=True, text=True)
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


def _clean(name, r, waves):
    print("RESOURCES", name, r)
    assert int(r["ScratchSize [bytes/lane]"]) == 0, (name, r)
    assert int(r["VGPRs Spill"]) == 0, (name, r)
    assert int(r["Occupancy [waves/SIMD]"]) == waves, (name, r)


def test_linearize_keeps_four_waves_without_scratch(remarks):
    got = {n: r for n, r in remarks.items() if n.startswith("_ZN3xba11k_linearizeE")}
    assert len(got) == 1
    for name, r in got.items():
        _clean(name, r, 4)
        assert int(r["VGPRs"]) <= 128, (name, r)


def test_schur_pairs_keeps_its_occupancy_without_scratch(remarks):
    # _ZN3xba13k_schur_pairsILb<GRAM>ELb<PREP>ELi<NIK>EEEv...
    got = {n: r for n, r in remarks.items() if n.startswith("_ZN3xba13k_schur_pairsILb")}
    keys = sorted(re.match(r"_ZN3xba13k_schur_pairsILb(\d)ELb(\d)ELi(\d)E", n).groups() for n in got)
    assert keys == sorted([("1", p, str(k)) for p in "01" for k in range(5)] + [("0", p, "0") for p in "01"]), keys
    for name, r in got.items():
        gram, _, nik = re.match(r"_ZN3xba13k_schur_pairsILb(\d)ELb(\d)ELi(\d)E", name).groups()
        _clean(name, r, 4 if (gram == "1" and nik != "4") else 3)
