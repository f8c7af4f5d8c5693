"""Register budget of gather_kernel<NV>, read from the compiler's kernel metadata (no GPU needed).

pre_sim_mlp's MFMA accumulators once gave the NV <= 4 instantiations 64 AGPRs on top of ~92 VGPRs: 156-160 registers,
3 waves per SIMD.  The second launch bound of the kernel keeps every instantiation within 96 VGPRs (512 / 5 = 102, rounded
down to the allocation granule of 8: 5 waves per SIMD) with no AGPRs and no scratch; this test pins that against an edit
that brings the accumulators back.  gather.hip is compiled to assembly with build.py's flags into a temporary directory.
"""
from __future__ import annotations

import os
import re
import shutil
import subprocess

import pytest

from uforecon_amd import build as B


def _hipcc():
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    return None


pytestmark = pytest.mark.skipif(_hipcc() is None, reason="hipcc not installed")


@pytest.fixture(scope="module")
def gather_metadata(tmp_path_factory):
    """{NV: {vgpr_count, agpr_count, private_segment_fixed_size}} from the .amdgpu_metadata of the device assembly."""
    out = tmp_path_factory.mktemp("gather_isa") / "gather.s"
    flags = [f for f in B.CXXFLAGS if f != "-fPIC"]
    cmd = [_hipcc(), *flags, "--cuda-device-only", "-S", os.path.join(B.CSRC, "gather.hip"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, f"{' '.join(cmd)}\n{r.stderr}"
    text = out.read_text()
    meta = text[text.index("amdhsa.kernels:"):]
    kernels = {}
    # one "- .agpr_count: ..." list item per kernel; keys are sorted, so split on the item marker
    for item in re.split(r"\n  - ", meta)[1:]:
        name = re.search(r"\.name:\s+(\S+)", item)
        if not name:
            continue
        m = re.search(r"gather_kernelILi(\d+)E", name.group(1))
        if not m:
            continue
        fields = {k: int(v) for k, v in re.findall(r"\.(vgpr_count|agpr_count|private_segment_fixed_size):\s+(\d+)", item)}
        kernels[int(m.group(1))] = fields
    return kernels


def test_every_view_count_is_instantiated(gather_metadata):
    assert sorted(gather_metadata) == [2, 3, 4, 5, 6, 7]


@pytest.mark.parametrize("nv", [2, 3, 4, 5, 6, 7])
def test_gather_register_budget(gather_metadata, nv):
    k = gather_metadata[nv]
    assert k.get("agpr_count", 0) == 0, k        # no accumulator registers of their own
    assert k["vgpr_count"] <= 96, k              # 5 waves per SIMD
    assert k["private_segment_fixed_size"] == 0, k   # no scratch
