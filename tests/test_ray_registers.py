"""Register budget of ray_transformer_kernel<LOWP, TAPE>, read from the compiler's kernel metadata (no GPU needed).

The forward-only instantiations walk sweep 1 over two column tiles per weight pass, one head group at a time
(csrc/ufr_layout_f16.h: kRt1GroupHeads).  They must stay within 208 VGPRs with no AGPRs and no scratch: two ray-transformer
waves (2 x 208) and one gather wave (88) then share a SIMD's 512 registers, the co-residency DESIGN.md section 7 measured.  A
two-tile sweep in the blob's k-step-major order needed 256 registers and spilled 30; this test pins the budget against an
edit that brings that back.  The tape instantiations (the backward's forward) only have to stay free of scratch.
ray_transformer.hip is compiled to assembly with build.py's flags into a temporary directory.
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
def ray_metadata(tmp_path_factory):
    """{(lowp, tape): {vgpr_count, agpr_count, private_segment_fixed_size}} from the .amdgpu_metadata of the assembly."""
    out = tmp_path_factory.mktemp("ray_isa") / "ray_transformer.s"
    flags = [f for f in B.CXXFLAGS if f != "-fPIC"]
    cmd = [_hipcc(), *flags, "--cuda-device-only", "-S", os.path.join(B.CSRC, "ray_transformer.hip"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, f"{' '.join(cmd)}\n{r.stderr}"
    text = out.read_text()
    meta = text[text.index("amdhsa.kernels:"):]
    kernels = {}
    for item in re.split(r"\n  - ", meta)[1:]:
        name = re.search(r"\.name:\s+(\S+)", item)
        if not name:
            continue
        m = re.search(r"ray_transformer_kernelILb([01])ELb([01])E", name.group(1))
        if not m:
            continue
        fields = {k: int(v) for k, v in re.findall(r"\.(vgpr_count|agpr_count|private_segment_fixed_size):\s+(\d+)", item)}
        kernels[(bool(int(m.group(1))), bool(int(m.group(2))))] = fields
    return kernels


def test_every_instantiation_is_there(ray_metadata):
    assert sorted(ray_metadata) == [(False, False), (False, True), (True, False), (True, True)]


@pytest.mark.parametrize("lowp", [False, True])
def test_forward_ray_register_budget(ray_metadata, lowp):
    k = ray_metadata[(lowp, False)]
    print(f"MEASURE ray_transformer_kernel<{lowp}, false>: {k}")
    assert k["vgpr_count"] <= 208, k                 # 2 x 208 + 88 <= 512: a gather wave fits beside two of these
    assert k.get("agpr_count", 0) == 0, k
    assert k["private_segment_fixed_size"] == 0, k   # no scratch


@pytest.mark.parametrize("lowp", [False, True])
def test_tape_ray_kernels_have_no_scratch(ray_metadata, lowp):
    k = ray_metadata[(lowp, True)]
    print(f"MEASURE ray_transformer_kernel<{lowp}, true>: {k}")
    assert k["private_segment_fixed_size"] == 0, k
