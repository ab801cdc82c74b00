"""Compiler-output checks for k_mesh_check and k_mesh_commit of rxr_project.hip (no GPU needed: hipcc cross-compiles for gfx950): no
scratch, and few enough registers for eight waves a SIMD -- both are streaming kernels whose loads want the occupancy.  Reads the
kernel descriptors' register and scratch metadata only, like tests/test_terrain_mesh_resources.py."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    import __graft_entry__ as G

    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out = tmp_path_factory.mktemp("isa") / "rxr_project.s"
    flags = [f for f in G.HIP_FLAGS if f not in ("-shared", "-fPIC")]
    subprocess.run([hipcc] + flags + ["--cuda-device-only", "-S", "-o", str(out), os.path.join(G.CSRC, "rxr_project.hip")],
                   check=True, stderr=subprocess.DEVNULL)
    return open(out).read()


def descriptor(isa, name, key):
    m = re.search(rf"\.amdhsa_kernel {name}\n(.*?)\.end_amdhsa_kernel", isa, flags=re.S)
    assert m, f"{name} is not in rxr_project.hip"
    return int(re.search(rf"\.amdhsa_{key} (\d+)", m.group(1)).group(1))


@pytest.mark.parametrize("kernel", ["k_mesh_check", "k_mesh_commit"])
def test_the_update_kernels_use_no_scratch_and_few_registers(isa, kernel):
    assert descriptor(isa, kernel, "private_segment_fixed_size") == 0
    assert descriptor(isa, kernel, "next_free_vgpr") <= 64          # 512 VGPRs a SIMD lane: eight waves
