"""Compiler-output checks for k_terrain_mesh of rxr_terrain_mesh.hip (no GPU needed: hipcc cross-compiles for gfx950): no scratch --
the 3 x 3 corners a vertex gathers its normal from stay in registers -- and the eight waves a SIMD that hide the height loads'
latency.  Reads the kernel descriptor's register and
scratch metadata only, like tests/test_terrain_hit_resources.py."""
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
    out = tmp_path_factory.mktemp("isa") / "rxr_terrain_mesh.s"
    flags = [f for f in G.HIP_FLAGS if f not in ("-shared", "-fPIC")]
    subprocess.run([hipcc] + flags + ["--cuda-device-only", "-S", "-o", str(out), os.path.join(G.CSRC, "rxr_terrain_mesh.hip")],
                   check=True, stderr=subprocess.DEVNULL)
    return open(out).read()


def descriptor(isa, name, key):
    m = re.search(rf"\.amdhsa_kernel {name}\n(.*?)\.end_amdhsa_kernel", isa, flags=re.S)
    return int(re.search(rf"\.amdhsa_{key} (\d+)", m.group(1)).group(1))


def test_the_mesh_kernel_uses_no_scratch_and_few_registers(isa):
    assert descriptor(isa, "k_terrain_mesh", "private_segment_fixed_size") == 0
    assert descriptor(isa, "k_terrain_mesh", "next_free_vgpr") <= 64          # 512 VGPRs a SIMD lane: eight waves
    assert descriptor(isa, "k_terrain_mesh", "group_segment_fixed_size") == 0  # (all of its LDS is sized at the launch)

