"""Compiler-output checks for the kernels of rxr_terrain_gen.hip (no GPU needed: hipcc cross-compiles for gfx950): none uses scratch,
and each stays at the register count of the occupancy step the build reaches.  Reads the kernel descriptors' register and scratch
metadata only, like tests/test_kernel_resources.py."""
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
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("isa") / "rxr_terrain_gen.s"
    flags = [f for f in G.HIP_FLAGS if f not in ("-shared", "-fPIC")]
    subprocess.run([hipcc] + flags + ["--cuda-device-only", "-S", "-o", str(out), os.path.join(G.CSRC, "rxr_terrain_gen.hip")],
                   check=True, stderr=subprocess.DEVNULL)
    return open(out).read()


def descriptor(isa, name, key):
    m = re.search(rf"\.amdhsa_kernel {name}\n(.*?)\.end_amdhsa_kernel", isa, flags=re.S)
    return int(re.search(rf"\.amdhsa_{key} (\d+)", m.group(1)).group(1))


# The kernels are VALU-bound loops over records that arrive in scalar registers: nothing but arithmetic latency is there to hide, and
# the build reaches the top occupancy step with room to spare (25 VGPRs for a height, 39 for a normal's three samples).  64 is that
# step's limit: 512 VGPRs a SIMD lane, eight waves.
@pytest.mark.parametrize("kernel", ["k_terrain_gen_heights", "k_terrain_gen_normals", "k_terrain_gen_grid"])
def test_generator_kernels_use_no_scratch_and_stay_at_eight_waves(isa, kernel):
    assert descriptor(isa, kernel, "private_segment_fixed_size") == 0
    assert descriptor(isa, kernel, "next_free_vgpr") <= 64
