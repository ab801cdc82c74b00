"""Compiler-output checks for the kernels of rxr_terrain_excl.hip (no GPU needed: hipcc cross-compiles for gfx950): none uses scratch,
and each stays at the register count of the top occupancy step.  Reads the kernel descriptors' register and scratch metadata only,
like tests/test_terrain_gen_resources.py."""
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
    out = tmp_path_factory.mktemp("isa") / "rxr_terrain_excl.s"
    flags = [f for f in G.HIP_FLAGS if f not in ("-shared", "-fPIC")]
    subprocess.run([hipcc] + flags + ["--cuda-device-only", "-S", "-o", str(out), os.path.join(G.CSRC, "rxr_terrain_excl.hip")],
                   check=True, stderr=subprocess.DEVNULL)
    return open(out).read()


def descriptor(isa, name, key):
    m = re.search(rf"\.amdhsa_kernel {name}\n(.*?)\.end_amdhsa_kernel", isa, flags=re.S)
    return int(re.search(rf"\.amdhsa_{key} (\d+)", m.group(1)).group(1))


# The classification is a VALU-bound loop over records that arrive in scalar registers, the height field's loops in front of it: as
# there, nothing but arithmetic latency is to be hidden, and 64 VGPRs is the limit of the top occupancy step (512 VGPRs a SIMD lane,
# eight waves).  The emission is a scan and stores: latency-bound, so it wants that step as well.
@pytest.mark.parametrize("kernel", ["k_terrain_excl_classify", "k_terrain_excl_emit"])
def test_exclusion_kernels_use_no_scratch_and_stay_at_eight_waves(isa, kernel):
    assert descriptor(isa, kernel, "private_segment_fixed_size") == 0
    assert descriptor(isa, kernel, "next_free_vgpr") <= 64


def test_the_emission_keeps_its_wave_totals_in_lds_and_nothing_else(isa):
    assert descriptor(isa, "k_terrain_excl_emit", "group_segment_fixed_size") == 16
    assert descriptor(isa, "k_terrain_excl_classify", "group_segment_fixed_size") == 0
