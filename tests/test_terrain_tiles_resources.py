"""Compiler-output checks for the tile emission kernel of rxr_terrain_excl.hip (no GPU needed: hipcc cross-compiles for gfx950).  Reads
the kernel descriptor's register, scratch and LDS metadata only, like tests/test_terrain_exclusion_resources.py."""
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


# The corner tables of the two triangles of a cell are indexed inside loops the compiler has to unroll: a table that survived as an
# array would live in the private segment.  The kernel is a scan, table look-ups and scattered stores -- latency-bound, one workgroup
# of four waves per box --, so it wants the top occupancy step like the emission it stands next to: 64 VGPRs at the most (512 a SIMD
# lane, eight waves).  The build that ships uses 46; registers are allotted in blocks of 8, so 48 is the bound that holds that figure:
# a build that needs a block more has changed what the kernel keeps live, and somebody should look.
def test_the_tile_emission_uses_no_scratch_and_stays_at_its_register_block(isa):
    assert descriptor(isa, "k_terrain_tiles_emit", "private_segment_fixed_size") == 0
    assert descriptor(isa, "k_terrain_tiles_emit", "next_free_vgpr") <= 48


# LDS: the bitmap of the slots present and its popcount prefix (RXR_TERRAIN_TILES_MAX_TILES / 32 words each), the four waves' totals
# and two running counters per group (RXR_TERRAIN_TILES_MAX_GROUPS each): (128 + 128 + 4 * 64 + 2 * 64) * 4 bytes
def test_the_tile_emission_keeps_its_bitmap_and_group_counters_in_lds(isa):
    assert descriptor(isa, "k_terrain_tiles_emit", "group_segment_fixed_size") == 2560
