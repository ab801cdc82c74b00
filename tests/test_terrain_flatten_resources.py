"""Compiler-output checks for k_terrain_flatten of rxr_terrain_flatten.hip (no GPU needed: hipcc cross-compiles for gfx950): no
scratch, no LDS of fixed size (its lists are sized at the launch from the registered counts), and register figures EQUAL to the ones
profiles/terrain_flatten/README.md records -- a change of the kernel that moves them has to be measured again and written down there.
Reads the kernel descriptor's metadata only, like tests/test_terrain_mesh_resources.py, and the bytes of LDS the host asks for at
the bounds."""
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
    out = tmp_path_factory.mktemp("isa") / "rxr_terrain_flatten.s"
    flags = [f for f in G.HIP_FLAGS if f not in ("-shared", "-fPIC")]
    subprocess.run([hipcc] + flags + ["--cuda-device-only", "-S", "-o", str(out), os.path.join(G.CSRC, "rxr_terrain_flatten.hip")],
                   check=True, stderr=subprocess.DEVNULL)
    return open(out).read()


def descriptor(isa, name, key):
    m = re.search(rf"\.amdhsa_kernel {name}\n(.*?)\.end_amdhsa_kernel", isa, flags=re.S)
    return int(re.search(rf"\.amdhsa_{key} (\d+)", m.group(1)).group(1))


def recorded(key):
    """`key N` on the README's line of figures for k_terrain_flatten"""
    text = open(os.path.join(ROOT, "profiles", "terrain_flatten", "README.md")).read()
    line = next(ln for ln in text.splitlines() if ln.startswith("k_terrain_flatten:"))
    return int(re.search(rf"{key} (\d+)", line).group(1))


def test_the_flatten_kernel_uses_no_scratch(isa):
    assert descriptor(isa, "k_terrain_flatten", "private_segment_fixed_size") == 0
    assert re.search(r"\.private_segment_fixed_size:\s+0\b", isa) and re.search(r"\.vgpr_spill_count:\s+0\b", isa) and re.search(r"\.sgpr_spill_count:\s+0\b", isa)


def test_registers_and_lds_are_the_recorded_ones(isa):
    for key in ("next_free_vgpr", "next_free_sgpr", "group_segment_fixed_size"):
        assert descriptor(isa, "k_terrain_flatten", key) == recorded(key), key
    assert descriptor(isa, "k_terrain_flatten", "next_free_vgpr") <= 64          # 512 VGPRs a SIMD lane: eight waves
    # the LDS a launch asks for at the bounds (flatten_lds_bytes: 12 bytes an op, 16 of wave totals, 2 a segment slot)
    from rusterix_amd import abi

    at_bounds = abi.RXR_TERRAIN_FLATTEN_MAX_OPS * 12 + 16 + abi.RXR_TERRAIN_FLATTEN_MAX_SEGMENTS * 2
    assert at_bounds == recorded("lds_bytes_at_the_bounds") and at_bounds <= 64 * 1024


def test_op_and_record_tables_are_read_through_scalar_loads(isa):
    """the per-op and per-edge records sit at wave-uniform addresses: the cell loop reads them with s_load, and the only vector
    loads left are the candidate tests of the two compactions (a lane a candidate) and a cell's own height and mask"""
    body = re.search(r"^k_terrain_flatten:[^\n]*\n(.*?)s_endpgm", isa, flags=re.S | re.M).group(1)
    assert len(re.findall(r"^\s+s_load_dwordx4", body, flags=re.M)) >= 4
    assert len(re.findall(r"^\s+global_load", body, flags=re.M)) <= 6
