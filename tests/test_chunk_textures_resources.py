"""Compiler-output checks for k_chunk_tex_commit of rxr_chunk_tex.hip (no GPU needed: hipcc cross-compiles for gfx950): a streaming copy
whose loads want the occupancy -- no scratch, no LDS, and few enough registers for eight waves a SIMD.  Reads the kernel descriptor's
register and scratch metadata only, like tests/test_mesh_update_resources.py.

The compiled kernel takes 47 VGPRs (sixteen dwords in flight per lane in the 4-byte path, four 16-byte values in the other, their
addresses and the alpha fold); the ceiling is that plus a margin of 9 for compiler versions: 56, still below the 64 of eight waves."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VGPR_COMPILED, VGPR_CEILING = 47, 56


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    import __graft_entry__ as G

    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out = tmp_path_factory.mktemp("isa") / "rxr_chunk_tex.s"
    flags = [f for f in G.HIP_FLAGS if f not in ("-shared", "-fPIC")]
    subprocess.run([hipcc] + flags + ["--cuda-device-only", "-S", "-o", str(out), os.path.join(G.CSRC, "rxr_chunk_tex.hip")],
                   check=True, stderr=subprocess.DEVNULL)
    return open(out).read()


def descriptor(isa, name, key):
    m = re.search(rf"\.amdhsa_kernel {name}\n(.*?)\.end_amdhsa_kernel", isa, flags=re.S)
    assert m, f"{name} is not in rxr_chunk_tex.hip"
    return int(re.search(rf"\.amdhsa_{key} (\d+)", m.group(1)).group(1))


def test_the_commit_kernel_uses_no_scratch_no_lds_and_few_registers(isa):
    assert descriptor(isa, "k_chunk_tex_commit", "private_segment_fixed_size") == 0
    assert descriptor(isa, "k_chunk_tex_commit", "group_segment_fixed_size") == 0
    vgprs = descriptor(isa, "k_chunk_tex_commit", "next_free_vgpr")
    print(f"k_chunk_tex_commit: {vgprs} VGPRs (compiled: {VGPR_COMPILED}, ceiling {VGPR_CEILING})")
    assert vgprs <= VGPR_CEILING


def test_the_body_moves_sixteen_bytes_per_lane(isa):
    m = re.search(r"\.globl\s+k_chunk_tex_commit.*?\.end_amdhsa_kernel", isa, flags=re.S)
    assert m
    body = m.group(0)
    assert len(re.findall(r"global_load_dwordx4", body)) >= 4 and len(re.findall(r"global_store_dwordx4", body)) >= 4


def test_the_source_is_part_of_the_build():
    import __graft_entry__ as G
    import inspect

    assert "rxr_chunk_tex.hip" in inspect.getsource(G.build)
