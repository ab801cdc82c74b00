"""Compiler-output checks for the kernels of the ranged ray refresh (no GPU needed: hipcc cross-compiles for gfx950).  Reads the kernel
descriptors' register, scratch and LDS metadata only, like tests/test_terrain_tiles_resources.py."""
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
    flags = [f for f in G.HIP_FLAGS if f not in ("-shared", "-fPIC")]
    text = ""
    for name in ("rxr_intersect", "rxr_ray_accel"):
        out = tmp_path_factory.mktemp("isa") / (name + ".s")
        subprocess.run([hipcc] + flags + ["--cuda-device-only", "-S", "-o", str(out), os.path.join(G.CSRC, name + ".hip")], check=True, stderr=subprocess.DEVNULL)
        text += open(out).read()
    return text


def descriptor(isa, name, key):
    m = re.search(rf"\.amdhsa_kernel (\w*{name}\w*)\n(.*?)\.end_amdhsa_kernel", isa, flags=re.S)
    assert m, name
    return int(re.search(rf"\.amdhsa_{key} (\d+)", m.group(2)).group(1))


def small_max():
    hdr = open(os.path.join(ROOT, "include", "rxr.h")).read()
    return int(re.search(r"#define RXR_RAY_REFIT_SMALL_MAX (\d+)u", hdr).group(1))


# All of them are short, latency-bound kernels -- a table look-up, a few gathers from the pools, a handful of stores -- launched over a
# stroke's worth of triangles or nodes: they want whole waves resident, not registers.  The bounds are the register blocks (of 8) that
# hold what the shipped build uses: k_isect_refresh 30, k_accel_refresh_records 38, k_accel_refit_leaves 35, k_accel_refit_level 22,
# k_accel_refit_small 37.  A build that needs a block more has changed what a kernel keeps live, and somebody should look.  None may
# spill: an AccelNode (eight floats) indexed in a way the compiler cannot resolve would live in the private segment.
@pytest.mark.parametrize("kernel,vgprs", [("k_isect_refresh", 32), ("k_accel_refresh_records", 40), ("k_accel_refit_leaves", 40),
                                          ("k_accel_refit_level", 24), ("k_accel_refit_small", 40)])
def test_no_scratch_and_the_shipped_register_block(isa, kernel, vgprs):
    assert descriptor(isa, kernel, "private_segment_fixed_size") == 0
    assert descriptor(isa, kernel, "next_free_vgpr") <= vgprs


# LDS of the one-launch route: the nodes this launch rewrote at the level below, 32 bytes each, at most RXR_RAY_REFIT_SMALL_MAX of them
# (a level's dirty nodes never outnumber the dirty leaves, and a level overwrites the one below in place) -- and nothing else; within
# the 64 KiB a workgroup may declare.
def test_the_small_route_keeps_one_level_of_dirty_nodes_in_lds(isa):
    assert descriptor(isa, "k_accel_refit_small", "group_segment_fixed_size") == 32 * small_max() <= 65536
    for kernel in ("k_isect_refresh", "k_accel_refresh_records", "k_accel_refit_leaves", "k_accel_refit_level"):
        assert descriptor(isa, kernel, "group_segment_fixed_size") == 0
