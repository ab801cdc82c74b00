"""Compiler-output checks for the wave walk of the ray box tree (k_accel_by_wave; no GPU needed: hipcc cross-compiles for gfx950).  Reads
the kernel descriptors' register, scratch and LDS metadata only, like tests/test_ray_refresh_resources.py, and holds them to the table
of profiles/ray_wave/README.md."""
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
    out = tmp_path_factory.mktemp("isa") / "rxr_ray_accel.s"
    subprocess.run([hipcc] + flags + ["--cuda-device-only", "-S", "-o", str(out), os.path.join(G.CSRC, "rxr_ray_accel.hip")], check=True, stderr=subprocess.DEVNULL)
    return open(out).read()


def descriptor(isa, name, key):
    m = re.search(rf"\.amdhsa_kernel (\w*{name}\w*)\n(.*?)\.end_amdhsa_kernel", isa, flags=re.S)
    assert m, name
    return int(re.search(rf"\.amdhsa_{key} (\d+)", m.group(2)).group(1))


def recorded():
    """{kernel: (VGPRs, SGPRs, LDS bytes, scratch bytes)} of the README's resource table"""
    text = open(os.path.join(ROOT, "profiles", "ray_wave", "README.md")).read()
    rows = re.findall(r"^\| `(k_accel_by_\w+<\w+>)` \| (\d+) \| (\d+) \| (\d+) \| (\d+) \|", text, flags=re.M)
    return {k: tuple(int(x) for x in v) for k, *v in rows}


INSTANCES = {"k_accel_by_wave<false>": "k_accel_by_waveILb0E", "k_accel_by_wave<true>": "k_accel_by_waveILb1E",
             "k_accel_by_ray<false>": "k_accel_by_rayILb0E", "k_accel_by_ray<true>": "k_accel_by_rayILb1E"}


# Four waves of a workgroup walk four rays and never meet; what bounds a small batch is the chain of dependent loads of each wave, so
# the kernel wants every wave it has resident: no scratch (the masks' stack is in LDS because a dynamically indexed register array
# would live in the private segment), and registers within the 64 that still allow eight waves a SIMD.
@pytest.mark.parametrize("kernel", ["k_accel_by_wave<false>", "k_accel_by_wave<true>"])
def test_no_scratch_and_the_recorded_registers_and_lds(isa, kernel):
    vgprs, sgprs, lds, scratch = recorded()[kernel]
    name = INSTANCES[kernel]
    assert descriptor(isa, name, "private_segment_fixed_size") == 0 == scratch
    assert descriptor(isa, name, "next_free_vgpr") == vgprs <= 64
    assert descriptor(isa, name, "next_free_sgpr") == sgprs
    # the level table (24 x 8 bytes, as k_accel_by_ray's) and four waves x 12 masks x 8 bytes
    assert descriptor(isa, name, "group_segment_fixed_size") == lds == 24 * 8 + 4 * 12 * 8


# the thread walk is the parent's: the registers its two instantiations had before this kernel was added next to them
@pytest.mark.parametrize("kernel,vgprs,sgprs", [("k_accel_by_ray<false>", 46, 46), ("k_accel_by_ray<true>", 48, 50)])
def test_the_thread_walk_is_unchanged(isa, kernel, vgprs, sgprs):
    name = INSTANCES[kernel]
    assert descriptor(isa, name, "private_segment_fixed_size") == 0
    assert (descriptor(isa, name, "next_free_vgpr"), descriptor(isa, name, "next_free_sgpr")) == (vgprs, sgprs)
    assert descriptor(isa, name, "group_segment_fixed_size") == 24 * 8
    assert recorded()[kernel][:2] == (vgprs, sgprs)
