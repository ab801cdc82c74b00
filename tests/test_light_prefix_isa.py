"""Compiler-output checks for the prefix loop of the relaxed light loop (shade3d_lights<LV, true>, rusterix_amd/csrc/rxr_kernels.hip; no GPU
needed: hipcc cross-compiles for gfx950, about a minute and a half, once per module).  The loop exists to drop what the general loop pays
around a fast light's arithmetic, so the listing is held to that: tools/light_loop_isa.py finds the loop and, in the same listing, the
fast term's cycle through the general loop (the parent's code, unchanged) to compare it with.

Scratch: several kernels of the file have always had some (the program interpreters, the cut-out and pair kernels; the table of
profiles/light_prefix/README.md has the parent's figures), so "no scratch" is asked of the kernels the loop lives in without any, and
of every kernel that it has no more than the parent's."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import light_loop_isa as L  # noqa: E402

KERNELS = ["k_raster_rl", "k_raster_rows_rl"]


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    import __graft_entry__ as G

    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    flags = [f for f in G.HIP_FLAGS if f not in ("-shared", "-fPIC")]
    out = tmp_path_factory.mktemp("isa") / "rxr_kernels.s"
    subprocess.run([hipcc] + flags + ["--cuda-device-only", "-S", "-o", str(out), os.path.join(G.CSRC, "rxr_kernels.hip")], check=True, stderr=subprocess.DEVNULL)
    return open(out).read()


def recorded():
    """{kernel: (VGPRs parent, VGPRs branch, scratch parent, scratch branch, waves parent, waves branch)} of the README's table"""
    text = open(os.path.join(ROOT, "profiles", "light_prefix", "README.md")).read()
    rows = re.findall(r"^\| `(k_\w+)` \| (\d+) / (\d+) \| (\d+) / (\d+) \| \d+ / \d+ \| (\d+) / (\d+) \|", text, flags=re.M)
    return {k: tuple(int(x) for x in v) for k, *v in rows}


def descriptor(isa, name, key):
    m = re.search(rf"\.amdhsa_kernel {name}\n(.*?)\.end_amdhsa_kernel", isa, flags=re.S)
    assert m, name
    return int(re.search(rf"\.amdhsa_{key} (\d+)", m.group(1)).group(1))


@pytest.mark.parametrize("kernel", KERNELS)
def test_the_prefix_loop_pays_nothing_around_its_arithmetic(isa, kernel):
    body = L.prefix_loop(isa, kernel)
    assert body is not None, f"{kernel}: no loop of two v_rsq_f32 in front of the general loop"
    loop, parent = L.count(body), L.count(L.fast_block(isa, kernel))
    print(kernel, "prefix loop", loop, "general loop's fast cycle", parent)
    assert loop["v_mov_from_vgpr"] == 0, [t for t in body if t.startswith("v_mov_b32")]
    assert loop["lane_moves"] == 0, "an SGPR spill inside the loop"
    assert loop["saveexec"] == 0
    assert loop["scalar_loads"] == 1 and loop["scalar_loads_from_kernarg"] == 0, [t for t in body if t.startswith("s_load")]
    # the general loop's cycle is the parent's fast block (the count of the parent's own listing stands in the README: 47)
    assert parent["saveexec"] == 1 and parent["scalar_loads"] == 2 and parent["v_mov_from_vgpr"] == 3
    assert loop["valu"] <= parent["valu"], (loop["valu"], parent["valu"])
    text = open(os.path.join(ROOT, "profiles", "light_prefix", "README.md")).read()
    m = re.search(rf"^\| `{kernel}` \| (\d+) \| (\d+) \|", text, flags=re.M)
    assert m, "the README's table of the two loops"
    assert (parent["valu"], loop["valu"]) == (int(m.group(1)), int(m.group(2)))


def test_no_kernel_gains_scratch_and_the_loops_kernels_have_none(isa):
    table = recorded()
    kernels = re.findall(r"\.amdhsa_kernel (\w+)\n", isa)
    assert sorted(kernels) == sorted(table), set(kernels) ^ set(table)
    for k in kernels:
        vp, vb, sp, sb, wp, wb = table[k]
        assert descriptor(isa, k, "private_segment_fixed_size") == sb <= sp, k
        assert descriptor(isa, k, "next_free_vgpr") == vb, k
        assert wb >= wp, k
    for k in KERNELS:
        assert table[k][3] == 0 and table[k][1] <= 64 and table[k][5] == 8, k
