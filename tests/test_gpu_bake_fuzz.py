"""The device interpreter (rxr_vm.h) against the oracle FLOAT FOR FLOAT, through the one place where its results leave the device as
floats: the `pixels` buffer of rxr_bake_shaders.  Every exact opcode over grids of operand pairs (special values from a palette,
full-mantissa values computed from uv), 200 random programs in two classes, directed stack depths around the LDS part of the value
stack and its bound -- each through k_bake (per-lane stack depths) and k_bake_s (static depths), with rxr_debug_last_bake_kernel
proving which of the two ran.  tests/test_bake_fuzz_cpu.py shows on the oracle alone that none of this is vacuous.

No tolerance appears here: where the oracle's channel is NaN the device's must be NaN, everywhere else the 32 bits must be equal."""
import ctypes as C

import numpy as np
import pytest

import rusterix_amd
from rusterix_amd import binding as B
from rusterix_amd.binding import Program
from tests import bake_fuzz as F
from tests import bake_ref as R

pytestmark = pytest.mark.gpu

K_BAKE, K_BAKE_S = 1, 2     # rxr_debug_last_bake_kernel


def last_bake_kernel(product):
    return rusterix_amd.rxr_abi().rxr_debug_last_bake_kernel(C.c_void_p(product.lib.rxh_context()))


def scene_of(product, programs):
    """a fresh scene: its programs become the context's resident set at the first bake (under the RXR_VM_NO_STATIC of that moment)"""
    scene = product.Scene.empty()
    for p in programs:
        scene.add_program(p)
    return scene


def bake(product, programs, size, assets_of, order=None, rgba=False):
    scene = scene_of(product, programs)
    return scene.bake_shaders(list(range(len(programs))) if order is None else order, size[0], size[1], assets=assets_of(product), rgba=rgba)


# ---- every exact opcode on a grid of operands ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", ["palette", "computed"])
def test_opcode_grids_float_for_float(oracle, product, monkeypatch, source):
    monkeypatch.delenv("RXR_VM_NO_STATIC", raising=False)
    progs = F.grid_programs(source)
    want = F.grid_reference(oracle, source)
    got = bake(product, list(progs.values()), (F.GRID, F.GRID), F.grid_assets)["pixels"]
    assert last_bake_kernel(product) == (K_BAKE if source == "palette" else K_BAKE_S)
    runs = [("", got)]
    if source == "computed":
        monkeypatch.setenv("RXR_VM_NO_STATIC", "1")
        again = bake(product, list(progs.values()), (F.GRID, F.GRID), F.grid_assets)["pixels"]
        assert last_bake_kernel(product) == K_BAKE
        runs.append((" (RXR_VM_NO_STATIC)", again))
    failures = []
    for note, pixels in runs:
        for i, op in enumerate(progs):
            def describe(y, x):
                return "operands " + ", ".join(f"{n} = {v.tolist()} (0x{' 0x'.join(format(int(b), '08x') for b in F.bits(v))})"
                                               for n, v in zip("abc", F.grid_operands(source, y, x)[:F.arity(op) if op != "Clamp" else 3]))
            try:
                F.assert_same_floats(pixels[i], want[op], f"{op}, {source} grid{note}", describe)
            except AssertionError as e:
                failures.append(str(e))
    assert not failures, f"{len(failures)} opcode grids differ from the oracle:\n" + "\n".join(failures)
    if source == "computed":
        assert np.array_equal(F.bits(runs[0][1]), F.bits(runs[1][1])), "k_bake_s and k_bake differ"


# ---- random programs ---------------------------------------------------------------------------------------------------------------
def compare_group(pixels, seeds, want, note):
    failures = []
    for j, s in enumerate(seeds):
        try:
            F.assert_same_floats(pixels[j], want[j], f"seed {s} ({F.class_of(s)}){note}", lambda y, x: f"gen.raw = {F.generate(s)[1].raw}")
        except AssertionError as e:
            failures.append(str(e))
    return failures


@pytest.mark.parametrize("cls", ["static", "dynamic"])
def test_random_programs_float_for_float(oracle, product, monkeypatch, cls):
    monkeypatch.delenv("RXR_VM_NO_STATIC", raising=False)
    expect = K_BAKE_S if cls == "static" else K_BAKE
    failures, firsts = [], []
    groups = F.groups(cls)
    assert sum(len(g) for g in groups) == 100
    for seeds in groups:
        got = bake(product, [F.generate(s)[0] for s in seeds], F.SIZE, F.fuzz_assets)["pixels"]
        assert last_bake_kernel(product) == expect, seeds
        firsts.append(got)
        failures += compare_group(got, seeds, F.group_reference(oracle, seeds), "")
    seeds = groups[1]      # a width that is no multiple of anything, 315 texels
    got = bake(product, [F.generate(s)[0] for s in seeds], F.ODD_SIZE, F.fuzz_assets)["pixels"]
    failures += compare_group(got, seeds, F.group_reference(oracle, seeds, F.ODD_SIZE), f" at {F.ODD_SIZE}")
    if cls == "static":
        monkeypatch.setenv("RXR_VM_NO_STATIC", "1")
        for seeds, first in zip(groups, firsts):
            got = bake(product, [F.generate(s)[0] for s in seeds], F.SIZE, F.fuzz_assets)["pixels"]
            assert last_bake_kernel(product) == K_BAKE, seeds
            failures += compare_group(got, seeds, F.group_reference(oracle, seeds), " (RXR_VM_NO_STATIC)")
            assert np.array_equal(F.bits(got), F.bits(first)), f"k_bake_s and k_bake differ for a program of seeds {seeds}"
    assert not failures, f"{len(failures)} programs differ from the oracle:\n" + "\n".join(failures)


def test_rgba_of_random_programs(oracle, product, monkeypatch):
    monkeypatch.delenv("RXR_VM_NO_STATIC", raising=False)
    for cls in ("static", "dynamic"):
        seeds = F.groups(cls)[0]
        got = bake(product, [F.generate(s)[0] for s in seeds], F.SIZE, F.fuzz_assets, rgba=True)["rgba"]
        for j, s in enumerate(seeds):
            R.check_bytes(got[j], F.group_reference(oracle, seeds)[j], f"seed {s} ({cls})")


def test_the_same_floats_in_a_mixed_call(product, monkeypatch):
    """the `jobs` indirection and the per-workgroup program index: a shuffled order with repeats in one launch"""
    monkeypatch.delenv("RXR_VM_NO_STATIC", raising=False)
    seeds = F.groups("dynamic")[2]
    scene = scene_of(product, [F.generate(s)[0] for s in seeds])
    assets = F.fuzz_assets(product)
    w, h = F.SIZE
    rng = np.random.default_rng([0x52585231, 5152])
    order = [int(i) for i in rng.permutation(len(seeds))] + [int(i) for i in rng.integers(0, len(seeds), 8)]
    mixed = scene.bake_shaders(order, w, h, assets=assets, rgba=False)["pixels"]
    assert last_bake_kernel(product) == K_BAKE
    single = {i: scene.bake_shaders([i], w, h, assets=assets, rgba=False)["pixels"][0] for i in sorted(set(order))}
    for slot, i in enumerate(order):
        assert np.array_equal(F.bits(mixed[slot]), F.bits(single[i])), f"slot {slot} (program {i}, seed {seeds[i]}) differs from that program's own bake"


# ---- the value stack: two slots in LDS, the rest in scratch, RXR_VM_STACK in all ------------------------------------------------------
DEPTHS = [1, 2, 3, 4, 5, F.VM_STACK - 1, F.VM_STACK]


def test_stack_depths_around_the_lds_part_and_the_bound(oracle, product, monkeypatch):
    monkeypatch.delenv("RXR_VM_NO_STATIC", raising=False)
    progs = [Program(F.depth_program(n)) for n in DEPTHS]
    ref = F.Reference(oracle, progs)
    want = [ref.pixels(i, *F.SIZE) for i in range(len(progs))]
    failures = []
    for no_static, kernel in ((False, K_BAKE_S), (True, K_BAKE)):
        if no_static:
            monkeypatch.setenv("RXR_VM_NO_STATIC", "1")
        got = bake(product, progs, F.SIZE, F.fuzz_assets)["pixels"]
        assert last_bake_kernel(product) == kernel
        for i, n in enumerate(DEPTHS):
            try:
                F.assert_same_floats(got[i], want[i], f"stack depth {n}, kernel {kernel}")
            except AssertionError as e:
                failures.append(str(e))
    assert not failures, "\n".join(failures)
    # one entry too many: the documented fault, with its texel; the context bakes on
    monkeypatch.delenv("RXR_VM_NO_STATIC")
    scene = scene_of(product, [progs[1], Program(F.depth_program(F.VM_STACK + 1))])
    assets = F.fuzz_assets(product)
    w, h = F.SIZE
    with pytest.raises(B.RasterizeError) as e:
        scene.bake_shaders([0, 1], w, h, assets=assets)
    msg = str(e.value)
    assert e.value.code == B.RXR_ERR_INVALID and "stack overflow" in msg and "program 1" in msg and "texel (" in msg, msg
    x, y = (int(v) for v in msg.split("texel (")[1].split(")")[0].split(","))
    assert 0 <= x < w and 0 <= y < h, msg
    assert last_bake_kernel(product) == K_BAKE        # (a program that can overflow keeps its set on the checking interpreter)
    F.assert_same_floats(scene.bake_shaders([0], w, h, assets=assets)["pixels"][0], want[1], "the bake after the fault")
