"""The material of tests/bake_fuzz.py without a GPU: what tests/test_gpu_bake_fuzz.py bakes is accepted by the device's validation,
fits the interpreter's limits, and is not vacuous -- judged on the oracle alone, over the very seeds and grids the GPU test uses."""
import collections
import os
import re

import numpy as np
import pytest

from rusterix_amd.binding import Program
from tests import bake_fuzz as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COVERED = F.UNARY + F.BINARY + ["Mix", "Smoothstep", "Clamp", "Pack2", "Pack3", "Dup", "Swap", "GetComponents", "SetComponents", "If", "For",
                                "FunctionCall", "Return", "Clear", "Sample", "SampleNormal", "LoadGlobal", "StoreGlobal", "PaletteIndex"]


def f32(x):
    return np.float32(x)


def test_limits_are_the_headers():
    dev = open(os.path.join(ROOT, "rusterix_amd", "csrc", "rxr_device.h")).read()
    vm = open(os.path.join(ROOT, "rusterix_amd", "csrc", "rxr_vm.h")).read()
    for name, value in (("RXR_VM_STACK", F.VM_STACK), ("RXR_VM_LOCALS", F.VM_LOCALS), ("RXR_VM_FRAMES", F.VM_FRAMES), ("RXR_VM_LOOPS", F.VM_LOOPS)):
        assert int(re.search(rf"#define {name} (\d+)", dev).group(1)) == value, name
    assert int(re.search(r"#define RXR_VM_LDS_STACK (\d+)", vm).group(1)) == F.VM_LDS_STACK


def test_every_seed_is_accepted_fits_the_limits_and_lands_in_its_class():
    classes = collections.Counter()
    deep = 0
    for cls in ("static", "dynamic"):
        for seeds in F.groups(cls):
            rc, each, said = F.check_set([F.generate(s)[0] for s in seeds])
            assert rc == 0 and not any(each), (seeds, [m for m in said if m][:2])
            for s in seeds:
                prog, gen = F.generate(s)
                names = set().union(*(F.op_names(f) for f in gen.raw))
                dynamic = bool(names & {"FunctionCall", "PaletteIndex"})
                assert dynamic == (cls == "dynamic"), (s, cls)
                classes[cls] += 1
                assert not names & {"Sin", "Sin1", "Sin2", "Cos", "Cos1", "Cos2", "Tan", "Atan", "Log", "Atan2", "Pow", "Rotate2D"}, s
                assert not names & {"SetMetallic", "SetBump", "SetUV", "SetOpacity", "SetEmissive"}, s
                assert "SetRoughness" in names or "Roughness" not in names, s     # (read only by the program that wrote it first)
                hw = F.high_water(gen.raw, gen.shade_locals)
                assert hw["stack"] <= F.VM_STACK and hw["locals"] <= F.VM_LOCALS and hw["frames"] <= F.VM_FRAMES and hw["loops"] <= F.VM_LOOPS, (s, hw)
                deep += hw["stack"] > F.VM_LDS_STACK
    n = len(F.SEEDS)
    assert n == 200 and classes["static"] >= n // 4 and classes["dynamic"] >= n // 4, classes
    assert deep >= 20, f"{deep} programs reach past the LDS part of the stack"
    print(f"classes {dict(classes)}; {deep} programs with a stack of 3 or more")


def test_the_generator_is_deterministic():
    a = F.BakeProgramGen(np.random.default_rng([0x52585231, 5150, 7]), F.class_of(7))
    a.program()
    assert a.raw == F.generate(7)[1].raw


def test_vacuity_and_opcode_coverage(oracle):
    """at most 15 % of the seeds give an image that is mostly non-finite or nearly constant; every opcode the GPU test is meant to
    check appears in at least five programs"""
    vacuous, seen = [], collections.Counter()
    for cls in ("static", "dynamic"):
        for seeds in F.groups(cls):
            for s, px in zip(seeds, F.group_reference(oracle, seeds)):    # (the reference asserts that it did not fault)
                assert (px[..., 3] == 1.0).all()
                if F.vacuous(px):
                    vacuous.append(s)
                seen.update(set().union(*(F.op_names(f) for f in F.generate(s)[1].raw)))
    print(f"vacuous: {len(vacuous)} of {len(F.SEEDS)} seeds {sorted(vacuous)}")
    assert len(vacuous) <= 0.15 * len(F.SEEDS), sorted(vacuous)
    rare = {op: seen[op] for op in COVERED if seen[op] < 5}
    assert not rare, rare
    print("programs per opcode: " + ", ".join(f"{op} {seen[op]}" for op in COVERED))


def test_lanes_of_one_wave_part_in_a_third_of_the_programs(oracle):
    """a top-level If of `shade` whose condition -- evaluated by the oracle on the program cut off at the If -- takes both values
    within 64 consecutive texels.  (Ifs in nested blocks and in callees, and the per-texel trip counts, come on top: not counted.)"""
    diverging = 0
    for s in F.SEEDS:
        gen = F.generate(s)[1]
        probes = [Program([p] + gen.raw[1:], shade_locals=gen.shade_locals, globals=gen.n_globals) for p in F.branch_probes(gen.raw)]
        if probes:
            ref = F.Reference(oracle, probes)
            diverging += any(F.diverges(ref.pixels(i, *F.SIZE)[..., 0]) for i in range(len(probes)))
    print(f"wave divergence at a top-level If: {diverging} of {len(F.SEEDS)} programs")
    assert diverging >= 0.3 * len(F.SEEDS)


@pytest.mark.parametrize("source", ["palette", "computed"])
def test_opcode_grids_are_accepted_and_not_vacuous(oracle, source):
    progs = F.grid_programs(source)
    rc, each, said = F.check_set(list(progs.values()))
    assert rc == 0 and not any(each), [m for m in said if m][:2]
    assert set(F.UNARY + F.BINARY + F.TERNARY) <= set(progs)
    for op, px in F.grid_reference(oracle, source).items():
        c = px[..., :3]
        finite = np.isfinite(c)
        distinct = len(np.unique(F.bits(c[finite])))
        assert finite.mean() >= 0.6, (op, float(finite.mean()))
        assert op in F.COMPARISONS or distinct >= 32, (op, distinct)
    print("; ".join(f"{op} {int(np.isfinite(px[..., :3]).sum())}" for op, px in F.grid_reference(oracle, source).items()))


def test_the_operand_table():
    t = F.TABLE
    assert len(t) == 64 and np.array_equal(F.bits(t[:16]), F.bits(np.array(F.SPECIALS, np.float32)))
    rest = t[16:]
    assert np.isfinite(rest).all() and (rest > 0).any() and (rest < 0).any()
    assert ((np.abs(rest) < 1.1754944e-38) & (rest != 0)).sum() == 2                           # two denormals
    assert ((F.bits(rest) & 0xFF) != 0).mean() > 0.9                                            # full mantissas
    assert len(np.unique(np.frexp(rest)[1])) >= 8
    # the operands the failure messages name are the operands the programs read
    a, b, c = F.grid_operands("palette", 0, 5)
    assert np.array_equal(F.bits(a), F.bits(np.array(F.GRID_PALETTE[5], np.float32))) and np.array_equal(F.bits(b), F.bits(np.array(F.GRID_PALETTE[0], np.float32)))
    a, b, c = F.grid_operands("palette", 3, 7)
    assert np.array_equal(F.bits(b), F.bits(np.array(F.GRID_PALETTE[61], np.float32))) and np.array_equal(F.bits(c), F.bits(np.array(F.GRID_PALETTE[4], np.float32)))


def test_reference_on_hand_computed_grid_cells(oracle):
    """a wrong oracle would move both sides of the GPU comparison: cells of the grids worked out here, in numpy float32 in the
    reference's operation order (rusteria/src/node/execution.rs), or by hand"""
    for source in ("palette", "computed"):
        ref = F.grid_reference(oracle, source)
        for (y, x) in [(0, 0), (5, 17), (40, 33), (63, 62), (17, 49), (22, 21)]:
            a, b, c = F.grid_operands(source, y, x)
            if not (np.isfinite(a).all() and np.isfinite(b).all() and np.isfinite(c).all()):
                continue
            with np.errstate(all="ignore"):
                want = {
                    "Add": a + b, "Sub": a - b, "Mul": a * b, "Div": a / b, "Neg": -a, "Abs": np.abs(a),
                    "Dot3": np.array([f32(f32(a[0] * b[0]) + f32(a[1] * b[1])) + f32(a[2] * b[2]), 0, 0], np.float32),
                    "Dot2": np.array([f32(a[0] * b[0]) + f32(a[1] * b[1]), 0, 0], np.float32),
                    "Cross": np.array([f32(a[1] * b[2]) - f32(a[2] * b[1]), f32(a[2] * b[0]) - f32(a[0] * b[2]), f32(a[0] * b[1]) - f32(a[1] * b[0])], np.float32),
                    "Length": np.full(3, np.sqrt(f32(f32(a[0] * a[0]) + f32(a[1] * a[1])) + f32(a[2] * a[2]), dtype=np.float32), np.float32),
                    "Mix": a + (b - a) * c, "Sqrt": np.sqrt(a), "Floor": np.floor(a), "Fract": a - np.floor(a),
                    "Mod": a - b * np.floor(a / b),
                }
            for op, w in want.items():
                w = np.asarray(w, np.float32) + f32(0.0)
                got = ref[op][y, x, :3]
                assert not F.differing(got, w).any(), (source, op, y, x, a.tolist(), b.tolist(), got.tolist(), w.tolist())
    # special operands, by hand: the palette's slots 0..15 are the SPECIALS (slot i: special i, i + 5, i + 11 -- x looks at special i)
    ref = F.grid_reference(oracle, "palette")
    cell = lambda op, ia, ib: ref[op][(F.GRID - ib) % F.GRID, ia, 0]   # noqa: E731  (operand a: SPECIALS[ia], operand b: SPECIALS[ib])
    sp = F.SPECIALS
    assert (sp[0], sp[1], sp[5], sp[15], sp[4]) == (0.0, -0.0, -2.5, 2.0, 0.5) and np.signbit(sp[1])
    # Max(+0, -0) and Max(-0, +0): f32::max as compiled returns the FIRST of operands that compare equal; the float buffer adds +0.0
    # (accum_from), which hides the sign -- 1 / x of it is covered by tests/test_gpu_shader_edge_values.py; here the values
    assert cell("Max", 0, 1) == 0.0 and cell("Min", 1, 0) == 0.0
    assert cell("Max", 8, 5) == -2.5 and cell("Min", 5, 8) == -2.5            # a NaN operand is dropped
    assert cell("Mod", 5, 15) == 1.5                                          # -2.5 - 2 * floor(-1.25) = 1.5
    assert cell("Round", 5, 0) == -3.0 and cell("Floor", 5, 0) == -3.0 and cell("Ceil", 5, 0) == -2.0    # half away from zero
    assert cell("Round", 4, 0) == 1.0                                         # Round(0.5) = 1, not the even 0
    assert np.isnan(cell("Sqrt", 3, 0)) and np.isposinf(cell("Div", 2, 0)) and np.isneginf(cell("Div", 2, 1)) and np.isnan(cell("Div", 0, 0))
    assert cell("Step", 8, 2) == 0.0 and cell("Eq", 8, 8) == 0.0 and cell("Ne", 8, 8) == 1.0      # comparisons with NaN
    assert cell("Sub", 6, 6) != cell("Sub", 6, 6) and cell("Mul", 6, 0) != cell("Mul", 6, 0)      # inf - inf, inf * 0


def test_round_of_two_and_a_half(oracle):
    """Round(2.5) = 3 (f32::round: half away from zero; rintf would give 2) and Round(-2.5) = -3, through a program of their own"""
    ref = F.Reference(oracle, [Program([[("Push", 2.5, -2.5, 0.5), "Round", "SetColor"]])])
    assert ref.pixels(0, 1, 1)[0, 0].tolist() == [3.0, -3.0, 1.0, 1.0]


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, F.VM_STACK - 1, F.VM_STACK, F.VM_STACK + 1])
def test_depth_programs_peak_where_they_say(oracle, n):
    raw = F.depth_program(n)
    assert F.high_water(raw, 0)["stack"] == n
    rc, each, said = F.check_set([Program(raw)])
    assert rc == 0 and each == [0], said        # (the overflowing one is a valid program too: the fault is found at run time)
    px = F.Reference(oracle, [Program(raw)]).pixels(0, *F.SIZE)
    assert not F.vacuous(px)
    cond = F.Reference(oracle, [Program([p]) for p in F.branch_probes(raw)]).pixels(0, *F.SIZE)[..., 0]
    assert F.diverges(cond)
