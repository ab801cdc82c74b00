"""The material of tests/jit_floats.py without a GPU, on the oracle alone: the windows hide nothing (every pair of neighbouring floats
of the shown range gets different bytes in some window), what tests/test_gpu_jit_floats.py renders is mostly shown by them, every set is
accepted by the device's validation and by the run-time compiler's generator, and every operation the GPU test is meant to check occurs."""
import collections

import numpy as np

from tests import bake_fuzz as F
from tests import jit_floats as J
from tests.test_shader_jit_cpu import generate

PW, PH = 256, 208                 # the pair pattern: 53 248 texels, one pair each
PER_VALUE = 26                    # partners of a value: its two neighbours, its 23 mantissa bits flipped one at a time, its negative


def bits_of(x):
    return int(np.array([x], np.float32).view(np.uint32)[0])


def shown_values():
    """2 048 floats over every exponent of the shown range (2^-11 .. 2^6) and both signs: full random mantissas, and at the front
    the exact powers of two and the largest mantissa of every exponent whose neighbours stay inside the range"""
    rng = np.random.default_rng([0x52585231, 5161])
    n = PW * PH // PER_VALUE
    exps = list(range(-11, 7))
    bits = np.empty(n, np.uint32)
    for i in range(n):
        e, negative = exps[i % len(exps)], (i // len(exps)) % 2
        m = int(rng.integers(1, 1 << 23))
        if i < 2 * len(exps) and e > exps[0]:
            m = 0                                   # 2^e: the neighbour below has the exponent e - 1
        elif i < 4 * len(exps) and e < exps[-1]:
            m = (1 << 23) - 1                       # the neighbour above is 2^(e + 1)
        bits[i] = ((e + 127) << 23) | m | (negative << 31)
    return bits.view(np.float32)


def pair_pattern():
    a = shown_values()
    partners = [np.nextafter(a, np.float32(np.inf)), np.nextafter(a, np.float32(-np.inf))]
    partners += [(a.view(np.uint32) ^ np.uint32(1 << j)).view(np.float32) for j in range(23)] + [-a]
    assert len(partners) == PER_VALUE
    p = np.zeros((PH * PW, 3), np.float32)
    p[:, 0] = np.repeat(a, PER_VALUE)
    p[:, 1] = np.stack(partners, axis=1).reshape(-1)
    return p.reshape(PH, PW, 3)


def index_pattern():
    """(x, y) of the texel as bytes: tests/test_gpu_libm_ulp.py's way of learning which pixel shows which texel"""
    p = np.zeros((PH, PW, 3), np.float32)
    p[..., 0] = (np.arange(PW, dtype=np.float32) / np.float32(255.0))[None, :]
    p[..., 1] = (np.arange(PH, dtype=np.float32) / np.float32(255.0))[:, None]
    p[..., 2] = 1.0
    return p


def test_the_windows_hide_nothing(oracle):
    """two floats that differ -- by one ulp, in any one mantissa bit, or in their sign -- get different bytes in at least one window,
    over the whole shown range: the proof of jit_floats.WINDOWS.  If a pair collides the window set is wrong, not this test."""
    pairs = pair_pattern()
    a, b = pairs[..., 0], pairs[..., 1]
    assert J.fully_shown(a).all() and J.fully_shown(b).all() and (F.bits(a) != F.bits(b)).all()
    assert len(np.unique(np.frexp(a)[1])) == 18 and (a > 0).any() and (a < 0).any()
    fetch = lambda pattern: ["UV", ("Push", 4.0), "Mul", ("Push", float(pattern)), "Sample"]   # noqa: E731  (uv / 4 reaches a 2D program)
    programs = [J.P([fetch(0) + J.TAIL]), J.P([fetch(1) + ["SetColor"]])]
    assets_of = lambda api: api.Assets.default().patterns([pairs, index_pattern()])   # noqa: E731
    shown = J.Frame(oracle, programs, (PW, PH), 2, assets_of).windows()
    index = J.Frame(oracle, [programs[1]] * 2, (PW, PH), 2, assets_of).at(1.0)
    assert (index[..., 2] == 255).all() and np.array_equal(index[:, PW:], shown[0][:, PW:])
    for half in (index[:, :PW], index[:, PW:]):                  # every texel is drawn by some pixel, in either rectangle
        seen = np.zeros((PH, PW), bool)
        seen[half[..., 1].astype(np.int64), half[..., 0].astype(np.int64)] = True
        assert seen.all(), f"{int((~seen).sum())} texels are drawn by no pixel"
    texel = index[:, :PW, :2].astype(np.int64)                   # which texel each pixel of the left rectangle samples
    left = shown[:, :, :PW, :]
    differs = (left[..., 0] != left[..., 1]).any(axis=0)         # [PH][PW] per PIXEL: some window tells a from b
    colliding = np.argwhere(~differs)
    said = [(float(a[ty, tx]), float(b[ty, tx]), left[:, y, x, :2].tolist()) for y, x in colliding[:3] for tx, ty in [texel[y, x]]]
    assert not len(colliding), f"{len(colliding)} pairs get the same bytes in every window; first (a, b, bytes per window): {said}"
    telling = (left[..., 0] != left[..., 1]).sum(axis=0)
    print(f"\n{PW * PH} pairs over {len(shown_values())} values, windows {J.WINDOWS}: 0 collide; windows that tell a pair apart: "
          f"min {int(telling.min())}, mean {float(telling.mean()):.2f}")


def test_the_random_programs_are_mostly_shown(oracle):
    """at least 85 % of all channel-pixels of the 96 programs' oracle frames are fully shown (zero, or finite with every bit inside
    the windows), no set of 16 below 70 %, no seed in use below 25 % -- and the seeds that were replaced are below it"""
    shares, groups = {}, collections.defaultdict(list)
    for fs in J.random_sets():
        assert len(fs.seeds) == J.PART[fs.group.split("-")[0]] and all(F.class_of(s) == fs.group.split("-")[0] for s in fs.seeds)
        got = J.shown_share(oracle, fs.seeds)         # (the layout of the frame the GPU test renders)
        shares.update(zip(fs.seeds, got))
        groups[fs.group] += got
    per_set = [float(np.mean(v)) for v in groups.values()]
    assert all(len(v) == J.GROUP for v in groups.values())
    assert len(shares) == J.N_SEEDS == 96 and len(per_set) == 6
    total = float(np.mean(list(shares.values())))
    print(f"\nfully shown: {100 * total:.2f} % of all channel-pixels; per set {[round(100 * s, 2) for s in per_set]}; "
          f"programs that show nothing: {sorted(s for s, v in shares.items() if v == 0)}")
    assert total >= 0.85 and min(per_set) >= 0.70, (total, per_set)
    low = {s: v for s, v in shares.items() if v < 0.25}
    assert not low, f"seeds to replace: {low}"
    # the list of replacements follows its rule: every replaced seed is below 25 %, and takes the next unused seed of its class
    unused = {"static": J.N_SEEDS, "dynamic": J.N_SEEDS + 1}
    replaced = collections.OrderedDict()
    for cls in ("static", "dynamic"):
        old = [s for s in range(J.N_SEEDS) if F.class_of(s) == cls]
        for i in range(0, len(old), J.GROUP):
            for s, share in zip(old[i:i + J.GROUP], J.shown_share(oracle, old[i:i + J.GROUP])):
                while share < 0.25:
                    new, unused[cls] = unused[cls], unused[cls] + 2
                    replaced.setdefault(s, []).append((new, round(share, 3)))
                    s, share = new, J.shown_share(oracle, [new])[0]
    print("replaced seeds (seed: [(replacement, the share that was too low)]): " + str(dict(replaced)))
    chain = {}
    for s, steps in replaced.items():
        for new, _ in steps:
            chain[s], s = new, new
    assert chain == J.REPLACED, (chain, J.REPLACED)


def test_every_set_is_accepted_and_every_operation_occurs():
    """rxr_check_shaders and rxr_check_bake accept every set, the run-time compiler's generator covers it (rxr_debug_jit_generate:
    no GPU needed), and the operations the GPU test is meant to check are all there"""
    seen = collections.Counter()
    fused = set()
    sets = J.all_sets()
    names = [fs.name for fs in sets]
    assert len(set(names)) == len(names) == 12 + 24 + 9 + 1 and names[-1] == "control-flow", names
    for fs in sets:
        rc, each, said = F.check_set(fs.programs)
        assert rc == 0 and not any(each), (fs.name, [m for m in said if m][:2])
        rc, src, msg = generate(fs.programs, 0)
        assert rc == 0 and f"rxr_jit_prog_{len(fs.programs) - 1}" in src, (fs.name, msg)
        w, h = fs.cols * fs.cell[0], -(-len(fs.programs) // fs.cols) * fs.cell[1]
        assert w * h <= 640 * 400, (fs.name, w, h)
        for prog in fs.programs:
            for f in prog.raw:
                seen.update(F.op_names(f))
            flat = prog.raw[0]
            for a, b in zip(flat, flat[1:]):
                if not isinstance(a, str) and a[0] == "Push" and len(a) == 2 and isinstance(b, str) and b in F.FUSABLE:
                    fused.add((b, bits_of(a[1])))
    wanted = F.UNARY + F.BINARY + ["Mix", "Smoothstep", "Clamp", "Pack2", "Pack3", "GetComponents", "SetComponents", "SetNormal", "Normal", "Sample",
                                   "SampleNormal", "PaletteIndex", "If", "For", "Return", "FunctionCall", "Dup", "Swap", "LoadGlobal", "StoreGlobal"]
    missing = [op for op in wanted if not seen[op]]
    assert not missing, missing
    assert not set(seen) & J.LIBM
    missing = [(op, c) for op in J.BINC_OPS for c in J.BINC_CONSTANTS if (op, bits_of(c)) not in fused]
    assert not missing, missing                       # (0.0 and -0.0 are told apart by their bits; 1e-40 is a denormal)
    entries = [e for es in J.grid_entries().values() for e in es]
    assert len([e for e in entries if e.label.startswith("Push")]) == 13 * 5
    assert {tuple(sw) for sw in J.SWIZZLES} >= {(0,), (2, 0), (1, 2, 0), (1, 1)}
    assert all(e.twin for e in entries if e.label.startswith("Push") or e.label in ("Mix", "Smoothstep", "Clamp"))
    # the stack depths: what the compiler accepts is in the set, the first it refuses is not
    assert J.DEPTHS == [1, 2, 3, 4, 5, F.VM_STACK - 1] and J.REFUSED_DEPTH == F.VM_STACK
    rc, _, msg = generate([J.P([J.with_tail(F.depth_program(J.REFUSED_DEPTH)[0])])], 0)
    assert rc != 0 and "stack" in msg, msg


def test_the_generator_is_deterministic_and_no_value_reads_the_window_factor():
    a = J.FrameProgramGen(np.random.default_rng([0x52585231, 5160, 7]), F.class_of(7))
    a.program()
    assert a.raw == J.generate(7)[1].raw
    assert sorted(J.seeds_in_use()) == sorted(set(J.seeds_in_use())) and len(J.seeds_in_use()) == 96
    for s in J.seeds_in_use():
        gen = J.generate(s)[1]
        names = J.value_ops(gen.raw)
        assert "Time" not in names and not names & J.LIBM, s
        assert bool(names & {"FunctionCall", "PaletteIndex"}) == (gen.cls == "dynamic"), s
    for fs in J.all_sets():
        for i, prog in enumerate(fs.programs):
            assert sum(J.time_reads_outside_tails(f) for f in prog.raw) == 0, (fs.name, i)
            twin = hasattr(fs, "slots") and fs.slots[i][1]          # (a class twin ends in its flags and is drawn at one time)
            assert (str(J.TAIL)[1:-1] in str(prog.raw[0])) != twin, (fs.name, i)


def test_which_pixel_of_a_grid_cell_reads_which_operands(oracle):
    """a cell of the opcode grids has one pixel centre per operand pair: column x reads slot x as operand a, row y slot y as b -- what
    the failure messages of the GPU test say (jit_floats.grid_operands)"""
    frame = J.Frame(oracle, [J.slot_probe()] * 3, J.GRID_CELL, 2, J.grid_assets).at(1.0)
    for k in range(3):
        cell = frame[(k // 2) * J.N:(k // 2 + 1) * J.N, (k % 2) * J.N:(k % 2 + 1) * J.N]
        assert np.array_equal(cell[..., 0], np.broadcast_to(np.arange(J.N)[None, :], (J.N, J.N))), k
        assert np.array_equal(cell[..., 1], np.broadcast_to(np.arange(J.N)[:, None], (J.N, J.N))), k
    a, b, c = J.grid_operands(J.GridEntry("Mix", 3, ["Mix"]), 3, 62)
    assert np.array_equal(F.bits(a), F.bits(np.array(F.GRID_PALETTE[62], np.float32))) and np.array_equal(F.bits(c), F.bits(np.array(F.GRID_PALETTE[1], np.float32)))


def test_the_class_twins_tell_what_the_windows_cannot(oracle):
    """-0.0 against +0.0 and NaN against an infinity: the same bytes in every window, different class flags"""
    values = [0.0, -0.0, float("nan"), float("inf"), float("-inf"), 3.0]
    progs = [J.P([[("Push", v)] + J.TAIL]) for v in values] + [J.P([[("Push", v), ("StoreLocal", 0)] + J.class_flags(0)], shade_locals=1) for v in values]
    shown = J.Frame(oracle, progs, (4, 4), len(values), J.fuzz_assets).windows()
    bytes_of = lambda i, row: shown[:, row * 4 + 1, i * 4 + 1, :3].tolist()   # noqa: E731
    assert bytes_of(0, 0) == bytes_of(1, 0) == bytes_of(2, 0) == bytes_of(3, 0) == bytes_of(4, 0) != bytes_of(5, 0)
    flags = [tuple(shown[0, 5, i * 4 + 1, :3].tolist()) for i in range(len(values))]
    assert len(set(flags)) == len(values), flags
    assert all((shown[k, 4:] == shown[0, 4:]).all() for k in range(len(J.WINDOWS)))      # (a twin does not read Time)
