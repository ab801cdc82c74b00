"""Material for comparing the device interpreter (rxr_vm.h, through the bake kernels k_bake / k_bake_s of rxr_bake.hip) with the oracle
FLOAT FOR FLOAT, shared by tests/test_bake_fuzz_cpu.py (no GPU: the material is not vacuous) and tests/test_gpu_bake_fuzz.py:

  * BakeProgramGen: tests/test_gpu_shaders.py's ProgramGen made bake-legal and extended, in two classes -- `static` (no calls, no
    PaletteIndex: tag_static_depths succeeds, the set runs k_bake_s) and `dynamic` (a call or a PaletteIndex: k_bake);
  * the opcode grids: one program per exact opcode over a 64 x 64 grid of operand pairs, the operands either read from a 64-slot
    palette (special values included; PaletteIndex: dynamic) or computed from uv (full-mantissa values; static);
  * directed programs whose value stack peaks at a given depth;
  * the comparison: NaN against NaN, every other value bit for bit.

No libm opcode appears anywhere here (tests/test_gpu_libm_ulp.py owns those), so no tolerance does either."""
import ctypes as C

import numpy as np

from rusterix_amd.binding import Program
from tests import bake_ref as R
from tests import test_gpu_shaders as S
from tests.test_gpu_shader_edge_values import SPECIALS

SEEDS = range(200)
GROUP = 16                  # programs per shader set (one bake call per set)
SIZE = (24, 16)             # 384 texels: one and a half workgroups, the last wave of the last workgroup half full
ODD_SIZE = (63, 5)
VM_STACK, VM_LOCALS, VM_FRAMES, VM_LOOPS, VM_LDS_STACK = 64, 48, 8, 8, 2   # rxr_device.h / rxr_vm.h (tests/test_bake_fuzz_cpu.py reads them back)

UNARY, BINARY, TERNARY = S.EXACT_UNARY, S.EXACT_BINARY, ["Mix", "Smoothstep"]
COMPARISONS = ["Not", "Step", "Eq", "Ne", "Lt", "Le", "Gt", "Ge", "And", "Or"]   # results are 0 or 1: exempt from the distinct-value count
FUSABLE = {"Add", "Sub", "Mul", "Div", "Min", "Max", "Mod", "Lt", "Le", "Gt", "Ge", "Eq", "Ne"}   # "Push c; op" is ONE instruction (VM_BINC)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def class_of(seed):
    return "static" if seed % 2 == 0 else "dynamic"


# ---- assets ------------------------------------------------------------------------------------------------------------------------
# the random programs' palette: every slot present (a guarded PaletteIndex always pushes), full-mantissa values
FUZZ_PALETTE = [tuple(float(x) for x in row) for row in
                np.random.default_rng([0x52585231, 5151]).uniform(-2.0, 2.0, (8, 3)).astype(np.float32)]
PATTERN_IDS = [0.0, 1.0, 2.0, 9.0]      # bake_ref.patterns() holds two: 2 and 9 are out of range (the result is zero)


def operand_table():
    """N = 64 operand floats: the 16 SPECIALS of tests/test_gpu_shader_edge_values.py, 46 full-mantissa normal values over ten
    exponents and both signs, and two denormals"""
    rng = np.random.default_rng([0x52585231, 6464])
    exps = [-20, 0, 1, 2, 3, 4, 5, 8, 12, 20]      # (mostly above 1: Floor, Ceil and Round keep them apart)
    out = list(SPECIALS)
    for i in range(46):
        m = np.float32(1.0) + np.float32(int(rng.integers(1, 1 << 23))) * np.float32(2.0 ** -23)
        sign = np.float32(-1.0 if i % 4 == 3 else 1.0)   # (one in four negative: Sqrt keeps a finite majority)
        out.append(float(sign * m * np.float32(2.0 ** exps[i % len(exps)])))
    for sign in (0, 0x80000000):
        out.append(float(np.array([int(rng.integers(1 << 10, 1 << 23)) | sign], np.uint32).view(np.float32)[0]))
    assert len(out) == 64
    return np.array(out, np.float32)


TABLE = operand_table()
N = len(TABLE)
GRID_PALETTE = [(float(TABLE[i]), float(TABLE[(i + 5) % N]), float(TABLE[(i + 11) % N])) for i in range(N)]


def fuzz_assets(api):
    pats = R.patterns()
    return api.Assets.default().patterns(pats).patterns(pats[::-1], normal=True).palette(FUZZ_PALETTE)


def grid_assets(api):
    return api.Assets.default().palette(GRID_PALETTE)


class Reference(R.Reference):
    """bake_ref.Reference with other assets"""

    def __init__(self, oracle, programs, assets_of=fuzz_assets):
        super().__init__(oracle, programs)
        self.assets = assets_of(oracle)


# ---- the random programs -----------------------------------------------------------------------------------------------------------
# uv is the only field that varies in a bake; the others hold their Execution::new constants (all zero: kept rare, they make results vacuous).
# `Roughness` is absent: rxr_set_shaders refuses a set in which one program reads it unwritten while another writes it.
SOURCES = ["UV"] * 9 + ["Color", "Time", "Metallic", "Hitpoint"]


class BakeProgramGen(S.ProgramGen):
    """ProgramGen for the bake: SetColor is the setter; SetNormal / SetRoughness only after an unconditional first write at the top of
    `shade` (then the field may be read: rxr_check_bake's rule), and the productions ProgramGen lacks.  Each is safe to compare bit
    for bit because the oracle computes it without rounding of its own:
      Pack2 / Pack3 / Dup / Swap  move values;
      LoadGlobal / StoreGlobal  move values; every global is written at the top of `shade` before anything can read it;
      Sample / SampleNormal     a lookup (patterns of multiples of 1/64; `* 2 - 1` is exact for them) at uv * k, finite; ids 2 and 9
                                name no pattern and give zero;
      PaletteIndex              (dynamic only) a lookup; the index is floor(uv * k) mod 8 and all eight slots exist, so it always pushes;
      If as a value, For with a per-texel trip count: control flow on a uv comparison, so that lanes of one wave part."""

    def __init__(self, rng, cls):
        n_functions = int(rng.integers(0, 3)) if cls == "dynamic" else 0
        super().__init__(rng, int(rng.integers(3, 6)), n_functions, setters=["SetColor"])
        self.cls = cls
        self.sources = list(SOURCES)
        self.n_globals = int(rng.integers(0, 3))
        self.globals_ready = 0
        self.extra_setters = [s for s in ("SetNormal", "SetRoughness") if rng.random() < 0.3]

    def uv_component(self):
        return ["UV", ("GetComponents", [int(self.rng.integers(0, 2))])]

    def uv_condition(self):
        """true for a part of every row (component 0) or of the rows (component 1)"""
        c = float(np.round(self.rng.uniform(0.2, 0.8), 2))
        return self.uv_component() + [("Push", c), str(self.rng.choice(["Lt", "Gt", "Le", "Ge"]))]

    def palette_value(self):
        return self.uv_component() + [("Push", float(self.rng.integers(2, 17))), "Mul", "Floor", ("Push", float(len(FUZZ_PALETTE))), "Mod", "PaletteIndex"]

    def value(self, depth):
        r = self.rng
        if depth < 4 and r.random() < 0.3:
            k = int(r.integers(0, 8))
            if k == 0:
                return self.value(depth + 1) + self.value(depth + 1) + ["Pack2"]
            if k == 7:   # (ProgramGen's own Pack3 production is never drawn)
                return self.value(depth + 1) + self.value(depth + 1) + self.value(depth + 1) + ["Pack3"]
            if k == 1:
                return self.value(depth + 1) + ["Dup", str(r.choice(S.BINARY))]
            if k == 2:
                return self.value(depth + 1) + self.value(depth + 1) + ["Swap", str(r.choice(S.BINARY))]
            if k == 3 and self.globals_ready:
                return [("LoadGlobal", int(r.integers(0, self.globals_ready)))]
            if k == 4:
                return ["UV", ("Push", float(r.integers(1, 9))), "Mul", ("Push", float(r.choice(PATTERN_IDS))), str(r.choice(["Sample", "SampleNormal"]))]
            if k == 5 and self.cls == "dynamic":
                return self.palette_value()
            if k == 6:
                return self.uv_condition() + [("If", self.value(depth + 1), self.value(depth + 1))]
            return ["UV", ("Push", float(np.round(r.uniform(0.5, 9.0), 3))), "Mul"]
        return super().value(depth)

    def statement(self, depth):
        r = self.rng
        if depth < 3 and r.random() < 0.3:
            k = int(r.integers(0, 3))
            if k == 0 and self.n_globals:
                return self.value(depth + 1) + [("StoreGlobal", int(r.integers(0, self.n_globals)))]
            if k == 1:
                els = self.block(depth + 1) if r.random() < 0.6 else None
                return self.uv_condition() + [("If", self.block(depth + 1), els)]
            i = self.n_locals + depth     # (the counter local ProgramGen's own For would take at this depth)
            trips = self.uv_component() + [("Push", float(r.integers(2, 6))), "Mul"]          # 0 .. 5 trips, by the texel
            return [("For", [("Push", 0.0), ("StoreLocal", i)], [("LoadLocal", i)] + trips + ["Lt"],
                     [("LoadLocal", i), ("Push", 1.0), "Add", ("StoreLocal", i)], self.block(depth + 1) + self.value(depth + 1))]
        return super().statement(depth)

    def program(self):
        r = self.rng
        shade = []
        self.first_callable = self.n_functions      # (no call before every global is written: a callee may read any of them)
        self.loadable = 0                           # (... and no local is written yet)
        for g in range(self.n_globals):
            shade += self.value(1) + [("StoreGlobal", g)]
            self.globals_ready = g + 1
        self.first_callable = 0
        for i in range(self.n_locals):
            self.loadable = i
            shade += self.value(1) + [("StoreLocal", i)]
        self.loadable = self.n_locals
        for s in self.extra_setters:       # the first write: unconditional, before any read of the field
            shade += ["UV", ("Push", 0.3, 0.6, 0.8), "Add", s] if s == "SetNormal" else self.value(1) + [s]
        shade_sources = self.sources + [s[3:] for s in self.extra_setters]
        function_sources = self.sources
        self.sources = shade_sources
        self.setters = ["SetColor"] + self.extra_setters
        shade += self.block(0) + self.block(0) + self.value(0) + self.value(0) + ["Add"]
        if self.cls == "dynamic":          # whatever the productions drew: a dynamic program has a PaletteIndex
            shade += self.palette_value() + [("Push", 0.125), "Mul", "Add"]
        shade += ["UV", ("Push", 3.7), "Mul", "Add"]
        if r.random() < 0.6:               # wrapped into [0, 1) -- or the raw value, sign and exponent included
            shade += ["Fract"]
        shade += ["SetColor"]
        functions = []
        shade_locals = self.n_locals
        self.sources = function_sources    # (a callee does not read what `shade` wrote: rxr_check_bake follows no call)
        self.setters = ["SetColor"]
        self.n_locals = self.loadable = 3
        for k in range(self.n_functions):
            self.first_callable = k + 1
            functions.append(self.function())
        self.raw = [shade] + functions     # kept printable for a failing seed
        self.shade_locals = shade_locals + 4
        return Program([shade] + functions, shade_locals=self.shade_locals, globals=self.n_globals)


_generated = {}


def generate(seed):
    """(Program, its generator) of a seed; the generator keeps raw (the op lists), cls, shade_locals, n_globals"""
    if seed not in _generated:
        gen = BakeProgramGen(np.random.default_rng([0x52585231, 5150, seed]), class_of(seed))
        _generated[seed] = (gen.program(), gen)
    return _generated[seed]


def groups(cls):
    """the seeds of a class, GROUP to a shader set"""
    seeds = [s for s in SEEDS if class_of(s) == cls]
    return [seeds[i:i + GROUP] for i in range(0, len(seeds), GROUP)]


# ---- counting what a generated program is made of ----------------------------------------------------------------------------------
def op_names(ops, out=None):
    """every opcode name in an op list, nested blocks included"""
    out = set() if out is None else out
    for op in ops:
        name = op if isinstance(op, str) else op[0]
        out.add(name)
        if name in ("If", "For"):
            for b in op[1:]:
                if b is not None:
                    op_names(b, out)
    return out


PUSH1 = {"UV", "Normal", "Hitpoint", "Time", "Color", "Roughness", "Metallic", "Emissive", "Opacity", "Bump", "LoadLocal", "LoadGlobal", "Push", "Dup"}
POP1 = {"StoreLocal", "StoreGlobal", "SetColor", "SetNormal", "SetRoughness", "SetMetallic", "SetBump", "SetUV", "SetOpacity", "SetEmissive", "Clear",
        "SetComponents", "Pack2", "Sample", "SampleNormal"} | set(BINARY)
POP2 = {"Pack3", "Mix", "Smoothstep", "Clamp"}
SAME = {"GetComponents", "Swap", "Return", "PaletteIndex"} | set(UNARY)     # (PaletteIndex: guarded, pops one and pushes one)


def high_water(raw, shade_locals):
    """the device's high-water marks of a program (raw: its functions' op lists, `shade` first), by walking the op lists as the
    flattened code runs them (a constant and a FUSABLE operation behind it are one instruction that pushes nothing):
    dict(stack, loops, frames, locals)"""
    top = dict(stack=0, loops=0, frames=0, locals=shade_locals)

    def walk(ops, d, loops, frames, locals_):
        i = 0
        while i < len(ops):
            op = ops[i]
            name = op if isinstance(op, str) else op[0]
            nxt = ops[i + 1] if i + 1 < len(ops) else None
            if name == "Push" and isinstance(nxt, str) and nxt in FUSABLE:
                i += 2
                continue
            if name == "If":
                d -= 1
                after = walk(op[1], d, loops, frames, locals_)
                if op[2] is not None:
                    assert walk(op[2], d, loops, frames, locals_) == after, "unbalanced If"
                d = after
            elif name == "For":
                top["loops"] = max(top["loops"], loops + 1)
                base = walk(op[1], d, loops + 1, frames, locals_)
                assert walk(op[2], base, loops + 1, frames, locals_) == base + 1
                assert walk(op[4], base, loops + 1, frames, locals_) >= base
                assert walk(op[3], base, loops + 1, frames, locals_) == base
                d = base
            elif name == "FunctionCall":
                arity, total, index = op[1:]
                d -= arity
                top["frames"] = max(top["frames"], frames + 1)
                top["locals"] = max(top["locals"], locals_ + total)
                walk(raw[index], d, loops, frames + 1, locals_ + total)
                d += 1
            elif name in PUSH1:
                d += 1
            elif name in POP1:
                d -= 1
            elif name in POP2:
                d -= 2
            else:
                assert name in SAME, name
            assert d >= 0, "underflow"
            top["stack"] = max(top["stack"], d)
            i += 1
        return d

    walk(raw[0], 0, 0, 0, shade_locals)
    return top


def branch_probes(prog_raw):
    """for every If at the top level of `shade`: the op list that ends where the If would pop its condition, with SetColor in its
    place -- baked by the oracle, color.x is the condition every texel arrives with"""
    shade = prog_raw[0]
    return [shade[:i] + ["SetColor"] for i, op in enumerate(shade) if not isinstance(op, str) and op[0] == "If"]


def diverges(conditions):
    """conditions: [texels] in bake order; true when one run of 64 consecutive texels -- a wave -- holds both outcomes"""
    taken = np.asarray(conditions).reshape(-1) != 0.0
    return any(taken[i:i + 64].any() and not taken[i:i + 64].all() for i in range(0, len(taken), 64))


def vacuous(pixels):
    """the issue's definition at 24 x 16: fewer than half of the texels finite, or fewer than 48 distinct finite texels"""
    c = pixels[..., :3].reshape(-1, 3)
    finite = np.isfinite(c).all(axis=1)
    return finite.mean() < 0.5 or len(np.unique(bits(c[finite]), axis=0)) < 48


# ---- the opcode grids --------------------------------------------------------------------------------------------------------------
GRID = 64


def grid_index(axis):
    """column (axis 0) or 64 - row mod 64 (axis 1; the Mod matters: uv.y is 1.0 in the top row) of the texel, exact in f32"""
    return ["UV", ("GetComponents", [axis]), ("Push", float(N)), "Mul", "Floor", ("Push", float(N)), "Mod"]


def palette_operands(n):
    ops = grid_index(0) + ["PaletteIndex"]
    if n >= 2:
        ops += grid_index(1) + ["PaletteIndex"]
    if n >= 3:
        ops += grid_index(0) + grid_index(1) + ["Add", ("Push", float(N)), "Mod", "PaletteIndex"]
    return ops


# awkward constants: u * A + v * B + C per component, every product and sum rounded -- the same roundings on both sides
COMPUTED = [[(7.5677, 0.00731, -3.3), (3.1417, 0.0213, -1.07), (1234.5677, 0.731, -3.3)],
            [(0.0113, 5.123456, -2.2), (0.0171, 2.7183, -0.93), (0.377, 777.7771, -5.1)],
            [(0.9371, 0.4113, -0.17), (0.6113, 0.8371, -0.31), (1.9371, 1.4113, -1.7)]]


def computed_operand(which):
    ops = []
    for (a, b, c) in COMPUTED[which]:
        ops += ["UV", ("GetComponents", [0]), ("Push", a), "Mul", "UV", ("GetComponents", [1]), ("Push", b), "Mul", "Add", ("Push", c), "Add"]
    return ops + ["Pack3"]


def computed_operands(n):
    ops = []
    for k in range(n):
        ops += computed_operand(k)
    return ops


def arity(op):
    return 1 if op in UNARY else (2 if op in BINARY else 3)


def grid_programs(source):
    """{opcode: Program} -- operands..., Op, SetColor.  `palette`: the operands are palette slots by column, row and their sum;
    `computed`: functions of uv, and Clamp joins with Min / Max of its second and third operand as bounds (f32::clamp panics unless
    min <= max; with NaN operands in the palette no such arrangement holds for every cell, so the palette grid leaves Clamp to the
    random programs)"""
    operands = palette_operands if source == "palette" else computed_operands
    out = {op: Program([operands(arity(op)) + [op, "SetColor"]]) for op in UNARY + BINARY + TERNARY}
    if source == "computed":
        bc = computed_operand(1) + computed_operand(2)
        out["Clamp"] = Program([computed_operand(0) + bc + ["Min"] + bc + ["Max", "Clamp", "SetColor"]])
    return out


def grid_operands(source, y, x):
    """the operands a, b, c of grid cell (row y, column x), as float32 triples"""
    if source == "palette":
        ia, ib = x, (GRID - y) % N
        return [np.array(GRID_PALETTE[i], np.float32) for i in (ia, ib, (ia + ib) % N)]
    u, v = np.float32(x) / np.float32(GRID), np.float32(1.0) - np.float32(y) / np.float32(GRID)
    return [np.array([np.float32(np.float32(u * np.float32(a)) + np.float32(v * np.float32(b))) + np.float32(c) for (a, b, c) in COMPUTED[k]], np.float32)
            for k in range(3)]


# ---- programs whose value stack peaks at exactly n ------------------------------------------------------------------------------------
def depth_program(n):
    """n uv-derived values pushed and folded by Add; after the first n // 2 of them an If on uv.x adds one more term on part of
    every row, so that the lanes of a wave wait at two depths.  The stack peaks at exactly n entries (measured by high_water)."""
    term = lambda k: ["UV", ("Push", 0.5 + ((k * 37) % 64) / 7.0, 1.25 + ((k * 11) % 64) / 9.0, 0.0), "Mul"]   # noqa: E731
    cond = ["UV", ("GetComponents", [0]), ("Push", 0.45), "Lt"]
    if n == 1:
        return [cond + [("If", term(1) + ["SetColor"], term(2) + ["SetColor"])]]
    m = n // 2
    ops = []
    for k in range(m):
        ops += term(k)
    ops += cond + [("If", term(n) + ["Add"], None)]
    for k in range(m, n):
        ops += term(k)
    return [ops + ["Add"] * (n - 1) + ["SetColor"]]


# ---- the comparison ----------------------------------------------------------------------------------------------------------------
def differing(got, want):
    """[h][w][4] bool: where the reference is NaN the device must be NaN (any sign, any payload); everywhere else the 32-bit patterns
    must be equal -- infinities, zeros and the alpha of 1.0 included"""
    return ~np.where(np.isnan(want), np.isnan(got), bits(got) == bits(want))


def assert_same_floats(got, want, label, describe=None):
    """`describe(y, x)`: what to say about a differing texel (operands, the op list)"""
    assert got.shape == want.shape, label
    bad = differing(got, want)
    if bad.any():
        y, x, c = (int(v) for v in np.argwhere(bad)[0])
        raise AssertionError(f"{label}: {int(bad.sum())} floats differ; first at texel (x {x}, y {y}) channel {c}: device 0x{int(bits(got)[y, x, c]):08x} "
                             f"({got[y, x, c]!r}), oracle 0x{int(bits(want)[y, x, c]):08x} ({want[y, x, c]!r})" + (("; " + describe(y, x)) if describe else ""))


# ---- the C structs again, with the banks (rxr_check_bake / rxr_check_shaders of a set as the GPU test bakes it) --------------------
def check_set(programs):
    """(rxr_check_shaders status, [rxr_check_bake status per program], messages)"""
    import rusterix_amd

    lib = rusterix_amd.rxr_abi()
    s, keep = R.shader_set(programs)
    msg = C.create_string_buffer(512)
    rc = lib.rxr_check_shaders(C.byref(s), None, msg, 512)
    out, said = [], [msg.value.decode()]
    for i in range(len(programs)):
        out.append(lib.rxr_check_bake(C.cast(C.byref(s), C.c_void_p), i, msg, 512))
        said.append(msg.value.decode())
    return rc, out, said


# ---- references, computed once per process -----------------------------------------------------------------------------------------
_references = {}


def group_reference(oracle, seeds, size=SIZE):
    """the oracle's float pixels of every seed of a group at `size` (width, height); the arrays are shared: do not write to them"""
    key = (tuple(seeds), size)
    if key not in _references:
        ref = Reference(oracle, [generate(s)[0] for s in seeds])
        _references[key] = [ref.pixels(i, *size) for i in range(len(seeds))]
    return _references[key]


def grid_reference(oracle, source):
    """{opcode: the oracle's [64][64][4] pixels} of grid_programs(source)"""
    key = ("grid", source)
    if key not in _references:
        progs = grid_programs(source)
        ref = Reference(oracle, list(progs.values()), grid_assets)
        _references[key] = {op: ref.pixels(i, GRID, GRID) for i, op in enumerate(progs)}
    return _references[key]
