"""Material for comparing the run-time COMPILED form of Rusteria programs (rxr_jit.hip, rxr_jit_ops.h) with the interpreter and the
oracle float for float in FRAMES, shared by tests/test_jit_floats_cpu.py (no GPU: the windows hide nothing, the material is not
vacuous) and tests/test_gpu_jit_floats.py.

A frame shows a program's colour as a byte, 256 levels.  Every program here therefore ends in

    <value: a Vec3>  Time  Mul  Fract  SetColor

and its set is rendered once per WINDOW k with time = 2^k: `Time` is a uniform, so nothing is compiled again, r * 2^k is exact,
Fract of it is exact below 2^23, and f32_to_u8_saturated (rxr_kernels.hip) is linear -- a window shows a little under eight bits of
r, the windows overlap (k steps by 7), and together they show every bit of every finite r with 2^-11 <= |r| < 2^7, and zero
(tests/test_jit_floats_cpu.py proves it on 53 248 pairs of neighbouring floats).  Not shown: the sign of a zero and which non-finite
value a channel holds -- the class twins of the opcode grids show those.

  * FrameProgramGen: bake_fuzz.BakeProgramGen without `Time` among its sources and with the tail above; 96 seeds in six groups of 16, uploaded four (static) or two (dynamic) programs at a time;
  * the opcode grids: one program per operation over the 64 x 64 pairs of bake_fuzz.TABLE (one pixel centre per pair), in nine sets;
  * directed control flow, one set.

No libm opcode appears anywhere here (tests/test_gpu_libm_ulp.py owns those), so no tolerance does either."""
import numpy as np

from rusterix_amd import binding as B
from rusterix_amd import scenes
from rusterix_amd.binding import Program
from tests import bake_fuzz as F
from tests import bake_ref as R

# ---- the windows -------------------------------------------------------------------------------------------------------------------
WINDOWS = (-8, -1, 6, 13, 20, 27)      # time = 2^k
TOP_BITS = 7                           # of a window's eight bits, the ones two neighbouring floats cannot share
TAIL = ["Time", "Mul", "Fract", "SetColor"]
SHOWN_BELOW = 2.0 ** (-WINDOWS[0] - 1)                   # |r| < 2^7: the lowest window keeps one bit above the value, for its sign
SHOWN_LAST_BIT = 2.0 ** (-WINDOWS[-1] - TOP_BITS)        # 2^-34: the smallest bit weight inside the top bits of the highest window
SHOWN_FROM = SHOWN_LAST_BIT * 2.0 ** 23                  # 2^-11 <= |r|: the last mantissa bit of such a float weighs 2^-34 or more
LIBM = {"Sin", "Sin1", "Sin2", "Cos", "Cos1", "Cos2", "Tan", "Atan", "Log", "Atan2", "Pow", "Rotate2D"}


def fully_shown(r):
    """the floats the windows show bit for bit: zero, or finite with SHOWN_FROM <= |r| < SHOWN_BELOW"""
    r = np.asarray(r, np.float32)
    with np.errstate(invalid="ignore"):
        return (r == 0) | (np.isfinite(r) & (np.abs(r) >= SHOWN_FROM) & (np.abs(r) < SHOWN_BELOW))


def with_tail(ops):
    """an op list with every SetColor replaced by the tail, nested blocks included"""
    out = []
    for op in ops:
        if op == "SetColor":
            out += TAIL
        elif not isinstance(op, str) and op[0] in ("If", "For"):
            out.append((op[0],) + tuple(None if b is None else with_tail(b) for b in op[1:]))
        else:
            out.append(op)
    return out


def P(functions, **kw):
    """a Program that keeps its op lists: `raw` (the functions, `shade` first)"""
    prog = Program(functions, **kw)
    prog.raw = functions
    return prog


def time_reads_outside_tails(ops):
    """how many `Time` an op list holds that are not the first opcode of a tail, nested blocks included"""
    n, i = 0, 0
    while i < len(ops):
        op = ops[i]
        if ops[i:i + len(TAIL)] == TAIL:
            i += len(TAIL)
            continue
        if op == "Time":
            n += 1
        elif not isinstance(op, str) and op[0] in ("If", "For"):
            n += sum(time_reads_outside_tails(b) for b in op[1:] if b is not None)
        i += 1
    return n


def value_ops(raw):
    """every opcode name of a program's functions with the tail of `shade` taken off: what must not read Time"""
    assert raw[0][-len(TAIL):] == TAIL
    return set().union(F.op_names(raw[0][:-len(TAIL)]), *(F.op_names(f) for f in raw[1:]))


# ---- frames ------------------------------------------------------------------------------------------------------------------------
def fuzz_assets(api):
    return F.fuzz_assets(api)


def grid_assets(api):
    """the 64-slot operand palette of bake_fuzz and the fuzz patterns (Sample / SampleNormal)"""
    pats = R.patterns()
    return api.Assets.default().patterns(pats).patterns(pats[::-1], normal=True).palette(F.GRID_PALETTE)


class Frame:
    """one 2D rectangle per program (cell = (width, height) pixels, `cols` to a row), as test_gpu_shader_jit.grid_scene lays them
    out: every program of the set runs in the same frame.  The set is uploaded with the first window and stays resident for the
    others: only `time` changes between them."""

    def __init__(self, api, programs, cell, cols, assets_of):
        scene = api.Scene.empty()
        cw, ch = cell
        rows = (len(programs) + cols - 1) // cols
        for k, prog in enumerate(programs):
            idx = scene.add_program(prog)
            r = api.Batch2D.from_rectangle(float((k % cols) * cw), float((k // cols) * ch), float(cw), float(ch))
            r.source(B.PixelSource.StaticTileIndex(0)).shader(idx)
            scene.add_d2_static(r)
        assets = assets_of(api).textures([B.Tile.from_texture(scenes.noise_texture(5, 32, 32))])
        self.time = 1.0
        self.cell, self.cols, self.n = cell, cols, len(programs)
        self.cfg = scenes._result(api, scene, assets, lambda: api.Rasterizer.setup(None, B.Mat4.identity(), B.Mat4.identity()).time(self.time),
                                  cols * cw, rows * ch, 40, "jit-floats")

    def at(self, time):
        self.time = float(time)
        return scenes.render(self.cfg).copy()

    def windows(self):
        """[len(WINDOWS)][height][width][4] bytes"""
        return np.stack([self.at(2.0 ** k) for k in WINDOWS])


SITE_W, SITE_H = 384, 256
SITES = ["cube", "pane"]


class SiteFrame(Frame):
    """the programs of a set at the 3D call sites, one small box each in a lattice in front of an orbit camera, under ambient light
    alone (no light source: nothing of the lighting goes through libm).  `cube`: opaque boxes run the scene's programs (the opaque
    pass); `pane`: thin boxes on a chunk's opacity list run the CHUNK's programs, over an opaque box with a program of its own, as
    tests/test_gpu_shader_jit.py builds its pane.  The sRGB encode of these passes is not linear: the windows prove nothing about
    completeness here, the three frames are only compared."""

    def __init__(self, api, programs, assets_of, site):
        scene = api.Scene.empty()
        n = len(programs)
        cols = int(np.ceil(np.sqrt(n)))
        step = 2.4 / cols
        size = float(np.float32(0.85 * step))
        at = lambda k: (float(np.float32(-1.2 + (k % cols) * step)), float(np.float32(-1.2 + (k // cols) * step)))   # noqa: E731
        if site == "cube":
            for k, prog in enumerate(programs):
                box = api.Batch3D.from_box(*at(k), -size / 2, size, size, size).cull_mode(B.CULL_OFF).with_computed_normals()
                box.source(B.PixelSource.StaticTileIndex(0)).repeat_mode(B.REPEAT_REPEAT_XY).shader(scene.add_program(prog))
                scene.add_d3_static(box)
        else:
            back = api.Batch3D.from_box(-1.3, -1.3, -0.4, 2.6, 2.6, 0.2).cull_mode(B.CULL_OFF).with_computed_normals()
            back.source(B.PixelSource.StaticTileIndex(0)).repeat_mode(B.REPEAT_REPEAT_XY).shader(scene.add_program(Program([["Color", "SetColor"]])))
            scene.add_d3_static(back)
            chunk = scene.add_chunk()
            for k, prog in enumerate(programs):
                chunk.add_shader(prog)
                pane = api.Batch3D.from_box(*at(k), 0.3, size, size, 0.02).with_computed_normals().source(B.PixelSource.Pixel((200, 220, 90, 255))).shader(k)
                chunk.add_batch3d_opacity(pane)
        assets = assets_of(api).textures([B.Tile.from_texture(scenes.noise_texture(6, 32, 32))])
        cam = api.D3OrbitCamera.new()
        cam.set_parameter_f32("distance", 3.2)
        cam.azimuth = 1.0
        cam.elevation = 0.5
        self.time = 1.0

        def setup():
            v, p = cam.matrices(float(SITE_W), float(SITE_H))
            return api.Rasterizer.setup(None, v, p).ambient((0.3, 0.3, 0.35, 1.0)).time(self.time)

        self.cfg = scenes._result(api, scene, assets, setup, SITE_W, SITE_H, 40, "jit-floats-" + site)


class FrameSet:
    """a named set: its programs, how its frame is laid out, and what to say about a pixel of program i"""

    def __init__(self, name, programs, cell, cols, assets_of, describe):
        self.name, self.programs, self.cell, self.cols, self.assets_of, self.describe = name, programs, cell, cols, assets_of, describe

    def frame(self, api):
        return Frame(api, self.programs, self.cell, self.cols, self.assets_of)


_reference = {}


def reference_windows(oracle, fs):
    """the oracle's frames of a set in every window, computed once per process; shared: do not write to them"""
    if fs.name not in _reference:
        w = fs.frame(oracle).windows()
        w.setflags(write=False)
        _reference[fs.name] = w
    return _reference[fs.name]


# ---- the random programs -----------------------------------------------------------------------------------------------------------
GROUP = 16
FUZZ_CELL, FUZZ_COLS = (48, 32), 4      # 1 536 pixel centres per program; the frame is 192 x 128
N_SEEDS = 96
# seeds whose oracle frames show fewer than 25 % of their channels fully (measured by tests/test_jit_floats_cpu.py, which also holds
# this list to its rule): each is replaced by the next unused seed of its class
REPLACED = {10: 96, 74: 98, 78: 100, 94: 102, 9: 97, 71: 99}


class FrameProgramGen(F.BakeProgramGen):
    """BakeProgramGen for a frame: `Time` is the window factor, so no value reads it, and the colour leaves through the tail.  Bake-legal
    programs are frame-legal (rxr_set_shaders' rules are the weaker ones); the other inputs differ from a bake's -- uv / 4, the texel as
    Color, the world position as Hitpoint."""

    def __init__(self, rng, cls):
        super().__init__(rng, cls)
        self.sources = [s for s in self.sources if s != "Time"]

    def program(self):
        super().program()
        assert self.raw[0][-1] == "SetColor"
        self.raw = [self.raw[0][:-1] + TAIL] + self.raw[1:]
        return P(self.raw, shade_locals=self.shade_locals, globals=self.n_globals)


_generated = {}


def generate(seed):
    """(Program, its generator) of a seed; the generator keeps raw (the op lists), cls, shade_locals, n_globals"""
    if seed not in _generated:
        gen = FrameProgramGen(np.random.default_rng([0x52585231, 5160, seed]), F.class_of(seed))
        _generated[seed] = (gen.program(), gen)
    return _generated[seed]


def seeds_in_use():
    out = []
    for s in range(N_SEEDS):
        while s in REPLACED:
            s = REPLACED[s]
        out.append(s)
    return out


def groups(cls):
    """the seeds of a class, GROUP to a shader set: three sets per class"""
    seeds = [s for s in seeds_in_use() if F.class_of(s) == cls]
    return [seeds[i:i + GROUP] for i in range(0, len(seeds), GROUP)]


# programs per uploaded set: a set of 16 compiles for 8 to 16 s and a dynamic set of 4 for up to 6 s -- slower than the slowest set of
# tests/test_gpu_shader_jit.py (5.7 s); these sizes keep every set below it
PART = {"static": 4, "dynamic": 2}


def random_sets():
    """the six groups of 16, each uploaded PART[class] programs at a time (profiles/jit_floats/README.md: the compile seconds)"""
    out = []
    for cls in ("static", "dynamic"):
        for g, group in enumerate(groups(cls)):
            for j in range(0, GROUP, PART[cls]):
                seeds = group[j:j + PART[cls]]

                def describe(i, y, x, seeds=seeds):
                    return f"seed {seeds[i]} ({F.class_of(seeds[i])}), gen.raw = {generate(seeds[i])[1].raw}"
                out.append(FrameSet(f"random-{cls}-{g}.{j // PART[cls]}", [generate(s)[0] for s in seeds], FUZZ_CELL, FUZZ_COLS, fuzz_assets, describe))
                out[-1].seeds, out[-1].group = seeds, f"{cls}-{g}"
    return out


def shown_twin(seed):
    """the program of a seed with this in place of the tail: per channel 1.0 where the value is fully shown, else 0.0 -- in exact
    operations, so that the oracle's frame of it counts what the oracle's frames of the program show"""
    gen = generate(seed)[1]
    keep = gen.shade_locals
    ops = gen.raw[0][:-len(TAIL)] + [("StoreLocal", keep)]
    for c in range(3):
        a = [("LoadLocal", keep), ("GetComponents", [c]), "Abs"]
        ops += a + [("Push", SHOWN_FROM), "Ge"] + a + [("Push", SHOWN_BELOW), "Lt", "And", ("LoadLocal", keep), ("GetComponents", [c]), ("Push", 0.0), "Eq", "Or"]
    return Program([ops + ["Pack3", "SetColor"]] + gen.raw[1:], shade_locals=keep + 1, globals=gen.n_globals)


def shown_share(oracle, seeds):
    """per seed of a set: the share of channel-pixels of its cell that the windows show fully, from the oracle's frame of the twins"""
    frame = Frame(oracle, [shown_twin(s) for s in seeds], FUZZ_CELL, FUZZ_COLS, fuzz_assets).at(1.0)
    assert set(np.unique(frame[..., :3])) <= {0, 255}
    cw, ch = FUZZ_CELL
    return [float((frame[(i // FUZZ_COLS) * ch:(i // FUZZ_COLS + 1) * ch, (i % FUZZ_COLS) * cw:(i % FUZZ_COLS + 1) * cw, :3] == 255).mean()) for i in range(len(seeds))]


# ---- the opcode grids --------------------------------------------------------------------------------------------------------------
N = F.N                       # 64 operands: a by the pixel's column, b by its row, c by their sum
GRID_CELL, GRID_COLS = (N, N), 8
SWIZZLES = [[0], [2, 0], [1, 2, 0], [1, 1], [3, 1]]          # (3: "not a component", skipped by GetComponents, ignored by SetComponents)
BINC_OPS = ["Add", "Sub", "Mul", "Div", "Min", "Max", "Mod", "Lt", "Le", "Gt", "Ge", "Eq", "Ne"]     # VM_BINC_ADD .. VM_BINC_NE
BINC_CONSTANTS = [0.37, -2.5, 0.0, -0.0, 1e-40]
PATTERN_IDS = [1.0, 9.0]                                      # two patterns exist: 9 names none (the result is zero)
assert set(BINC_OPS) == F.FUSABLE


def slot(axis):
    """the operand index of the pixel: the 2D pass hands uv / 4 to programs, a cell has N pixels a side, so uv * 4 N is the pixel's
    column (row) plus one half; exact in f32"""
    return ["UV", ("GetComponents", [axis]), ("Push", 4.0 * N), "Mul", "Floor", ("Push", float(N)), "Mod"]


def operands(n):
    ops = slot(0) + ["PaletteIndex"]
    if n >= 2:
        ops += slot(1) + ["PaletteIndex"]
    if n >= 3:
        ops += slot(0) + slot(1) + ["Add", ("Push", float(N)), "Mod", "PaletteIndex"]
    return ops


# Clamp: f32::clamp panics unless min <= max, and with NaN in the palette no pair of slots is ordered in every cell: the bounds are
# min(b, c, 0) and max(b, c, 0) -- f32::min / max drop a NaN operand, so the two are ordered and never NaN
_BC = operands(3)[len(operands(1)):]
CLAMP_OPERANDS = operands(1) + _BC + ["Min", ("Push", 0.0), "Min"] + _BC + ["Max", ("Push", 0.0), "Max"]


def class_flags(keep):
    """what the windows cannot show of the Vec3 in local `keep`, per component: r > 0, 1 / r > 0 (the sign of a zero), r != r,
    |r| > 3e38 -- the flags of test_gpu_shader_edge_values.programs_for and the sign of an infinity, the four of a component packed
    into one channel as sixteenths (sixteen different bytes)"""
    ops = []
    for c in range(3):
        r = [("LoadLocal", keep), ("GetComponents", [c])]
        ops += r + [("Push", 0.0), "Gt", ("Push", 8.0), "Mul"]
        ops += [("Push", 1.0)] + r + ["Div", ("Push", 0.0), "Gt", ("Push", 4.0), "Mul", "Add"]
        ops += r + r + ["Ne", ("Push", 2.0), "Mul", "Add"]
        ops += r + ["Abs", ("Push", 3.0e38), "Gt", "Add", ("Push", 0.0625), "Mul"]
    return ops + ["Pack3", "SetColor"]


class GridEntry:
    def __init__(self, label, n_operands, ops, load=None, twin=False):
        self.label, self.n_operands, self.ops, self.twin = label, n_operands, ops, twin
        self.load = operands(n_operands) if load is None else load

    def program(self):
        return P([self.load + self.ops + TAIL])

    def class_program(self):
        return P([self.load + self.ops + [("StoreLocal", 0)] + class_flags(0)], shade_locals=1)


def grid_entries():
    """{set name: [GridEntry]}: every operation, in sets small enough to compile in about five seconds each"""
    # a unary operation's operand is (a.x, b.x, c.x): 4 096 triples of every pairing of magnitudes, where a palette slot alone would
    # give 64 triples whose components lie exponents apart (the association of a sum of squares shows only between like magnitudes)
    unary = [GridEntry(op + " of (a.x, b.x, c.x)", 3, [op], load=operands(3) + ["Pack3"]) for op in F.UNARY]
    binary = [GridEntry(op, 2, [op]) for op in F.BINARY]
    other = [GridEntry("Mix", 3, ["Mix"], twin=True), GridEntry("Smoothstep", 3, ["Smoothstep"], twin=True),
             GridEntry("Clamp", 3, ["Clamp"], load=CLAMP_OPERANDS, twin=True), GridEntry("Pack2", 2, ["Pack2"]), GridEntry("Pack3", 3, ["Pack3"])]
    other += [GridEntry(f"GetComponents {sw}", 1, [("GetComponents", sw)]) for sw in SWIZZLES]
    other += [GridEntry(f"SetComponents {sw}", 2, [("SetComponents", sw)]) for sw in SWIZZLES]
    other += [GridEntry("SetNormal, Normal of (a.x, b.x, c.x)", 3, ["SetNormal", "Normal"], load=operands(3) + ["Pack3"])]
    other += [GridEntry(f"{op} {int(i)}", 1, [("Push", i), op]) for op in ("Sample", "SampleNormal") for i in PATTERN_IDS]
    binc = {op: [GridEntry(f"Push {c!r}; {op}", 1, [("Push", c), op], twin=True) for c in BINC_CONSTANTS] for op in BINC_OPS}
    pick = lambda ops: [e for op in ops for e in binc[op]]   # noqa: E731
    return {"grid-unary": unary, "grid-ternary": other[:5], "grid-swizzle": other[5:], "grid-binc-min-max": pick(["Min", "Max"]),
            "grid-binary": binary, "grid-binc-0": pick(["Add", "Sub"]), "grid-binc-1": pick(["Mul", "Div"]), "grid-binc-2": pick(["Mod", "Lt", "Le"]),
            "grid-binc-3": pick(["Gt", "Ge", "Eq", "Ne"])}


def grid_operands(entry, y, x):
    """the operands of the pixel (row y, column x) of an entry's cell, as float32 triples"""
    idx = [x, y, (x + y) % N][:entry.n_operands]
    return [np.array(F.GRID_PALETTE[i], np.float32) for i in idx]


def grid_sets():
    out = []
    for name, entries in grid_entries().items():
        slots = [(e, False) for e in entries] + [(e, True) for e in entries if e.twin]

        def describe(i, y, x, slots=slots):
            e, twin = slots[i]
            said = ", ".join(f"{n} = {v.tolist()} (0x{' 0x'.join(format(int(b), '08x') for b in F.bits(v))})" for n, v in zip("abc", grid_operands(e, y, x)))
            return f"{e.label}{' (class flags)' if twin else ''}: operands {said}"
        out.append(FrameSet(name, [e.class_program() if twin else e.program() for e, twin in slots], GRID_CELL, GRID_COLS, grid_assets, describe))
        out[-1].slots = slots
    return out


def slot_probe():
    """(column index, row index, 0) / 255 of a grid cell's pixel: the oracle's frame of it says which pixel reads which operands"""
    return Program([slot(0) + slot(1) + [("Push", 0.0), "Pack3", ("Push", 255.0), "Div", "SetColor"]])


# ---- directed control flow ---------------------------------------------------------------------------------------------------------
DEPTHS = [1, 2, 3, 4, 5, F.VM_STACK - 1]      # tests/test_gpu_bake_fuzz.py's, less RXR_VM_STACK itself: the compiler refuses a value stack that deep
REFUSED_DEPTH = F.VM_STACK                     # (tests/test_jit_floats_cpu.py holds both to rxr_debug_jit_generate)
FACT = [("LoadLocal", 0), ("Push", 1.0), "Le", ("If", [("Push", 1.0), "Return"], None),
        ("LoadLocal", 0), ("LoadLocal", 0), ("Push", 1.0), "Sub", ("FunctionCall", 1, 1, 1), "Mul", "Return"]
# even(n) = n == 0 ? 1 : odd(n - 1);  odd(n) = n == 0 ? 0 : even(n - 1)   (odd keeps a second local)
EVEN = [("LoadLocal", 0), ("Push", 0.0), "Eq", ("If", [("Push", 1.0), "Return"], None), ("LoadLocal", 0), ("Push", 1.0), "Sub", ("FunctionCall", 1, 2, 2), "Return"]
ODD = [("LoadLocal", 0), ("StoreLocal", 1), ("LoadLocal", 1), ("Push", 0.0), "Eq", ("If", [("Push", 0.0), "Return"], None),
       ("LoadLocal", 1), ("Push", 1.0), "Sub", ("FunctionCall", 1, 1, 1), "Return"]
FULL = ("Push", 1.2345678, 0.87654321, 3.1415927)            # full-mantissa factors


def control_flow_programs():
    """{name: Program}: the generator's slot assignment under lane divergence (uv / 4 reaches the program: uv.x * 40 runs over 0 .. 9
    across a rectangle, so neighbouring lanes of a wave take different trip counts and branches)"""
    ux, uy = ["UV", ("GetComponents", [0])], ["UV", ("GetComponents", [1])]
    loop = [("Push", 0.0), ("StoreLocal", 0)] + ux + [("Push", 40.0), "Mul", "Floor", ("StoreLocal", 2),
            ("For", [("Push", 0.0), ("StoreLocal", 1)], [("LoadLocal", 1), ("LoadLocal", 2), "Lt"], [("LoadLocal", 1), ("Push", 1.0), "Add", ("StoreLocal", 1)],
             [("LoadLocal", 0), ("Push", 1.0371), "Mul", "UV", FULL, "Mul", "Add", ("StoreLocal", 0), ("Push", 5.0)]),      # (a temporary the loop truncates)
            ("LoadLocal", 0), ("LoadLocal", 2), ("Push", 0.137), "Mul", "Add"] + TAIL
    if_value = ux + [("Push", 0.11), "Gt", ("If", ["UV", FULL, "Mul", ("Push", 7.3), "Mul"], ["UV", FULL, "Div", ("Push", 0.3), "Add"])] + uy + ["Add"] + TAIL
    early = ux + [("Push", 0.07), "Lt", ("If", ["UV", FULL, "Mul"] + TAIL + ["Return"], None), "UV", ("Push", 4.0), "Mul", FULL, "Add"] + TAIL
    fact = ux + [("Push", 24.0), "Mul", "Floor", ("FunctionCall", 1, 1, 1), "UV", FULL, "Mul", "Mul"] + TAIL          # 0! .. 5!, times a full mantissa
    parity = ux + [("Push", 28.0), "Mul", "Floor", ("FunctionCall", 1, 1, 1), "UV", FULL, "Mul", "Mul", "UV", "Add"] + TAIL
    out = {"for with a per-pixel trip count": P([loop], shade_locals=3), "if as a value": P([if_value]),
           "early return inside an if": P([early]), "factorial": P([fact, FACT]), "even / odd": P([parity, EVEN, ODD])}
    for n in DEPTHS:      # (sums of up to 64 terms below 2.4: a quarter of them stays below 2^7)
        raw = F.depth_program(n)[0]
        raw = [op for o in raw for op in ([("Push", 0.25), "Mul", o] if o == "SetColor" else [o])] if n > 1 else raw
        out[f"stack depth {n}"] = P([with_tail(raw)])
    return out


def control_flow_set():
    progs = control_flow_programs()
    names = list(progs)
    return FrameSet("control-flow", list(progs.values()), (48, 32), 4, fuzz_assets, lambda i, y, x: names[i])


def all_sets():
    return random_sets() + grid_sets() + [control_flow_set()]


# ---- the comparison ----------------------------------------------------------------------------------------------------------------
def assert_same_frames(fs, ref, interp, compiled, note=""):
    """[windows][h][w][4] bytes three ways: equal everywhere, or the first differing pixel with its program, window and bytes"""
    assert ref.shape == interp.shape == compiled.shape, (fs.name, ref.shape, interp.shape, compiled.shape)
    bad = ((ref != interp) | (ref != compiled)).any(axis=3)
    if bad.any():
        cw, ch = fs.cell
        per_window = bad.reshape(len(bad), -1).sum(axis=1).tolist()
        k, y, x = (int(v) for v in np.argwhere(bad)[0])
        i, cy, cx = (y // ch) * fs.cols + (x // cw), y % ch, x % cw
        progs = sorted({(int(yy) // ch) * fs.cols + (int(xx) // cw) for _, yy, xx in np.argwhere(bad)})
        raise AssertionError(f"{fs.name}{note}: {int(bad.sum())} pixels differ (per window {dict(zip(WINDOWS, per_window))}) in programs {progs}; first in "
                             f"window 2^{WINDOWS[k]} at pixel (x {x}, y {y}), program {i} cell (x {cx}, y {cy}): oracle {ref[k, y, x].tolist()}, interpreted "
                             f"{interp[k, y, x].tolist()}, compiled {compiled[k, y, x].tolist()}; {fs.describe(i, cy, cx)}")
