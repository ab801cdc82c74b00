"""Reference for the shader-texture bake (rxr_bake_shaders, include/rxr.h), shared by tests/test_bake_cpu.py and
tests/test_gpu_bake.py: Rusteria::shade over a W x H RenderBuffer (reference rusteria/src/lib.rs:161-210) restated with the oracle's
single-invocation entry point, and RenderBuffer::as_rgba_bytes (rusteria/src/renderbuffer.rs:88-107) in numpy.

float pixels: one orc_vm_shade per texel on a FRESH Execution with uv = (x / W, 1 - y / H, 0) in f32 and every other field at its
Execution::new value; then `+ 0.0`, what RenderBuffer::accum_from does to a value at accum == 1 (-0.0 -> +0.0).  For the programs
the device accepts a fresh Execution per texel is what the reference's per-tile Execution amounts to.
bytes: v = pow(c, 0.4545f) * 255 in float64 from those floats; the expected byte is trunc(v), saturated, NaN -> 0.  A device byte
may differ from it by exactly 1 only where v lies within BAND of an integer: BAND = 17 * 2^-24 * 255 -- 16 ulp for powf (the OpenCL
bound, the loosest the device library can be held to) plus one rounding of the product, at the top of the byte range.  The device's
powf is held to those 16 ulp over its whole domain by tests/test_gpu_libm_ulp.py, with 3 000 bases in [0, 1] at this very exponent;
what it measured on the device, and glibc's figure, are in profiles/libm_ulp/README.md (row Pow)."""
import ctypes as C

import numpy as np

from rusterix_amd.abi import rxr_function as RxrFunction, rxr_program as RxrProgram, rxr_shader_set as RxrShaderSet
from rusterix_amd.binding import Program

GAMMA = float(np.float32(0.4545))          # `let gamma_correction = 0.4545` is an f32 in the reference
BAND = 17.0 * 2.0 ** -24 * 255.0           # (the measured Pow maximum: profiles/libm_ulp/README.md)
FIELDS = ["uv", "color", "roughness", "metallic", "emissive", "opacity", "bump", "normal", "hitpoint", "time"]
SIZES = [(64, 64), (1, 1), (63, 65), (80, 80), (81, 1), (257, 3)]   # (width, height): the bake's own size, partial last workgroups, the reference's tile edge


def shader_set(programs):
    """(RxrShaderSet, keep-alive list) for a list of Program; no patterns, no palette"""
    keep = []
    progs = (RxrProgram * max(len(programs), 1))()
    for i, p in enumerate(programs):
        fns = (RxrFunction * max(len(p.functions), 1))()
        for k, f in enumerate(p.functions):
            arr = np.asarray(f if len(f) else [0], np.uint32)
            keep.append(arr)
            fns[k] = RxrFunction(arr.ctypes.data, len(f))
        keep.append(fns)
        progs[i] = RxrProgram(p.globals, p.shade_index, p.shade_locals, fns, len(p.functions))
    keep.append(progs)
    return RxrShaderSet(progs, len(programs), None, 0, None, 0, None, None, 0), keep


# ---- test material ---------------------------------------------------------------------------------------------------------------
def patterns():
    """two small colour patterns (and, reversed, the normal bank): multiples of 1/64, exact in f32"""
    rng = np.random.default_rng(0x42414B45)
    return [rng.integers(0, 65, size=(h, w, 3)).astype(np.float32) / np.float32(64.0) for (h, w) in ((8, 8), (5, 7))]


PALETTE = [(0.75, 0.25, 0.5), None, (0.125, 0.5, 0.875)]


def make_assets(api):
    pats = patterns()
    return api.Assets.default().patterns(pats).patterns(pats[::-1], normal=True).palette(PALETTE)


def P(ops, *functions, **kw):
    return Program([ops] + list(functions), **kw)


def exact_programs():
    """programs built from exactly rounded operations only (name -> Program): their float buffers are compared bit for bit"""
    from tests.test_oracle_reference_tests import FIB

    loop = [("Push", 0.0), ("StoreLocal", 0), "UV", ("GetComponents", [0]), ("Push", 12.0), "Mul", "Floor", ("StoreLocal", 2),
            ("For", [("Push", 0.0), ("StoreLocal", 1)], [("LoadLocal", 1), ("LoadLocal", 2), "Lt"],
             [("LoadLocal", 1), ("Push", 1.0), "Add", ("StoreLocal", 1)],
             [("LoadLocal", 1), ("Push", 2.0), "Mod", ("Push", 0.0), "Eq",
              ("If", [("LoadLocal", 0), ("Push", 0.07), "Add", ("StoreLocal", 0)], [("LoadLocal", 0), ("Push", 0.02), "Add", ("StoreLocal", 0)])]),
            ("LoadLocal", 0), "UV", ("GetComponents", [1]), "Mul", "SetColor"]
    return {
        "gradient": P(["UV", "SetColor"]),
        "arith": P(["UV", ("Push", 5.0), "Mul", "Fract", ("Push", 0.9, 0.1, 0.3), ("Push", 0.1, 0.8, 0.6), "UV", ("GetComponents", [1]), "Mix", "Mul",
                    ("Push", 0.05), ("Push", 0.85), "Clamp", ("Push", 0.3), "UV", ("GetComponents", [0]), "Step", ("Push", 0.25), "Mul", "Add",
                    "UV", ("Push", 7.0), "Mul", "Floor", ("Push", 0.03), "Mul", "Add", ("Push", 3.0), "Div", "SetColor"]),
        "loop": P(loop, shade_locals=3),
        "call": P(["UV", ("Push", 3.0), "Mul", ("FunctionCall", 1, 2, 1), "UV", ("GetComponents", [1, 0]), ("FunctionCall", 1, 2, 1), "Add",
                   ("Push", 0.25), "Mul", "SetColor"],
                  [("LoadLocal", 0), "Fract", ("StoreLocal", 1), ("LoadLocal", 1), ("LoadLocal", 1), "Mul", ("Push", 0.5), "Gt",
                   ("If", [("LoadLocal", 1), "Return"], None), ("LoadLocal", 0), ("Push", 0.5), "Mul", "Fract"]),
        "patterns": P(["UV", ("Push", 3.0), "Mul", ("Push", 0.0), "Sample", "UV", ("Push", 2.0), "Mul", ("Push", 1.0), "SampleNormal", ("Push", 0.25), "Mul", "Add",
                       "UV", ("Push", 5.0), "Mul", ("Push", 1.0), "Sample", ("Push", 0.5), "Mul", "Add", "UV", ("Push", 9.0), "Sample", "Add",
                       ("Push", 0.4), "Mul", "SetColor"]),
        # (PaletteIndex pushes nothing for the empty slot 1 and the missing slot 3: the constant below it is what gets multiplied then)
        "palette": P([("Push", 0.5), "UV", ("GetComponents", [0]), ("Push", 4.0), "Mul", "Floor", "PaletteIndex", "UV", ("GetComponents", [1]), "Mul", "SetColor"]),
        # a field that is only read holds its Execution::new constant: roughness 0.5, the rest 0 -- hitpoint and time included
        "fields": P(["Roughness", "UV", "Mul", "Metallic", "Add", "Opacity", "Add", "Bump", "Add", "Normal", "Add", "Hitpoint", "Add", "Time", "Add",
                     "Emissive", "Add", "SetColor"]),
        # ... and one that is written first may be read afterwards
        # (normal only: a program that writes roughness / metallic / opacity / bump makes rxr_set_shaders refuse the set "fields" is in)
        "written": P(["UV", ("Push", 0.0, 0.6, 0.8), "Add", "SetNormal", "Normal", ("Push", 0.5), "Mul", "UV", "Add", "SetColor"]),
        # the two programs the reference holds known answers for (rusteria/src/lib.rs:274-296), wrapped so that they set the colour
        "addition": P([("Push", 2.0), ("StoreGlobal", 0), ("LoadGlobal", 0), ("Push", 2.0), "Add", ("Push", 0.125), "Mul", "SetColor"], globals=1),
        "fib": P(["UV", ("GetComponents", [0]), ("Push", 6.0), "Mul", "Floor", ("FunctionCall", 1, 1, 1), ("Push", 0.125), "Mul", "SetColor"], FIB),
    }


STATIC_SET = ["gradient", "arith", "loop", "patterns", "fields", "written", "addition"]   # no calls, no PaletteIndex: static stack depths (k_bake_s)


def special_programs():
    """every class of value the cast rules of `as u8` treat specially, per channel: negative, zero, -0.0, one, above one, +-inf, NaN"""
    u = ["UV", ("GetComponents", [0])]
    return {
        "negative_zero_one": P(u + [("Push", 0.5), "Sub", ("Push", 0.0), ("Push", 1.0), "Pack3", "SetColor"]),            # (u - 0.5, 0, 1)
        "minus_zero_above_one": P(u + [("Push", 0.0), "Mul", "Neg", u[0], u[1], ("Push", 2.0), "Add", ("Push", 1.0), "Pack3", "SetColor"]),   # (-0.0, u + 2, 1)
        "infinities": P([("Push", 1.0), ("Push", 0.0), "Div", ("Push", -1.0), ("Push", 0.0), "Div"] + u + ["Pack3", "SetColor"]),   # (+inf, -inf, u)
        "nan": P([("Push", 0.0), ("Push", 0.0), "Div"] + u + [("Push", 0.5), "Sub", "Sqrt", ("Push", 1.0), "Pack3", "SetColor"]),   # (NaN, sqrt(u - 0.5), 1)
    }


def libm_programs():
    """sin / cos / pow / atan2 / ln: compared at +-1 per byte, floats not bitwise"""
    return {
        "sincos": P(["UV", ("Push", 6.0), "Mul", "Sin", ("Push", 0.5), "Mul", ("Push", 0.5), "Add", "UV", ("Push", 4.0), "Mul", "Cos", ("Push", 0.25), "Mul", "Add",
                     ("Push", 0.7), "Mul", "SetColor"]),
        "pow_atan2_ln": P(["UV", ("Push", 0.1), "Add", ("Push", 1.7), "Pow", "UV", ("Push", 0.2), "Add", "UV", ("GetComponents", [1, 0]), ("Push", 0.3), "Add",
                           "Atan2", ("Push", 0.3), "Mul", "Add", "UV", ("Push", 1.0), "Add", "Log", ("Push", 0.5), "Mul", "Add", ("Push", 0.4), "Mul", "SetColor"]),
    }


# ---- the reference ---------------------------------------------------------------------------------------------------------------
def uv_of(width, height):
    """uv per texel, row-major, top row first: (x as f32 / W as f32, 1.0 - (y as f32 / H as f32), 0.0)"""
    x = np.arange(width, dtype=np.float32) / np.float32(width)
    y = np.float32(1.0) - np.arange(height, dtype=np.float32) / np.float32(height)
    uv = np.zeros((height, width, 3), np.float32)
    uv[..., 0] = x[None, :]
    uv[..., 1] = y[:, None]
    return uv


class Reference:
    """an oracle scene holding `programs` (a list of Program) as scene.shaders, and the test assets"""

    def __init__(self, oracle, programs):
        self.oracle = oracle
        self.scene = oracle.Scene.empty()
        for p in programs:
            self.scene.add_program(p)
        self.assets = make_assets(oracle)
        self.shade = oracle.lib.orc_vm_shade
        self.shade.restype = C.c_int
        self.shade.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_float)]

    def pixels(self, program, width, height):
        """RenderBuffer.pixels of a width x height bake: [height][width][4] float32"""
        uv = uv_of(width, height).reshape(-1, 3)
        out = np.zeros((height * width, 4), np.float32)
        f = np.zeros((10, 3), np.float32)
        fp = f.ctypes.data_as(C.POINTER(C.c_float))
        for i in range(height * width):
            f[:] = 0.0
            f[2] = 0.5                     # Execution::new: roughness = broadcast(0.5)
            f[0] = uv[i]
            rc = self.shade(self.scene._h, self.assets._h, program, fp)
            assert rc == 0, f"the reference faulted in program {program} at texel {i}"
            out[i, :3] = f[1]
        out[:, :3] += np.float32(0.0)      # accum_from at accum == 1: old * 0 + new * 1 (-0.0 -> +0.0)
        out[:, 3] = 1.0
        return out.reshape(height, width, 4)


def gamma_values(pixels):
    """float64 pow(c, 0.4545f) * 255 of the colour channels"""
    c = pixels[..., :3].astype(np.float64)
    with np.errstate(all="ignore"):
        return np.power(c, GAMMA) * 255.0


def expected_bytes(pixels):
    """as_rgba_bytes of float pixels: trunc(v) saturated to [0, 255], NaN -> 0; alpha 255"""
    v = gamma_values(pixels)
    b = np.where(np.isnan(v), 0.0, np.clip(np.nan_to_num(v, nan=0.0, posinf=255.0, neginf=0.0), 0.0, 255.0))
    out = np.full(pixels.shape, 255, np.uint8)
    out[..., :3] = np.trunc(b).astype(np.uint8)
    return out


def boundary_band(pixels):
    """colour channels whose v lies within BAND of an integer in (0, 255]: where a correctly rounded pow and a 16-ulp pow may truncate
    to different bytes.  Channels the cast rules decide (c <= 0, c == 1, c > 1, infinities, NaN, -0.0) are never in the band."""
    c = pixels[..., :3]
    v = gamma_values(pixels)
    with np.errstate(all="ignore"):
        near = (np.abs(v - np.rint(v)) <= BAND) & (np.rint(v) >= 1)
    decided = ~(c > 0) | (c >= 1) | ~np.isfinite(c)
    return near & ~decided


def check_bytes(got, pixels, label):
    """device bytes against the reference floats: exact outside the boundary band, off by exactly 1 at most inside it"""
    want = expected_bytes(pixels)
    assert got.shape == want.shape, label
    assert (got[..., 3] == 255).all(), f"{label}: alpha"
    diff = np.abs(got[..., :3].astype(np.int16) - want[..., :3].astype(np.int16))
    band = boundary_band(pixels)
    bad = (diff != 0) & ~band
    assert not bad.any(), f"{label}: {int(bad.sum())} channels differ outside the boundary band; first at {np.argwhere(bad)[:3].tolist()}"
    assert int(diff.max(initial=0)) <= 1, f"{label}: a channel in the boundary band differs by {int(diff.max())}"
    return int((diff != 0).sum()), int(band.sum())
