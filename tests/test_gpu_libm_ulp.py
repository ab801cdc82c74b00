"""The libm-backed opcodes on the device in ulps (tests/libm_ref.py): Sin, Sin1, Sin2, Cos, Cos1, Cos2, Tan, Atan, Log, Atan2, Pow and
Rotate2D over whole-domain operand sets -- range reduction at large arguments, neighbours of k pi/2, Log next to 1, Pow with a base
next to 1 and a large exponent, denormal operands and results -- against a float64 reference, at the single-precision bounds of the
OpenCL full profile (sin / cos 4, tan 5, atan 5, atan2 6, log 3, pow 16 ulp; Rotate2D: the absolute bound derived from them in
libm_ref.rotate_reference).  The bounds come from that standard, not from what the device measures; the measured maxima are printed
(pytest -s) and recorded in profiles/libm_ulp/README.md.

A 64 x 64 bake puts each operand in front of the opcode and returns its f32 result bit for bit (k_bake_s); the same programs with
the opcode inside a function take k_bake and must return the same floats; and the frame paths -- the interpreter kernels
(RXR_SHADER_JIT=0) and the run-time compiled ones (RXR_SHADER_JIT=1) -- are tied to those floats by showing eight bits of each
result at a time, Fract(r * 2^k) for k = 0, 8, 16, 24, next to a libm-free twin that samples the bake's own result."""
import numpy as np
import pytest

from rusterix_amd import binding as B
from rusterix_amd import scenes
from rusterix_amd.binding import Program
from tests import libm_ref as L
from tests.test_gpu_shader_jit import jit_info

pytestmark = pytest.mark.gpu
W, H = L.W, L.H
FW, FH = 256, 160            # the frame: four rectangles of 128 x 80, each showing a whole 64 x 64 pattern
SHIFTS = [0, 8, 16, 24]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_floats(a, b):
    """bit for bit, any NaN for a NaN"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))


def device_bake(product, progs, patterns):
    """[len(progs)][H][W][3] per operand texel"""
    scene = product.Scene.empty()
    for p in progs:
        scene.add_program(p)
    assets = product.Assets.default().patterns(patterns)
    px = scene.bake_shaders(list(range(len(progs))), W, H, assets=assets, rgba=False)["pixels"]
    assert (px[..., 3] == 1.0).all()
    return [L.by_operand(px[i]) for i in range(len(progs))]


_DEVICE = {}


def device_results(product, op):
    """the opcode on its operand set through k_bake_s; computed once, not to be written to"""
    if op not in _DEVICE:
        r = device_bake(product, [L.program(op)], L.operand_set(op).patterns())[0].copy()
        r.setflags(write=False)
        _DEVICE[op] = r
    return _DEVICE[op]


# ---- the bake --------------------------------------------------------------------------------------------------------------------
def test_pass_through_agrees_with_the_cpu_run_bit_for_bit(oracle, product):
    o = L.oracle_results(oracle)
    index = np.zeros((H, W, 3), np.float32)
    index[..., 0], index[..., 1], index[..., 2] = np.arange(W)[None, :], np.arange(H)[:, None], np.arange(W * H).reshape(H, W)
    for name, pattern in [("index", index)] + [(op, L.operand_set(op).a) for op in ("Sin", "Atan", "Log", "Pow")]:
        got = device_bake(product, [L.PASS_THROUGH], [pattern])[0]
        want = L.by_operand(o.bake(L.PASS_THROUGH, [pattern]))
        assert same_floats(got, want).all(), f"{name}: {int((~same_floats(got, want)).sum())} operands come back differently on the device"
        denormal = (pattern != 0) & (np.abs(pattern) < 2.0 ** -126)
        assert np.array_equal(bits(got)[denormal], bits(pattern)[denormal]), f"{name}: a denormal operand did not reach the program"


@pytest.mark.parametrize("op", L.OPS)
def test_class_rule_and_ulp_bound(product, op):
    v = L.judge(op, device_results(product, op))
    print("\ndevice " + v.line())
    assert not v.failures, v.message()


def test_the_two_bake_kernels_return_the_same_floats(product):
    """the opcode inside a function: the set has a call, so no static stack depths -- k_bake instead of k_bake_s"""
    for op in L.OPS:
        wrapped = device_bake(product, [L.program(op, wrapped=True)], L.operand_set(op).patterns())[0]
        same = same_floats(wrapped, device_results(product, op))
        assert same.all(), f"{op}: {int((~same).sum())} floats differ between k_bake and k_bake_s; first at {np.argwhere(~same)[:3].tolist()}"


@pytest.mark.parametrize("op", L.OPS)
def test_oracle_and_device_differ_by_no_more_than_their_two_errors(oracle, product, op):
    """the float form of the +-1 byte the byte-level tests assume: outside the exemption band, |device - oracle| is at most the
    opcode's bound plus the oracle's own measured maximum, in ulps of the reference; and their classes agree"""
    s = L.operand_set(op)
    orc = L.oracle_results(oracle).results(op)
    dev = device_results(product, op)
    own = L.judge(op, orc)
    assert not own.failures, own.message()
    m = L.used(op) & L.judged_mask(op)
    assert np.array_equal(L.classes(orc)[m], L.classes(dev)[m]) or op == "Rotate2D", f"{op}: classes differ at {np.argwhere(m & (L.classes(orc) != L.classes(dev)))[:3].tolist()}"
    finite = np.isfinite(orc) & np.isfinite(dev) & m
    with np.errstate(all="ignore"):
        diff = np.abs(orc.astype(np.float64) - dev.astype(np.float64))
    if op == "Rotate2D":
        allowed = L.rotate_reference(s.a, s.b)[1] * (1.0 + own.max_ulp) + 2.0 ** -149      # (own.max_ulp: the oracle's error as a fraction of the bound)
    else:
        allowed = (L.BOUND[op] + own.max_ulp) * L.ulp32(L.reference(op, s.a, s.b))
    bad = finite & ~(diff <= allowed)
    print(f"\n{op}: oracle and device differ in {int((finite & (diff > 0)).sum())} of {int(finite.sum())} finite results")
    assert not bad.any(), f"{op}: {int(bad.sum())} results differ by more than the two errors allow; first at {np.argwhere(bad)[:3].tolist()}"


# ---- the frame paths -------------------------------------------------------------------------------------------------------------
def encode(k):
    return [("Push", float(2.0 ** k)), "Mul", "Fract", "SetColor"]


def fetch(pattern):
    """the 2D pass hands uv / 4 to the program: uv * 4 runs over [0, 1) across the rectangle"""
    return ["UV", ("Push", 4.0), "Mul", ("Push", float(pattern)), "Sample"]


def frame_programs(op):
    """the set of an opcode's frames: operand -> OP -> encode for every window, the twin Sample(result) -> encode for every window,
    and the index program (one set per opcode: what is compiled at run time stays a few seconds' work)"""
    progs = [Program([fetch(0) + (fetch(1) if op in L.BINARY else []) + [op] + encode(k)]) for k in SHIFTS]
    twins = [Program([fetch(2) + encode(k)]) for k in SHIFTS]
    return progs + twins + [Program([fetch(2) + ["SetColor"]])]


OP_PROGRAMS, TWIN_PROGRAMS, INDEX_PROGRAM = [0, 1, 2, 3], [4, 5, 6, 7], 8


def frame_scene(api, op, shaders, patterns):
    scene = api.Scene.empty()
    for p in frame_programs(op):
        scene.add_program(p)
    for k, idx in enumerate(shaders):
        r = api.Batch2D.from_rectangle(float((k % 2) * (FW // 2)), float((k // 2) * (FH // 2)), float(FW // 2), float(FH // 2))
        r.source(B.PixelSource.Pixel((255, 255, 255, 255))).shader(idx)
        scene.add_d2_static(r)
    assets = api.Assets.default().patterns(patterns)

    def setup():
        return api.Rasterizer.setup(None, B.Mat4.identity(), B.Mat4.identity())

    return scenes._result(api, scene, assets, setup, FW, FH, 40, "libm-frame")


def index_pattern():
    p = np.zeros((H, W, 3), np.float32)
    p[..., 0] = (np.arange(W, dtype=np.float32) / np.float32(255.0))[None, :]     # byte x
    p[..., 1] = (np.arange(H, dtype=np.float32) / np.float32(255.0))[:, None]     # byte y
    p[..., 2] = 1.0
    return p


_TEXEL = {}


def texel_of_pixel(oracle):
    """[FH][FW][2] (x, y) of the pattern texel each frame pixel samples, from the ORACLE's frame of the index program"""
    if "map" not in _TEXEL:
        zero = np.zeros((H, W, 3), np.float32)
        frame = scenes.render(frame_scene(oracle, "Sin", [INDEX_PROGRAM] * 4, [zero, zero, index_pattern()]))
        assert (frame[..., 2] == 255).all() and (frame[..., 3] == 255).all(), "the four rectangles do not cover the frame"
        _TEXEL["map"] = frame[..., :2].astype(np.int64).copy()
    return _TEXEL["map"]


def test_every_pattern_texel_is_drawn_by_some_pixel_of_every_rectangle(oracle, product):
    t = texel_of_pixel(oracle)
    assert t[..., 0].max() == W - 1 and t[..., 1].max() == H - 1
    for k in range(4):
        part = t[(k // 2) * (FH // 2):(k // 2 + 1) * (FH // 2), (k % 2) * (FW // 2):(k % 2 + 1) * (FW // 2)]
        seen = np.zeros((H, W), bool)
        seen[part[..., 1], part[..., 0]] = True
        assert seen.all(), f"rectangle {k}: {int((~seen).sum())} pattern texels are drawn by no pixel"
    zero = np.zeros((H, W, 3), np.float32)
    got = scenes.render(frame_scene(product, "Sin", [INDEX_PROGRAM] * 4, [zero, zero, index_pattern()]))
    assert np.array_equal(got[..., :2], t)           # the device samples the same texels


@pytest.mark.parametrize("op", L.OPS)
def test_frame_paths_compute_the_floats_of_the_bake(oracle, product, monkeypatch, op):
    """interpreted, compiled and the libm-free twin of the bake's result: the same bytes in all four windows, on every pixel whose
    operand has its result's last bit inside them (2^-8 <= |r| < 256)"""
    s = L.operand_set(op)
    result = np.array(device_results(product, op))
    seen = L.in_window(result) & L.used(op)
    assert seen.sum() >= 0.5 * L.used(op).sum(), (op, int(seen.sum()))
    t = texel_of_pixel(oracle)
    mask = seen[t[..., 1], t[..., 0]]                                      # [FH][FW][3]: the channels compared
    patterns = [s.a, s.b if s.b is not None else s.a, result]
    build = lambda api, shaders: frame_scene(api, op, shaders, patterns)   # noqa: E731
    monkeypatch.setenv("RXR_SHADER_JIT", "0")
    interp = scenes.render(build(product, OP_PROGRAMS)).copy()
    assert jit_info(product) == ""
    twin = scenes.render(build(product, TWIN_PROGRAMS)).copy()
    monkeypatch.setenv("RXR_SHADER_JIT", "1")
    compiled = scenes.render(build(product, OP_PROGRAMS)).copy()
    info = jit_info(product)
    monkeypatch.setenv("RXR_SHADER_JIT", "0")
    assert info.startswith("compiled:"), info
    for name, frame in (("interpreted", interp), ("compiled", compiled)):
        differ = (frame[..., :3] != twin[..., :3]) & mask
        assert not differ.any(), (f"{op}: the {name} frame shows other floats than the bake in {int(differ.sum())} channels; first at "
                                  f"(y, x, c) {np.argwhere(differ)[:3].tolist()}")
    assert np.array_equal(interp, compiled), f"{op}: compiled and interpreted frames differ in {int((interp != compiled).any(axis=2).sum())} pixels"
    assert len(np.unique(twin[..., :3][mask])) > 100, "the windows show nothing"
