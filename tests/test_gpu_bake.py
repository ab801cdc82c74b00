"""The shader-texture bake on the device (rxr_bake_shaders / rxr_bake_shaders_to, Rusteria::shade + RenderBuffer::as_rgba_bytes)
against the reference of tests/bake_ref.py: float buffers bit for bit for programs of exactly rounded operations, bytes exact
outside the boundary band of the gamma curve, the mirror's baking Chunk::add_shader end to end, and the error paths."""
import ctypes as C

import numpy as np
import pytest

import rusterix_amd
from rusterix_amd import binding as B
from rusterix_amd import scenes
from rusterix_amd.binding import Program
from rusterix_amd.abi import RXR_ERR_INVALID, RXR_ERR_UNSUPPORTED, RXR_OK
from tests import bake_ref as R
from tests.bake_ref import P

pytestmark = pytest.mark.gpu

TOLERANCE = 1    # bytes of programs that use sin / cos / pow / atan2 / ln (the project's tolerance for these opcodes)


def scene_of(api, programs):
    scene = api.Scene.empty()
    for p in programs:
        scene.add_program(p)
    return scene, R.make_assets(api)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def context_of(product):
    return C.c_void_p(product.lib.rxh_context())


def last_error(rxr, ctx):
    return (rxr.rxr_last_error(ctx) or b"").decode()


@pytest.mark.parametrize("which", ["static", "dynamic"])
def test_float_buffer_bit_for_bit_and_bytes(oracle, product, which):
    """several programs in one call, one of them twice, at every size; `static`: a set whose stack depths are static (k_bake_s),
    `dynamic`: with calls and PaletteIndex (k_bake)"""
    progs = R.exact_programs()
    names = R.STATIC_SET if which == "static" else list(progs)
    scene, assets = scene_of(product, [progs[n] for n in names])
    ref = R.Reference(oracle, [progs[n] for n in names])
    order = list(range(len(names))) + [1, 0]           # (the same program twice)
    flips = bands = 0
    for (w, h) in R.SIZES:
        got = scene.bake_shaders(order, w, h, assets=assets)
        assert got["pixels"].shape == (len(order), h, w, 4) and got["rgba"].shape == (len(order), h, w, 4)
        for j, p in enumerate(order):
            want = ref.pixels(p, w, h)
            label = f"{names[p]} {w}x{h} (bake {j})"
            assert (got["pixels"][j][..., 3] == 1.0).all(), label
            same = bits(got["pixels"][j]) == bits(want)
            assert same.all(), f"{label}: {int((~same).sum())} floats differ; first at {np.argwhere(~same)[:3].tolist()}"
            f, b = R.check_bytes(got["rgba"][j], want, label)
            flips += f
            bands += b
    print(f"{which}: {flips} bytes differ by one inside the boundary band ({bands} channels in the band)")
    # one output alone
    only = scene.bake_shaders([0], 5, 3, assets=assets, pixels=False)
    assert set(only) == {"rgba"} and np.array_equal(only["rgba"], scene.bake_shaders([0], 5, 3, assets=assets)["rgba"])


def test_special_values_follow_the_cast_rules(oracle, product):
    """c <= 0, c == 1, c > 1, +-inf, NaN and -0.0: exactly 0 or 255"""
    sp = R.special_programs()
    scene, assets = scene_of(product, list(sp.values()))
    ref = R.Reference(oracle, list(sp.values()))
    got = scene.bake_shaders(list(range(len(sp))), 64, 64, assets=assets)
    for i, n in enumerate(sp):
        want = ref.pixels(i, 64, 64)
        R.check_bytes(got["rgba"][i], want, n)
        c = want[..., :3]
        decided = ~(c > 0) | (c >= 1) | ~np.isfinite(c)
        assert decided.any(), n
        assert np.isin(got["rgba"][i][..., :3][decided], (0, 255)).all(), n
        assert np.array_equal(got["rgba"][i][..., :3][decided], R.expected_bytes(want)[..., :3][decided]), n
        assert not np.signbit(got["pixels"][i][got["pixels"][i] == 0]).any(), f"{n}: -0.0 in the float buffer"
        finite = np.isfinite(want)
        assert np.array_equal(bits(got["pixels"][i])[finite], bits(want)[finite]) and np.array_equal(np.isnan(got["pixels"][i]), np.isnan(want)), n


def test_transcendental_programs_within_one_byte(oracle, product):
    lm = R.libm_programs()
    scene, assets = scene_of(product, list(lm.values()))
    ref = R.Reference(oracle, list(lm.values()))
    for (w, h) in [(64, 64), (63, 65)]:
        got = scene.bake_shaders(list(range(len(lm))), w, h, assets=assets)
        for i, n in enumerate(lm):
            want = R.expected_bytes(ref.pixels(i, w, h))
            diff = np.abs(got["rgba"][i].astype(np.int16) - want.astype(np.int16))
            assert int(diff.max()) <= TOLERANCE, f"{n} {w}x{h}: {(diff > TOLERANCE).sum()} channels differ by more than {TOLERANCE} (max {diff.max()})"
            assert (got["rgba"][i][..., 3] == 255).all()
            assert len(np.unique(got["rgba"][i].reshape(-1, 4), axis=0)) > 100, n


# ---- the mirror's Chunk::add_shader, end to end ------------------------------------------------------------------------------------
W, H = 208, 144
CHECKER = Program([["UV", ("Push", 4.0), "Mul", "Fract", ("Push", 0.5), "Step", ("Push", 0.6), "Mul", "UV", ("Push", 0.4), "Mul", "Add", "SetColor"]])


def baked_chunk_scene(api, texture):
    """an unlit chunk box whose shader has a baked texture (sampled in the opaque pass, src/rasterizer.rs:1226-1267); `texture`:
    a Texture / None given to add_shader, or "bake": baked on the device"""
    scene = api.Scene.empty()
    scene.add_program(Program([[("Push", 0.0, 0.0, 1.0), "SetColor"]]))
    chunk = scene.add_chunk()
    assets = api.Assets.default().textures([B.Tile.from_texture(scenes.noise_texture(8, 32, 32))])
    s0 = chunk.add_shader(CHECKER, bake=True, assets=assets) if texture == "bake" else chunk.add_shader(CHECKER, texture)
    none = chunk.add_shader(Program([[("Push", 0.5), "SetColor"]], shade_index=None), bake=True, assets=assets) if texture == "bake" else None
    box = api.Batch3D.from_box(-0.5, -0.5, -0.5, 1.0, 1.0, 1.0).cull_mode(B.CULL_OFF).with_computed_normals()
    box.source(B.PixelSource.StaticTileIndex(0)).repeat_mode(B.REPEAT_REPEAT_XY).shader(s0)
    chunk.add_batch3d(box)
    cam = api.D3OrbitCamera.new()
    cam.set_parameter_f32("distance", 2.4)
    cam.azimuth = 1.2
    cam.elevation = 0.5

    def setup():
        v, p = cam.matrices(float(W), float(H))
        return api.Rasterizer.setup(None, v, p).ambient((1.0, 1.0, 1.0, 1.0))

    return scenes._result(api, scene, assets, setup, W, H, 40, "baked-chunk", chunk=chunk, s0=s0, none=none)


def test_add_shader_with_bake_end_to_end(oracle, product):
    cfg = baked_chunk_scene(product, "bake")
    tex = cfg.chunk.shader_texture(cfg.s0)
    assert tex is not None and (tex.width, tex.height) == (64, 64)
    assert cfg.chunk.shader_texture(cfg.none) is None            # a program without `shade`: None, nothing baked
    want = R.Reference(oracle, [CHECKER]).pixels(0, 64, 64)
    R.check_bytes(tex.data.reshape(64, 64, 4), want, "add_shader(bake=True)")
    got = scenes.render(cfg).copy()
    ref = scenes.render(baked_chunk_scene(oracle, tex))          # the oracle scene with the device's bytes
    assert np.array_equal(got, ref), f"{(got != ref).any(axis=2).sum()} pixels differ from the oracle"
    host = scenes.render(baked_chunk_scene(product, tex))        # the same bytes supplied by the host
    assert np.array_equal(got, host)
    plain = scenes.render(baked_chunk_scene(product, None))
    assert (got != plain).any(axis=2).mean() > 0.02, "the baked texture should show on the box"


def test_add_shader_with_bake_refuses_what_the_device_cannot_bake(product):
    scene = product.Scene.empty()
    chunk = scene.add_chunk()
    with pytest.raises(B.RasterizeError) as e:
        chunk.add_shader(P(["Normal", "SetColor", ("Push", 0.0, 1.0, 0.0), "SetNormal"]), bake=True)
    assert e.value.code == RXR_ERR_UNSUPPORTED and "normal" in str(e.value)
    assert chunk.add_shader(P(["UV", "SetColor"]), bake=True) == 0            # nothing was added by the refused call
    assert chunk.shader_texture(0) is not None


# ---- the ABI directly ----------------------------------------------------------------------------------------------------------------
def resident(product, programs):
    """makes `programs` the process context's resident set (through one mirror bake); returns (rxr, ctx)"""
    scene, assets = scene_of(product, programs)
    scene.bake_shaders([0], 1, 1, assets=assets)
    return rusterix_amd.rxr_abi(), context_of(product)


def test_to_form_on_another_stream_equals_the_host_form(product):
    import torch

    progs = R.exact_programs()
    rxr, ctx = resident(product, list(progs.values()))
    order = np.array([3, 0, 5, 3], np.uint32)
    w, h = 63, 65
    host_px, host_b = np.zeros((4, h, w, 4), np.float32), np.zeros((4, h, w, 4), np.uint8)
    assert rxr.rxr_bake_shaders(ctx, order.ctypes.data, 4, w, h, host_px.ctypes.data, host_b.ctypes.data) == RXR_OK, last_error(rxr, ctx)
    stream = torch.cuda.Stream()
    px = torch.zeros((4, h, w, 4), dtype=torch.float32, device="cuda")
    by = torch.zeros((4, h, w, 4), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    sp = C.c_void_p(stream.cuda_stream)
    assert rxr.rxr_bake_shaders_to(ctx, order.ctypes.data, 4, w, h, px.data_ptr(), by.data_ptr(), sp) == RXR_OK, last_error(rxr, ctx)
    order[:] = 0   # (the list was read before the call returned)
    assert rxr.rxr_bake_shaders_to(ctx, order.ctypes.data, 1, w, h, None, by.data_ptr() + 0, sp) == RXR_OK    # bytes alone, queued behind
    assert rxr.rxr_synchronize(ctx) == RXR_OK, last_error(rxr, ctx)
    stream.synchronize()
    assert np.array_equal(bits(px.cpu().numpy()), bits(host_px))
    got_b = by.cpu().numpy()
    assert np.array_equal(got_b[1:], host_b[1:]) and np.array_equal(got_b[0], host_b[1])   # (the second call baked program 0 into slot 0)
    # arguments: host memory where device memory is expected, a misaligned pointer, sizes (a tensor is a slice of the framework's pool:
    # whether an array is large enough is not something the library can see)
    assert rxr.rxr_bake_shaders_to(ctx, order.ctypes.data, 1, w, h, host_px.ctypes.data, None, sp) == RXR_ERR_INVALID
    assert rxr.rxr_bake_shaders_to(ctx, order.ctypes.data, 1, w, h, px.data_ptr() + 4, None, sp) == RXR_ERR_INVALID
    for (ww, hh) in [(0, 4), (4, 0), (16385, 1), (1, 16385)]:
        assert rxr.rxr_bake_shaders(ctx, order.ctypes.data, 1, ww, hh, host_px.ctypes.data, None) == RXR_ERR_INVALID, (ww, hh)
    assert rxr.rxr_bake_shaders(ctx, order.ctypes.data, 4, 16384, 16384, host_px.ctypes.data, None) == RXR_ERR_INVALID   # 2^30 texels
    assert rxr.rxr_bake_shaders(ctx, None, 1, 4, 4, host_px.ctypes.data, None) == RXR_ERR_INVALID
    assert rxr.rxr_bake_shaders(ctx, None, 0, 4, 4, None, None) == RXR_OK
    assert rxr.rxr_synchronize(ctx) == RXR_OK


def test_a_bake_between_upload_and_render_leaves_the_frame_alone(product):
    lib, rxr = product.lib, rusterix_amd.rxr_abi()
    cfg = baked_chunk_scene(product, None)
    want = scenes.render(cfg).copy()
    r = cfg.setup()
    assert lib.rxh_rasterizer_upload(r._h, cfg.scene._h, cfg.width, cfg.height, cfg.tile_size, cfg.assets._h) == 0
    ctx = context_of(product)
    order = np.array([1, 0, 1], np.uint32)     # the resident set: scene.shaders[0], then the chunk's CHECKER
    out = np.zeros((3, 64, 64, 4), np.uint8)
    assert rxr.rxr_bake_shaders(ctx, order.ctypes.data, 3, 64, 64, None, out.ctypes.data) == RXR_OK, last_error(rxr, ctx)
    assert (out[1][..., :3] == (0, 0, 255)).all() and len(np.unique(out[0].reshape(-1, 4), axis=0)) > 50
    got = np.zeros((cfg.height, cfg.width, 4), np.uint8)
    assert rxr.rxr_render_download(ctx, got.ctypes.data) == RXR_OK, last_error(rxr, ctx)
    assert np.array_equal(got, want)


def test_a_bake_is_the_same_before_and_after_the_set_is_compiled(oracle, product, monkeypatch):
    from tests.test_gpu_shader_jit import grid_scene, jit_info

    progs = R.exact_programs()
    programs = [progs[n] for n in R.STATIC_SET]
    monkeypatch.setenv("RXR_SHADER_JIT", "1")          # compiled when a frame first needs it
    cfg = grid_scene(product, programs)
    order = list(range(len(programs)))
    before = cfg.scene.bake_shaders(order, 64, 64, assets=cfg.assets)
    frame = scenes.render(cfg).copy()
    assert jit_info(product).startswith("compiled:"), jit_info(product)
    after = cfg.scene.bake_shaders(order, 64, 64, assets=cfg.assets)
    assert np.array_equal(bits(before["pixels"]), bits(after["pixels"])) and np.array_equal(before["rgba"], after["rgba"])
    assert jit_info(product).startswith("compiled:")   # the bake left the compiled set in place ...
    assert np.array_equal(scenes.render(cfg), frame)   # ... and the frames it renders
    monkeypatch.setenv("RXR_SHADER_JIT", "0")


# ---- errors ------------------------------------------------------------------------------------------------------------------------
def frame_still_renders(oracle, product):
    got = scenes.render(scenes.cube_scene(product, width=160, height=96, tile_size=40, textured=True, logo_size=64))
    ref = scenes.render(scenes.cube_scene(oracle, width=160, height=96, tile_size=40, textured=True, logo_size=64))
    assert int(np.abs(got.astype(np.int16) - ref.astype(np.int16)).max()) <= 1


def test_errors_leave_the_context_usable(oracle, product):
    rxr = rusterix_amd.rxr_abi()
    out = np.zeros((1, 4, 4, 4), np.float32)
    zero = np.zeros(1, np.uint32)
    # no shader set
    empty = product.Scene.empty()
    frame_still_renders(oracle, product)      # (a frame without programs: the context's set is empty)
    ctx = context_of(product)
    assert rxr.rxr_set_shaders(ctx, None) == RXR_OK
    assert rxr.rxr_bake_shaders(ctx, zero.ctypes.data, 1, 4, 4, out.ctypes.data, None) == RXR_ERR_INVALID and "no shader set" in last_error(rxr, ctx)
    with pytest.raises(B.RasterizeError) as e:
        empty.bake_shaders([0], 4, 4)
    assert e.value.code == RXR_ERR_INVALID
    frame_still_renders(oracle, product)
    # an unsupported program, a program without shade, an index outside the set
    bad = P(["Normal", "SetColor", ("Push", 0.0, 1.0, 0.0), "SetNormal"])
    scene, assets = scene_of(product, [P(["UV", "SetColor"]), bad, Program([[("Push", 0.5), "SetColor"]], shade_index=None)])
    for index, code in ((1, RXR_ERR_UNSUPPORTED), (2, RXR_ERR_INVALID), (3, RXR_ERR_INVALID)):
        with pytest.raises(B.RasterizeError) as e:
            scene.bake_shaders([0, index], 4, 4, assets=assets)
        assert e.value.code == code and f"programs[1] = {index}" in str(e.value), str(e.value)
    assert scene.bake_shaders([0], 4, 4, assets=assets)["pixels"][0, 0, 0].tolist() == [0.0, 1.0, 0.0, 1.0]
    frame_still_renders(oracle, product)


@pytest.mark.parametrize("kind", ["underflow", "steps"])
def test_a_faulting_program_is_reported_with_its_texel(oracle, product, kind):
    """ordinary VM faults, reported through the status path: a stack underflow where the reference panics, and the interpreter's
    bound on backward jumps for a loop that never ends"""
    if kind == "underflow":   # only texels right of the middle take the branch that pops an empty stack
        prog = P(["UV", ("GetComponents", [0]), ("Push", 0.5), "Ge", ("If", ["Add"], None), "UV", "SetColor"])
        what, first_x = "stack underflow", 4
    else:
        prog = P([("For", [], [("Push", 1.0)], [], []), "UV", "SetColor"])
        what, first_x = "instruction limit", 0
    rxr, ctx = resident(product, [P(["UV", "SetColor"]), prog])
    order = np.array([0, 1], np.uint32)
    out = np.zeros((2, 1, 8, 4), np.float32)
    assert rxr.rxr_bake_shaders(ctx, order.ctypes.data, 2, 8, 1, out.ctypes.data, None) == RXR_ERR_INVALID
    msg = last_error(rxr, ctx)
    assert what in msg and "program 1" in msg and "texel (" in msg, msg
    if kind == "underflow":
        x = int(msg.split("texel (")[1].split(",")[0])
        assert x >= first_x, msg
    # the queued form reports at the next rxr_synchronize, once
    import torch

    px = torch.zeros((2, 1, 8, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    assert rxr.rxr_bake_shaders_to(ctx, order.ctypes.data, 2, 8, 1, px.data_ptr(), None, None) == RXR_OK
    assert rxr.rxr_synchronize(ctx) == RXR_ERR_INVALID and what in last_error(rxr, ctx)
    assert rxr.rxr_synchronize(ctx) == RXR_OK
    # the good program's bake of the same call is complete, and the context goes on
    assert np.array_equal(px.cpu().numpy()[0], out[0]) and out[0][0, 2].tolist() == [0.25, 1.0, 0.0, 1.0]
    assert rxr.rxr_bake_shaders(ctx, order.ctypes.data, 1, 8, 1, out.ctypes.data, None) == RXR_OK
    frame_still_renders(oracle, product)


def test_to_form_on_a_multi_device_handle_is_unsupported(product):
    rxr = rusterix_amd.rxr_abi()
    multi = C.c_void_p()
    devs = (C.c_int * 2)(0, 0)
    assert rxr.rxr_create_multi(C.byref(multi), devs, 2) == RXR_OK
    try:
        zero = np.zeros(1, np.uint32)
        assert rxr.rxr_bake_shaders_to(multi, zero.ctypes.data, 1, 4, 4, None, None, None) == RXR_ERR_UNSUPPORTED
        assert "multi-device" in last_error(rxr, multi)
        # the host form runs on member 0 (which holds no set here)
        out = np.zeros((1, 4, 4, 4), np.float32)
        assert rxr.rxr_bake_shaders(multi, zero.ctypes.data, 1, 4, 4, out.ctypes.data, None) == RXR_ERR_INVALID
        assert "no shader set" in last_error(rxr, multi)
    finally:
        rxr.rxr_destroy(multi)
