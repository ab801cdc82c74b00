"""The terrain bake on the device (rxr_set_terrain / rxr_bake_terrain / rxr_bake_terrain_to, Terrain::bake_chunk) against the numpy
restatement of tests/terrain_ref.py: every byte equal, no tolerance.  Shapes are the smallest at which the kernel can go wrong: a
wave owns an 8 x 8 texel block inside one tile cell, so pixels-per-tile of 1, 3, 5 (partial blocks), 8 (one block) and 16 (four),
mixed and uniform blend modes, chunks without cells, coordinates where floor(tile) leaves the cell (the per-lane path), batching
past the 64 chunks one launch carries, and launches split by work."""
import ctypes as C

import numpy as np
import pytest

import rusterix_amd
from rusterix_amd import binding as B
from rusterix_amd import scenes
from tests import terrain_ref as R
from tests.terrain_ref import NONE, OFFSET, RADIUS, RXR_ERR_INVALID, RXR_ERR_UNSUPPORTED, RXR_OK, TerrainSpec

pytestmark = pytest.mark.gpu


def context_of(product):
    return C.c_void_p(product.lib.rxh_context())


def last_error(rxr, ctx):
    return (rxr.rxr_last_error(ctx) or b"").decode()


def set_terrain(rxr, ctx, spec):
    keep, args = spec.arrays()
    return rxr.rxr_set_terrain(ctx, *args)


def bake(rxr, ctx, spec, coords, ppt):
    cc = np.ascontiguousarray(np.asarray(coords, np.int32).reshape(-1, 2))
    side = spec.chunk_size * ppt
    out = np.zeros((len(cc), side, side, 4), np.uint8)
    assert rxr.rxr_bake_terrain(ctx, cc.ctypes.data, len(cc), ppt, out.ctypes.data) == RXR_OK, last_error(rxr, ctx)
    return out


def expect(got, spec, coords, ppt, label=""):
    for i, coord in enumerate(coords):
        want = spec.bake(tuple(coord), ppt)
        assert np.array_equal(got[i], want), f"{label} chunk {tuple(coord)} ppt {ppt}: {R.first_difference(got[i], want)}"


@pytest.fixture(scope="module")
def base_refs():
    """the base scene's reference bakes, computed once"""
    out = {}
    for scale in [(1.0, 1.0), (0.75, 1.5)]:
        spec = R.base_scene(scale)
        out[scale] = (spec, np.stack([spec.bake(c, 8) for c in R.BASE_COORDS]))
    return out


# ---- through the mirror ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [(1.0, 1.0), (0.75, 1.5)])
def test_base_scene(product, base_refs, scale):
    spec, want = base_refs[scale]
    got = spec.product(product).bake_chunks(R.BASE_COORDS, 8)
    assert got.shape == want.shape
    for i, coord in enumerate(R.BASE_COORDS):
        assert np.array_equal(got[i], want[i]), f"scale {scale} chunk {coord}: {R.first_difference(got[i], want[i])}"
    assert len(np.unique(got[3].reshape(-1, 4), axis=0)) == 2          # the chunk without cells: the pure checker
    assert (got[1][..., 3] != 255).any() and len(np.unique(got[1].reshape(-1, 4), axis=0)) > 50


@pytest.mark.parametrize("chunk_size,ppt", [(3, 5), (4, 1), (5, 3)])
def test_sides_that_are_no_multiple_of_the_texel_block(product, chunk_size, ppt):
    spec = R.base_scene(chunk_size=chunk_size)
    coords = [(0, 0), (-1, -2)]
    expect(spec.product(product).bake_chunks(coords, ppt), spec, coords, ppt)


def test_one_larger_chunk(product):
    spec = R.uniform_scene(RADIUS, 2, chunk_size=16)
    expect(spec.product(product).bake_chunks([(0, 0)], 16), spec, [(0, 0)], 16)


def test_large_chunk_coordinates_take_the_per_lane_path(product):
    spec, coord = R.far_scene()
    t = spec.product(product)
    for ppt in (8, 5):
        expect(t.bake_chunks([coord], ppt), spec, [coord], ppt)


def test_the_plain_loop_and_the_separable_set_up_give_the_same_bytes(product, base_refs, monkeypatch):
    spec, want = base_refs[(0.75, 1.5)]
    t = spec.product(product)
    monkeypatch.setenv("RXR_TERRAIN_NAIVE", "1")
    got = t.bake_chunks(R.BASE_COORDS, 8)
    monkeypatch.delenv("RXR_TERRAIN_NAIVE")
    assert np.array_equal(got, want) and np.array_equal(t.bake_chunks(R.BASE_COORDS, 8), want)


def test_batching_and_launch_splitting(product, base_refs, monkeypatch):
    """five chunks in one call equal five calls; 70 chunks cross the 64 one launch carries; the same bake with the work bound lowered
    takes several launches and gives the same bytes"""
    spec, want = base_refs[(1.0, 1.0)]
    t = spec.product(product)
    rxr, ctx = rusterix_amd.rxr_abi(), context_of(product)
    coords = R.BASE_COORDS + [(-2, 1)]
    five = t.bake_chunks(coords, 8)
    assert rxr.rxr_debug_terrain_launches(ctx) == 1
    assert np.array_equal(five[:4], want)
    for i, c in enumerate(coords):
        assert np.array_equal(t.bake_chunks([c], 8)[0], five[i]), c
    many = [coords[i % 5] for i in range(70)]
    got = t.bake_chunks(many, 8)
    assert rxr.rxr_debug_terrain_launches(ctx) == 2
    for i in range(70):
        assert np.array_equal(got[i], five[i % 5]), i
    for bound in ("50000", "1"):       # a few launches; one wave per launch where a block's work exceeds the bound
        monkeypatch.setenv("RXR_TERRAIN_LAUNCH_TAPS", bound)
        split = t.bake_chunks(coords, 8)
        launches = rxr.rxr_debug_terrain_launches(ctx)
        assert launches >= 3 and (bound != "1" or launches == 5 * 16), (bound, launches)
        assert np.array_equal(split, five), bound
    monkeypatch.delenv("RXR_TERRAIN_LAUNCH_TAPS")
    assert np.array_equal(t.bake_chunks(coords, 8), five) and rxr.rxr_debug_terrain_launches(ctx) == 1


def test_steps_bound(product):
    """steps == 64 (16 641 taps a texel) is accepted and exact; 65 is refused"""
    spec = TerrainSpec((2.0, 2.0), 2)
    rng = np.random.default_rng(5)
    tex = spec.texture(R.random_texture(rng, 4, 4))
    for y in range(-40, 42):
        for x in range(-40, 42):
            if (x * 7 + y * 3) % 5:
                spec.source(x, y, tex)
    for y in range(2):
        for x in range(2):
            spec.blend(x, y, RADIUS, 64)
    expect(spec.product(product).bake_chunks([(0, 0)], 2), spec, [(0, 0)], 2)
    spec.blend(1, 1, RADIUS, 65)
    with pytest.raises(B.RasterizeError) as e:
        spec.product(product).bake_chunks([(0, 0)], 2)
    assert e.value.code == RXR_ERR_UNSUPPORTED and "RXR_TERRAIN_MAX_STEPS" in str(e.value)


@pytest.mark.parametrize("seed", range(50))
def test_fuzz(product, seed):
    spec, coord, ppt = R.fuzz_scene(seed)
    got = spec.product(product).bake_chunks([coord], ppt)[0]
    want = spec.bake(coord, ppt)
    assert np.array_equal(got, want), f"seed {seed} (scale {spec.scale}, chunk {coord}, ppt {ppt}): {R.first_difference(got, want)}"


# ---- the ABI directly -----------------------------------------------------------------------------------------------------------------
def test_to_form_on_another_stream_equals_the_blocking_call(product, base_refs):
    import torch

    spec, want = base_refs[(0.75, 1.5)]
    rxr, ctx = rusterix_amd.rxr_abi(), context_of(product)
    assert set_terrain(rxr, ctx, spec) == RXR_OK, last_error(rxr, ctx)
    host = bake(rxr, ctx, spec, R.BASE_COORDS, 8)
    assert np.array_equal(host, want)
    cc = np.array(R.BASE_COORDS, np.int32)
    stream = torch.cuda.Stream()
    dev = torch.zeros(want.shape, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    sp = C.c_void_p(stream.cuda_stream)
    assert rxr.rxr_bake_terrain_to(ctx, cc.ctypes.data, 4, 8, dev.data_ptr(), sp) == RXR_OK, last_error(rxr, ctx)
    cc[:] = 99       # (the coordinates were read before the call returned)
    assert rxr.rxr_synchronize(ctx) == RXR_OK, last_error(rxr, ctx)
    stream.synchronize()
    assert np.array_equal(dev.cpu().numpy(), want)
    cc[:] = R.BASE_COORDS
    # host memory where device memory is expected, a misaligned pointer, sizes, NULL
    assert rxr.rxr_bake_terrain_to(ctx, cc.ctypes.data, 4, 8, host.ctypes.data, sp) == RXR_ERR_INVALID and "device memory" in last_error(rxr, ctx)
    assert rxr.rxr_bake_terrain_to(ctx, cc.ctypes.data, 1, 8, dev.data_ptr() + 2, sp) == RXR_ERR_INVALID
    assert rxr.rxr_bake_terrain_to(ctx, cc.ctypes.data, 1, 8, None, sp) == RXR_ERR_INVALID
    for ppt in (0, -1, 4097):                       # 4 * 4097 > RXR_BAKE_MAX_DIM
        assert rxr.rxr_bake_terrain(ctx, cc.ctypes.data, 1, ppt, host.ctypes.data) == RXR_ERR_INVALID, ppt
    assert rxr.rxr_bake_terrain(ctx, cc.ctypes.data, 4, 4096, host.ctypes.data) == RXR_ERR_INVALID          # 2^30 texels
    assert rxr.rxr_bake_terrain(ctx, None, 1, 8, host.ctypes.data) == RXR_ERR_INVALID
    far = np.array([[2 ** 30, 0]], np.int32)
    assert rxr.rxr_bake_terrain(ctx, far.ctypes.data, 1, 8, host.ctypes.data) == RXR_ERR_INVALID and "i32" in last_error(rxr, ctx)
    assert rxr.rxr_bake_terrain(ctx, None, 0, 8, None) == RXR_OK
    assert rxr.rxr_synchronize(ctx) == RXR_OK
    assert np.array_equal(bake(rxr, ctx, spec, R.BASE_COORDS, 8), want)


def test_multi_device_handles(product):
    rxr = rusterix_amd.rxr_abi()
    multi = C.c_void_p()
    devs = (C.c_int * 2)(0, 0)
    assert rxr.rxr_create_multi(C.byref(multi), devs, 2) == RXR_OK
    try:
        zero = np.zeros((1, 2), np.int32)
        out = np.zeros((4, 4, 4), np.uint8)
        assert rxr.rxr_bake_terrain(multi, zero.ctypes.data, 1, 2, out.ctypes.data) == RXR_ERR_INVALID and "no terrain" in last_error(rxr, multi)
        spec = TerrainSpec((1.0, 1.0), 2).blend(0, 0, RADIUS, 1)
        assert set_terrain(rxr, multi, spec) == RXR_OK, last_error(rxr, multi)
        assert rxr.rxr_bake_terrain_to(multi, zero.ctypes.data, 1, 2, None, None) == RXR_ERR_UNSUPPORTED and "multi-device" in last_error(rxr, multi)
        assert rxr.rxr_bake_terrain(multi, zero.ctypes.data, 1, 2, out.ctypes.data) == RXR_OK, last_error(rxr, multi)       # member 0
        assert np.array_equal(out, spec.bake((0, 0), 2))
    finally:
        rxr.rxr_destroy(multi)


def test_re_registration_and_removal(product):
    rxr = rusterix_amd.rxr_abi()
    ctx = C.c_void_p()
    assert rxr.rxr_create(C.byref(ctx), 0) == RXR_OK
    try:
        coords = [(0, 0), (-1, -1)]
        cc = np.array(coords, np.int32)
        out = np.zeros((2, 12, 12, 4), np.uint8)
        assert rxr.rxr_bake_terrain(ctx, cc.ctypes.data, 2, 4, out.ctypes.data) == RXR_ERR_INVALID and "no terrain" in last_error(rxr, ctx)
        first, second = R.base_scene(chunk_size=3, seed=1), R.base_scene((0.5, 2.0), chunk_size=3, seed=2)
        assert set_terrain(rxr, ctx, first) == RXR_OK, last_error(rxr, ctx)
        expect(bake(rxr, ctx, first, coords, 4), first, coords, 4, "first")
        assert set_terrain(rxr, ctx, second) == RXR_OK, last_error(rxr, ctx)
        expect(bake(rxr, ctx, second, coords, 4), second, coords, 4, "second")
        # a refused call leaves the resident terrain as it was
        assert set_terrain(rxr, ctx, TerrainSpec((0.0, 1.0), 3)) == RXR_ERR_INVALID and "scale" in last_error(rxr, ctx)
        expect(bake(rxr, ctx, second, coords, 4), second, coords, 4, "after a refused call")
        # n_cells == 0 removes it: the pure checker, with the new scale and chunk size
        empty = TerrainSpec((1.0, 1.0), 3)
        assert set_terrain(rxr, ctx, empty) == RXR_OK
        got = bake(rxr, ctx, empty, coords, 4)
        expect(got, empty, coords, 4, "empty")
        assert set(np.unique(got[..., :3]).tolist()) == {120, 135} and (got[..., 3] == 255).all()
        # a coordinate given twice: the later entry wins
        keep, args = first.arrays()
        n = len(keep["tex"])
        twice = {k: np.concatenate([keep[k], keep[k][:1]]) for k in ("xy", "tex", "blend", "off")}
        twice["tex"][n] = -1
        twice["blend"][n] = RADIUS | 3 << 8
        assert rxr.rxr_set_terrain(ctx, args[0], args[1], twice["xy"].ctypes.data, twice["tex"].ctypes.data, twice["blend"].ctypes.data,
                                   twice["off"].ctypes.data, n + 1, args[7], args[8]) == RXR_OK, last_error(rxr, ctx)
        x, y = (int(v) for v in keep["xy"][0])
        first.source(x, y, None).blend(x, y, RADIUS, 3)
        around = [(x // 3, y // 3)]
        expect(bake(rxr, ctx, first, around, 4), first, around, 4, "later entry")
    finally:
        rxr.rxr_destroy(ctx)


# ---- frames ----------------------------------------------------------------------------------------------------------------------------
W, H = 208, 144


def terrain_frame(api, texture, origin, size):
    """an unlit floor quad over one chunk that samples chunk.terrain_texture by world position (src/chunk.rs:133-151)"""
    from tests.test_gpu_chunks import floor_quad

    scene = api.Scene.empty()
    chunk = scene.add_chunk()
    chunk.terrain(texture, origin=origin, size=size)
    chunk.terrain_batch3d(floor_quad(api, 0.0, 0.0, 8.0, 8.0).source(B.PixelSource.Terrain()))
    cam = api.D3OrbitCamera.new()
    cam.set_parameter_f32("distance", 9.0)
    cam.center = (4.0, 0.0, 4.0)
    cam.azimuth, cam.elevation = 0.9, 0.8

    def setup():
        v, p = cam.matrices(float(W), float(H))
        return api.Rasterizer.setup(None, v, p).ambient((1.0, 1.0, 1.0, 1.0))

    return scenes._result(api, scene, api.Assets.default(), setup, W, H, 40, "terrain-frame", chunk=chunk)


def test_frames(oracle, product):
    """a frame uploaded before a bake renders the same bytes after it; a chunk whose terrain_texture came from build_chunk_at on the
    device renders the same frame as one given the reference's texture"""
    spec = R.uniform_scene(RADIUS, 1, chunk_size=8, seed=9)
    for (x, y) in [(1, 1), (5, 2), (3, 6)]:
        spec.blend(x, y, NONE)
    want_tex = spec.bake((0, 0), 8)
    given = B.Texture(want_tex.reshape(-1).copy(), 64, 64)
    ref_frame = scenes.render(terrain_frame(product, given, (0, 0), 8)).copy()
    assert len(np.unique(ref_frame.reshape(-1, 4), axis=0)) > 200, "the terrain texture should be visible"
    assert np.array_equal(ref_frame, scenes.render(terrain_frame(oracle, given, (0, 0), 8)))
    # build_chunk_at on the device
    cfg = terrain_frame(product, None, (0, 0), 8)
    t = spec.product(product)
    assert cfg.chunk.terrain_texture() is None
    t.build_chunk_at((3, 3), 8, cfg.chunk)             # the terrain has no chunk there: nothing is set, as in the reference
    assert cfg.chunk.terrain_texture() is None
    t.build_chunk_at((0, 0), 8, cfg.chunk)
    tex = cfg.chunk.terrain_texture()
    assert (tex.width, tex.height) == (64, 64) and np.array_equal(np.asarray(tex.data).reshape(64, 64, 4), want_tex)
    assert np.array_equal(scenes.render(cfg), ref_frame)
    # a bake between upload and render
    lib, rxr = product.lib, rusterix_amd.rxr_abi()
    r = cfg.setup()
    assert lib.rxh_rasterizer_upload(r._h, cfg.scene._h, cfg.width, cfg.height, cfg.tile_size, cfg.assets._h) == 0
    assert np.array_equal(t.bake_chunks([(0, 0), (1, 0)], 8)[0], want_tex)
    got = np.zeros((H, W, 4), np.uint8)
    ctx = context_of(product)
    assert rxr.rxr_render_download(ctx, got.ctypes.data) == RXR_OK, last_error(rxr, ctx)
    assert np.array_equal(got, ref_frame)
