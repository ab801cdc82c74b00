"""Small host-projected frames carry their set-up records in the frame blob (rxr_upload_frame, rusterix_amd/csrc/rxr_upload.hip): the
TriSetup / TriShade records are built on the host by the function that defines them (rxr_tri_records, rxr_device.h) and a render whose
row band lies on tile rows launches no k_setup3d.

  (a) records, byte for byte: rxr_debug_setup_records hands back the host-made records and what k_setup3d writes for the whole-frame band
      (into zeroed scratch); all n x 96 and n x 80 bytes must be equal, a NaN counting as equal to a NaN (differing_words);
  (b) frames, byte for byte: RXR_HOST_SETUP=1 against 0 (read by rxr_create: a context of its own per setting), both light modes, whole
      frames, stripes, bands on and off tile rows, several uploads, member contexts; rxr_debug_last_setup_route proves the route.

What of a record can change between an upload and a render: nothing.  Every input -- arrays, batch headers, the descriptor table (a copy of
the resident textures' descriptors made at upload, chunk textures included), the clip rectangles, sample_mode, the frame size -- lives in
the frame blob or in the parameter block that rxr_upload_frame fills, and neither is written again before the next upload
(rxr_update_chunk_textures writes texels, not the blob's descriptors; rxr_update_meshes concerns device-projected frames, which carry no
host records).  So there is no case here that changes an input after the upload; the cases that upload again are below.

The frames are small: 333 x 187 (the height is no multiple of the 16-pixel tile) and 171 x 107."""
import ctypes as C

import numpy as np
import pytest

import rusterix_amd
from rusterix_amd import binding as B
from rusterix_amd import scenes
from tests.test_gpu_routes import knobs
from tests.test_gpu_special_inputs import build as special_build
from tests.test_gpu_special_inputs import build_random as special_random

pytestmark = pytest.mark.gpu

STAGE_TRIS = 128                     # RXR_STAGE_TRIS (rxr_device.h)
NOTHING, HOST_RECORDS, DEVICE_LAUNCH = 0, 1, 2   # rxr_debug_last_setup_route
SETUP_BYTES, SHADE_BYTES = 96, 80
BX_WORD, BY_WORD = 20, 21            # TriSetup.bx / .by, in 32-bit words


def ctx_of(product):
    return C.c_void_p(product.lib.rxh_context())


def upload(product, cfg):
    """the frame made resident on the host mirror's context; the Rasterizer is returned so that it outlives the renders"""
    r = cfg.setup()
    assert product.lib.rxh_rasterizer_upload(r._h, cfg.scene._h, cfg.width, cfg.height, cfg.tile_size, cfg.assets._h) == 0, product.lib.rxh_last_error()
    return r


def setup_route(product, ctx=None):
    return rusterix_amd.rxr_abi().rxr_debug_last_setup_route(ctx if ctx is not None else ctx_of(product))


def records(product, capacity=1024):
    """(has host records, n, host TriSetup, host TriShade, device TriSetup, device TriShade) of the resident frame, as uint32 words"""
    rxr = rusterix_amd.rxr_abi()
    bufs = [np.full(capacity * nbytes, 0xA5, np.uint8) for nbytes in (SETUP_BYTES, SHADE_BYTES, SETUP_BYTES, SHADE_BYTES)]
    n = C.c_uint32(0)
    rc = rxr.rxr_debug_setup_records(ctx_of(product), *[C.c_void_p(b.ctypes.data) for b in bufs], capacity, C.byref(n))
    assert rc in (0, 1), rxr.rxr_last_error(ctx_of(product))
    words = [b[:n.value * nbytes].view(np.uint32).reshape(n.value, nbytes // 4) for b, nbytes in zip(bufs, (SETUP_BYTES, SHADE_BYTES, SETUP_BYTES, SHADE_BYTES))]
    return (rc == 1, n.value, *words)


def differing_words(a, b, n_float):
    """(triangle, word) pairs in which two record arrays differ.  Words are compared by bit pattern; in the float fields (the first
    n_float words of a record) a NaN equals a NaN: which NaN an operation returns is the processor's choice, not the expression's -- x86
    answers an invalid operation with the negative quiet NaN and lets `a - NaN` keep the operand's sign, the device answers with the
    positive one and negates the operand of a subtraction -- and nothing reads a NaN's sign or payload: the records take part in
    float arithmetic and comparisons only (the Edges records of a frame handed over with them have always carried the host's NaNs)"""
    fa, fb = a[:, :n_float].view(np.float32), b[:, :n_float].view(np.float32)
    diff = a != b
    diff[:, :n_float] &= ~(np.isnan(fa) & np.isnan(fb))
    return np.argwhere(diff)


def assert_records_equal(product, what, expect_host=True):
    has, n, hs, hh, ds, dh = records(product)
    assert has == expect_host, f"{what}: host records {'missing' if expect_host else 'present'} ({n} triangles)"
    if has:
        for name, a, b, n_float in (("TriSetup", hs, ds, 19), ("TriShade", hh, dh, 18)):
            bad = differing_words(a, b, n_float)
            assert len(bad) == 0, f"{what}: {name} differs in {len(bad)} words; first (triangle, word) {bad[:4].tolist()}: host {[hex(a[tuple(i)]) for i in bad[:4]]} device {[hex(b[tuple(i)]) for i in bad[:4]]}"
    return n, hs if has else ds, hh if has else dh


# ---- (a) the records ---------------------------------------------------------------------------------------------------------------
SIZES = [(333, 187), (171, 107)]


@pytest.mark.parametrize("width,height", SIZES)
@pytest.mark.parametrize("sample_mode", [B.SAMPLE_NEAREST, B.SAMPLE_LINEAR])
@pytest.mark.parametrize("which", ["cube", "map"])
def test_records_of_the_cube_and_the_map(product, which, sample_mode, width, height):
    if which == "cube":
        cfg = scenes.cube_scene(product, width=width, height=height, tile_size=40, textured=True, distance=3.0, sample_mode=sample_mode, logo_size=32, rect_size=8.0)
    else:
        cfg = scenes.map_scene(product, width=width, height=height, n_lights=16, logo_size=16, sample_mode=sample_mode, rect_size=8.0)
    keep = upload(product, cfg)
    n, s, h = assert_records_equal(product, f"{which}, sample mode {sample_mode}, {width} x {height}")
    assert 0 < n <= STAGE_TRIS and (s[:, BY_WORD] != 0).any(), "no triangle of the scene has a pixel box"
    assert (h[:, 18:20] != 0).any(), "no record carries its texture descriptor"
    del keep


@pytest.mark.parametrize("cutout", [False, True])
@pytest.mark.parametrize("sample_mode", [B.SAMPLE_NEAREST, B.SAMPLE_LINEAR])
def test_records_of_poisoned_triangles(product, sample_mode, cutout):
    """NaN, +-inf, +-0, a denormal and the largest floats in a position or a texture coordinate of one triangle after the other
    (tests/test_gpu_special_inputs.py).  Linear sampling: the NaN-uv rule sets DB_ALPHA_TEST in the record's copy of the batch flags"""
    keep = upload(product, special_build(product, sample_mode, B.REPEAT_REPEAT_XY, cutout))
    n, s, _ = assert_records_equal(product, f"poisoned triangles, sample mode {sample_mode}, cutout {cutout}")
    assert n >= 42   # (40 poisoned triangles and the backdrop; near-plane clipping may append fans)
    if sample_mode == B.SAMPLE_LINEAR and not cutout:
        assert ((s[:, 22] & 4) != 0).any(), "no triangle took the NaN-uv rule"   # (TriSetup.bflags & DB_ALPHA_TEST)
    del keep


@pytest.mark.parametrize("seed", range(8))
def test_records_of_seeded_scenes(product, seed):
    """the seeded generators: random poisoned numbers, cull modes, passes; the fuzz scenes.  (A projected w of exactly 0, 1 / w = inf, is
    built on purpose where projected vertices can be written directly: tests/abi_no_normals.c)"""
    keep = upload(product, special_random(product, seed))
    assert_records_equal(product, f"special-random seed {seed}")
    from tests.test_gpu_fuzz import build as fuzz_build

    keep = upload(product, fuzz_build(product, 200 + seed, 171, 107))
    n = records(product)[1]
    assert_records_equal(product, f"fuzz seed {200 + seed}", expect_host=0 < n <= STAGE_TRIS)
    del keep


def triangles_scene(api, n_tris, width=171, height=107, cull=B.CULL_OFF, source=None, textures=None, huge=None, tile_size=40):
    """n_tris small triangles in front of the camera, one batch (two from three triangles on, so that batch bases matter)"""
    rng = np.random.default_rng([0x52585231, 4242, n_tris])
    scene = api.Scene.empty()
    left = n_tris
    for part in ([n_tris] if n_tris < 3 else [n_tris // 2, n_tris - n_tris // 2]):
        centre = rng.uniform(-1.0, 1.0, size=(part, 1, 3)) * np.array([1.6, 1.0, 0.5])
        verts = (centre + rng.normal(0.0, 0.25, size=(part, 3, 3))).reshape(-1, 3).astype(np.float32)
        if huge is not None:
            verts[1, 0] = huge
        v4 = np.concatenate([verts, np.ones((len(verts), 1), np.float32)], axis=1)
        uv = rng.uniform(-0.5, 2.0, (part * 3, 2)).astype(np.float32)
        b = api.Batch3D.new(v4, np.arange(part * 3, dtype=np.uint32).reshape(part, 3), uv).with_computed_normals().cull_mode(cull)
        b.source(source if source is not None else B.PixelSource.StaticTileIndex(0)).repeat_mode(B.REPEAT_REPEAT_XY).ambient_color((0.9, 0.8, 0.7))
        scene.add_d3_static(b)
        left -= part
    assert left == 0
    assets = api.Assets.default().textures(textures or [B.Tile.from_texture(scenes.brick_texture(2))])
    cam = api.D3OrbitCamera.new()
    cam.set_parameter_f32("distance", 3.0)
    cam.azimuth = float(np.float32(np.pi / 2))

    def setup():
        v, p = cam.matrices(float(width), float(height))
        return api.Rasterizer.setup(None, v, p).sample_mode(B.SAMPLE_LINEAR).ambient((1.0, 1.0, 1.0, 1.0))

    return scenes._result(api, scene, assets, setup, width, height, tile_size, f"{n_tris} triangles")


@pytest.mark.parametrize("n_tris", [1, STAGE_TRIS, STAGE_TRIS + 1])
def test_records_at_the_triangle_limit(product, n_tris):
    keep = upload(product, triangles_scene(product, n_tris))
    n, s, _ = assert_records_equal(product, f"{n_tris} triangles", expect_host=n_tris <= STAGE_TRIS)   # 129: "no host records"
    assert n == n_tris and (s[:, BY_WORD] != 0).any()
    del keep


def test_records_of_a_frame_without_a_drawable_triangle(product):
    """every triangle culled (one of the two cull modes hides a triangle whichever way it faces) or its batch skipped (DB_SKIP: a constant texel whose alpha is not 255 is never written): the
    records are empty boxes in zeroed words on both sides"""
    all_empty = 0
    for cull in (B.CULL_BACK, B.CULL_FRONT):
        keep = upload(product, triangles_scene(product, 1, cull=cull))
        n, s, h = assert_records_equal(product, f"one triangle, cull mode {cull}")
        if not s.any() and not h.any():
            all_empty += 1
        del keep
    assert all_empty == 1, "one cull mode must hide the triangle and the other show it"
    keep = upload(product, triangles_scene(product, 7, source=B.PixelSource.Pixel((200, 100, 50, 128))))
    n, s, h = assert_records_equal(product, "batches that are skipped")
    assert n >= 7 and not s.any() and not h.any()
    del keep


@pytest.mark.parametrize("tile_size", [8, 40, 300])
@pytest.mark.parametrize("huge", [-1.0e30, 1.0e7])
def test_records_under_a_risky_batch_box(product, huge, tile_size):
    """a vertex far off to the side: the batch's box arithmetic cannot be trusted and the pixel boxes are clipped to the tiles the
    reference draws the batch in (RasterParams.batch_clip3d, tests/test_gpu_special_inputs.py)"""
    keep = upload(product, triangles_scene(product, 9, width=208, height=144, huge=huge, tile_size=tile_size))
    n, _, _ = assert_records_equal(product, f"huge coordinate {huge}, tile size {tile_size}")
    assert n >= 9   # (near-plane clipping may append fans)
    del keep


def test_records_with_and_without_edges_records(product):
    """ABI 5: the frame handed over with one `visible` word per triangle (the default; Edges::new runs where the records are made) and
    the same frame with the host's Edges records: the records agree with the device's either way, and with each other"""
    got = {}
    for form in (1, 0):
        product.lib.rxh_set_device_edges(form)
        try:
            for cull in (B.CULL_OFF, B.CULL_BACK, B.CULL_FRONT):
                keep = upload(product, triangles_scene(product, 31, cull=cull))
                got[form, cull] = assert_records_equal(product, f"edges form {form}, cull mode {cull}")
                del keep
        finally:
            product.lib.rxh_set_device_edges(1)
    for cull in (B.CULL_OFF, B.CULL_BACK, B.CULL_FRONT):
        assert not len(differing_words(got[1, cull][1], got[0, cull][1], 19)) and not len(differing_words(got[1, cull][2], got[0, cull][2], 18)), f"cull mode {cull}: the two forms differ"


def test_records_whose_descriptor_words_stay_zero(product):
    """a constant-pixel source and a texture wider than 8191 texels: the record's two spare words stay zero (the shading pass goes
    through the batch header); a texture of 8191 texels fills them"""
    keep = upload(product, triangles_scene(product, 5, source=B.PixelSource.Pixel((200, 100, 50, 255))))
    _, _, h = assert_records_equal(product, "constant pixel")
    assert h.any() and not h[:, 18:20].any()
    for w, filled in ((8192, False), (8191, True)):
        img = np.full((1, w, 4), 255, np.uint8)
        img[0, :, 0] = np.arange(w) % 251
        keep = upload(product, triangles_scene(product, 5, textures=[B.Tile([B.Texture(img.reshape(-1), w, 1)])]))
        _, _, h = assert_records_equal(product, f"texture {w} texels wide")
        assert h.any() and bool(h[:, 18:20].any()) == filled, f"texture {w} texels wide: descriptor words"
    del keep


# ---- (b) the frames ----------------------------------------------------------------------------------------------------------------
def render_all_ways(product, cfg):
    """the resident frame rendered whole, as the stripes of rank 1 of 3, as a band on tile rows and as one that is not; with the route
    each render took"""
    import torch

    rxr = rusterix_amd.rxr_abi()
    keep = upload(product, cfg)
    ctx = ctx_of(product)
    W, H = cfg.width, cfg.height
    out, routes = {}, {}

    def run(name, rows, call):
        buf = torch.full((rows, W, 4), 9, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        assert call(C.c_void_p(buf.data_ptr())) == 0, rxr.rxr_last_error(ctx)
        assert rxr.rxr_synchronize(ctx) == 0, rxr.rxr_last_error(ctx)
        out[name] = buf.cpu().numpy()
        routes[name] = setup_route(product)

    n_stripes = (H + 15) // 16
    run("whole", H, lambda p: rxr.rxr_render_rows_to(ctx, 0, H, p, None))
    run("stripes", len(range(1, n_stripes, 3)) * 16, lambda p: rxr.rxr_render_stripes_to(ctx, 1, 3, p, None))
    run("band on tile rows", 64, lambda p: rxr.rxr_render_rows_to(ctx, 32, 96, p, None))
    run("last rows", H - 48, lambda p: rxr.rxr_render_rows_to(ctx, 48, H, p, None))
    run("band off tile rows", 95, lambda p: rxr.rxr_render_rows_to(ctx, 5, 100, p, None))
    del keep
    return out, routes


def frame_scenes(api):
    return {
        "map": scenes.map_scene(api, width=333, height=187, n_lights=16, logo_size=16, rect_size=8.0),
        "cube": scenes.cube_scene(api, width=171, height=107, tile_size=40, textured=True, distance=3.0, sample_mode=B.SAMPLE_LINEAR, logo_size=32, rect_size=8.0),
        "poisoned": special_build(api, B.SAMPLE_LINEAR, B.REPEAT_REPEAT_XY, False),
    }


@pytest.mark.parametrize("light_math", ["relaxed", "exact"])
@pytest.mark.parametrize("which", ["map", "cube", "poisoned"])
def test_frames_equal_with_and_without_host_records(product, monkeypatch, which, light_math):
    monkeypatch.setenv("RXR_LIGHT_MATH", light_math)
    with knobs(product, monkeypatch, ctx_env={"RXR_HOST_SETUP": "0"}):
        want, want_routes = render_all_ways(product, frame_scenes(product)[which])
    assert set(want_routes.values()) == {DEVICE_LAUNCH}, want_routes
    got, routes = render_all_ways(product, frame_scenes(product)[which])
    assert routes == {"whole": HOST_RECORDS, "stripes": HOST_RECORDS, "band on tile rows": HOST_RECORDS, "last rows": HOST_RECORDS,
                      "band off tile rows": DEVICE_LAUNCH}, routes
    assert want["whole"][..., :3].any(), "the frame is empty"
    for name in want:
        d = (got[name] != want[name]).any(axis=2)
        assert not d.any(), f"{which}, {light_math}, {name}: {int(d.sum())} pixels differ; first {np.argwhere(d)[:3].tolist()}"


def test_a_sparse_frame_under_row_spans(product, monkeypatch):
    """a small cube in the middle of the frame with the sparse-frame thresholds at zero: content rows are clamped, the raster grid is
    narrowed to row spans and EVERY pixel box is clipped to its batch's tiles -- the host records are built knowing that"""
    monkeypatch.setenv("RXR_CONTENT_MIN_TILES", "0")
    cfg = lambda: scenes.cube_scene(product, width=333, height=187, tile_size=16, textured=True, distance=6.0, logo_size=32, rect_size=8.0)  # noqa: E731
    with knobs(product, monkeypatch, ctx_env={"RXR_HOST_SETUP": "0"}):
        want, _ = render_all_ways(product, cfg())
    got, routes = render_all_ways(product, cfg())
    assert routes["whole"] == routes["stripes"] == HOST_RECORDS, routes
    for name in want:
        d = (got[name] != want[name]).any(axis=2)
        assert not d.any(), f"{name}: {int(d.sum())} pixels differ; first {np.argwhere(d)[:3].tolist()}"
    keep = upload(product, cfg())
    info = (C.c_uint32 * 4)()
    rxr = rusterix_amd.rxr_abi()
    assert rxr.rxr_debug_content(ctx_of(product), info) == 0
    assert info[0] == 1 and info[3] == 1, f"the frame takes no row spans: {list(info)}"
    assert_records_equal(product, "cube under row spans")
    del keep


def test_uploads_that_follow_each_other(product, monkeypatch):
    """two different frames on one context, then one that no longer qualifies (129 triangles: binned), then a small one again"""
    order = [("map", lambda: frame_scenes(product)["map"]), ("cube", lambda: frame_scenes(product)["cube"]),
             ("129 triangles", lambda: triangles_scene(product, STAGE_TRIS + 1)), ("map again", lambda: frame_scenes(product)["map"])]
    with knobs(product, monkeypatch, ctx_env={"RXR_HOST_SETUP": "0"}):
        want = [scenes.render(make()).copy() for _, make in order]
    for (name, make), ref in zip(order, want):
        got = scenes.render(make()).copy()
        assert setup_route(product) == (DEVICE_LAUNCH if name == "129 triangles" else HOST_RECORDS), name
        assert np.array_equal(got, ref), f"{name}: {(got != ref).any(axis=2).sum()} pixels differ"


def test_member_contexts_read_their_own_records(product, monkeypatch):
    """two member contexts on one device: each uploads the frame into its own blob and renders its stripes from its own records"""
    rxr = rusterix_amd.rxr_abi()
    cfg = frame_scenes(product)["map"]
    with knobs(product, monkeypatch, ctx_env={"RXR_HOST_SETUP": "0"}):
        want = scenes.render(cfg).copy()
    try:
        product.lib.rxh_set_devices((C.c_int * 2)(0, 0), 2)
        group = product.lib.rxh_context()
        assert rxr.rxr_member_count(group) == 2
        got = scenes.render(cfg).copy()
        assert [setup_route(product, C.c_void_p(rxr.rxr_member(group, k))) for k in range(2)] == [HOST_RECORDS, HOST_RECORDS]
    finally:
        product.lib.rxh_set_device(0)
    assert np.array_equal(got, want), f"{(got != want).any(axis=2).sum()} pixels differ"
