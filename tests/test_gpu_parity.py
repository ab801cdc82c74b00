"""GPU parity: the HIP path (through the C ABI of include/rxr.h) against the CPU oracle on the same
scene descriptions.

Bars (BASELINE.json north_star):
  * bit-exact for Nearest sampling on integer-coordinate 2D batches and for everything that involves
    no transcendental (coverage, depth, texel selection with unlit shading);
  * within 1 per 8-bit channel for the float-interpolated, lit 3D paths.  The only arithmetic that is
    not bit-reproducible between glibc and OCML is log2f/exp2f in pow32_fast (rasterizer.rs:1895-1901)
    and acosf in the spot light; everything else is IEEE-exact on both sides, so a +-1 step can only
    come from there.  TOLERANCE = 1.
"""
import zlib

import numpy as np
import pytest

from rusterix_amd import binding as B
from rusterix_amd import scenes

pytestmark = pytest.mark.gpu

TOLERANCE = 1  # per 8-bit channel, lit 3D only


def both(oracle, product, builder, **kw):
    got = scenes.render(builder(product, **kw))
    ref = scenes.render(builder(oracle, **kw))
    return got, ref


def assert_exact(got, ref, what):
    if not np.array_equal(got, ref):
        d = np.argwhere((got != ref).any(axis=2))
        y, x = d[0]
        raise AssertionError(f"{what}: {len(d)} pixels differ; first at (x={x}, y={y}): gpu={got[y, x]} oracle={ref[y, x]}")


def assert_close(got, ref, what, tol=TOLERANCE, max_outliers=0):
    diff = np.abs(got.astype(np.int16) - ref.astype(np.int16)).max(axis=2)
    bad = np.argwhere(diff > tol)
    if len(bad) > max_outliers:
        y, x = bad[0]
        raise AssertionError(f"{what}: {len(bad)} pixels differ by more than {tol}; first at (x={x}, y={y}): "
                             f"gpu={got[y, x]} oracle={ref[y, x]}")
    return int((diff > 0).sum())


# ---- 2D: bit-exact ------------------------------------------------------------------------------------
def scene_2d(api, width=256, height=160, alpha=128, background=None, ambient=None, preserve=False, lights=False,
             linedef=False, vgradient=True):
    rects = [
        api.Batch2D.from_rectangle(0.0, 0.0, 200.0, 120.0).source(B.PixelSource.Pixel((200, 40, 90, alpha))),
        api.Batch2D.from_rectangle(30.0, 20.0, 100.0, 100.0).source(B.PixelSource.StaticTileIndex(0)),
        api.Batch2D.from_rectangle(90.0, 60.0, 150.0, 90.0).source(B.PixelSource.StaticTileIndex(1)).repeat_mode(B.REPEAT_REPEAT_XY),
        api.Batch2D.from_rectangle(10.0, 100.0, 60.0, 40.0).source(B.PixelSource.StaticTileIndex(7)),  # missing tile -> transparent
    ]
    scene = api.Scene.from_static(rects, [])
    if vgradient:
        scene.background(api.VGrayGradientShader())
    if lights:
        scene.lights([B.Light(B.LIGHT_POINT).with_position((100.0, 0.0, 80.0)).with_color((1.0, 0.9, 0.6)).with_intensity(1.0)
                      .with_start_distance(20.0).with_end_distance(120.0).compile(),
                      B.Light(B.LIGHT_AMBIENT).with_color((0.2, 0.2, 0.3)).with_intensity(0.5).compile()])
    assets = api.Assets.default().textures([B.Tile.from_texture(scenes.logo_texture(1, 64)), B.Tile.from_texture(scenes.fence_texture(6))])

    def setup():
        cam = api.D3OrbitCamera.new()
        v, p = cam.matrices(float(width), float(height))
        r = api.Rasterizer.setup(None, v, p).render_mode(B.RenderMode.render_2d())
        if background is not None:
            r.background(background)
        if ambient is not None:
            r.ambient(ambient)
        if preserve:
            r.preserve_transparency(True)
        if linedef:
            r.mapmini_add_linedef((60.0, 0.0), (60.0, 200.0))
            r.mapmini_add_occluder((120.0, 0.0), (400.0, 60.0), 0.5)
        return r

    return scenes._result(api, scene, assets, setup, width, height, 40, "2d")


@pytest.mark.parametrize("kw", [
    dict(),
    dict(alpha=255),
    dict(background=(10, 20, 30, 0), vgradient=False, preserve=True),
    dict(ambient=(0.7, 0.8, 0.9, 1.0)),
    dict(ambient=(0.5, 0.5, 0.5, 1.0), lights=True, linedef=True),
    dict(lights=True),
    dict(width=203, height=77),
])
def test_2d_batches_bit_exact(oracle, product, kw):
    got, ref = both(oracle, product, scene_2d, **kw)
    assert_exact(got, ref, f"2D scene {kw}")


def test_2d_diagonal_blended_twice(oracle, product):
    """SURVEY section 8c pin 1: the rectangle's diagonal is covered by both triangles and blended twice."""
    got, ref = both(oracle, product, scene_2d, alpha=128, background=(0, 0, 0, 255), vgradient=False)
    assert_exact(got, ref, "2D diagonal")
    # the 200x120 rectangle's diagonal passes through the centre of pixel (x=2, y=1): 2.5 * 0.6 == 1.5
    assert tuple(got[1, 3]) == (100, 20, 45, 255)   # one blend of (200,40,90,128) over black, truncated
    assert tuple(got[1, 2]) == (150, 30, 67, 255)   # blended by both triangles (edge.rs:31 is inclusive)


def lines_scene(api, width=200, height=120):
    v = np.array([[10.2, 10.7], [150.9, 30.1], [90.0, 110.5], [20.0, 90.0], [-5.5, 40.0], [199.0, 119.0]], np.float32)
    uv = np.zeros_like(v)
    tris = np.array([[0, 1, 0], [1, 2, 0], [2, 3, 0], [4, 5, 0]], np.uint32)
    lines = api.Batch2D.new(v, tris, uv).mode(B.MODE_LINES).source(B.PixelSource.Pixel((255, 200, 0, 255)))
    strip = api.Batch2D.new(v[:4] + np.float32(7.0), tris[:1], uv[:4]).mode(B.MODE_LINE_STRIP)
    loop = api.Batch2D.new(v[:4] * np.float32(0.5), tris[:1], uv[:4]).mode(B.MODE_LINE_LOOP).source(B.PixelSource.Pixel((0, 255, 255, 255)))
    rect = api.Batch2D.from_rectangle(40.0, 40.0, 60.0, 30.0).source(B.PixelSource.Pixel((80, 80, 200, 100)))
    scene = api.Scene.from_static([lines, rect, strip, loop], [])
    assets = api.Assets.default()

    def setup():
        v_, p_ = api.D3OrbitCamera.new().matrices(float(width), float(height))
        return api.Rasterizer.setup(None, v_, p_).render_mode(B.RenderMode.render_2d()).background((5, 5, 5, 255))

    return scenes._result(api, scene, assets, setup, width, height, 40, "lines")


def test_bresenham_lines_bit_exact(oracle, product):
    got, ref = both(oracle, product, lines_scene)
    assert_exact(got, ref, "Bresenham line modes")
    assert (got[..., 0] == 255).any()


def test_2d_matrix_projection(oracle, product):
    def build(api):
        cfg = scene_2d(api)
        m = B.Mat3.from_rows([[1.5, 0.0, 12.0], [0.0, 1.5, -8.0], [0.0, 0.0, 1.0]])
        base = cfg.setup

        def setup():
            r0 = base()
            v, p = api.D3OrbitCamera.new().matrices(float(cfg.width), float(cfg.height))
            r = api.Rasterizer.setup(m, v, p).render_mode(B.RenderMode.render_2d()).ambient((1.0, 1.0, 1.0, 1.0))
            del r0
            return r

        cfg.setup = setup
        return cfg

    got, ref = scenes.render(build(product)), scenes.render(build(oracle))
    assert_exact(got, ref, "2D with Mat3 projection")


@pytest.mark.parametrize("params", [
    dict(),                                                              # GridShader::new(): 30 / 2 / (0, 0)
    dict(grid_size=17.0, subdivisions=3.0, offset=(5.5, -3.25)),
    dict(grid_size=8.0, subdivisions=1.0, offset=(-100.0, 250.0)),
    dict(grid_size=50.0, subdivisions=2.6, offset=(0.25, 0.75)),        # non-integer subdivisions: round() in sub_size, raw in `extra`
    dict(grid_size=0.0, subdivisions=2.0),                               # division by zero: NaN everywhere -> background colour
])
@pytest.mark.parametrize("size", [(320, 200), (333, 211)])
def test_grid_shader_background(oracle, product, params, size):
    """F2: GridShader as the scene background (shader/grid.rs), evaluated per pixel on the device, under a 2D rectangle"""
    def build(api):
        sh = api.GridShader()
        if "grid_size" in params:
            sh.set_parameter_f32("grid_size", params["grid_size"]).set_parameter_f32("subdivisions", params["subdivisions"])
        if "offset" in params:
            sh.set_parameter_vec2("offset", params["offset"])
        scene = api.Scene.empty().background(sh)
        scene.add_d2_static(api.Batch2D.from_rectangle(40.0, 30.0, 90.0, 60.0).source(B.PixelSource.Pixel((200, 40, 90, 128))))
        v, p = api.D3OrbitCamera.new().matrices(float(size[0]), float(size[1]))
        return scenes._result(api, scene, api.Assets.default(), lambda: api.Rasterizer.setup(None, v, p).render_mode(B.RenderMode.render_2d()),
                              size[0], size[1], 40, "grid")

    got, ref = scenes.render(build(product)), scenes.render(build(oracle))
    assert_exact(got, ref, f"grid shader {params} {size}")
    assert len(np.unique(got[..., 0])) >= 2 or params.get("grid_size") == 0.0


# ---- 3D -------------------------------------------------------------------------------------------------
def test_empty_scene_3d_is_black(oracle, product):
    """SURVEY section 8c pin 3: in 3D mode every non-hit pixel is [0,0,0,255] regardless of the background."""
    def build(api):
        scene = api.Scene.empty().background(api.VGrayGradientShader())
        v, p = api.D3OrbitCamera.new().matrices(64.0, 48.0)
        return scenes._result(api, scene, api.Assets.default(), lambda: api.Rasterizer.setup(None, v, p).background((9, 9, 9, 9)), 64, 48, 16, "empty")

    got = scenes.render(build(product))
    assert (got == np.array([0, 0, 0, 255], np.uint8)).all()
    assert_exact(got, scenes.render(build(oracle)), "empty scene")


@pytest.mark.parametrize("kw", [
    dict(width=320, height=200, distance=3.0, textured=True, logo_size=128),
    dict(width=320, height=200, distance=3.0, textured=False),
    dict(width=333, height=211, distance=1.2, textured=True, logo_size=128),   # near plane clipping + odd size
    dict(width=320, height=200, distance=3.0, textured=True, logo_size=128, sample_mode=B.SAMPLE_LINEAR),
])
def test_cube_unlit_bit_exact(oracle, product, kw):
    """C1: no lights, no ambient -> lit == 0 -> the colour path has no transcendental: bit-exact."""
    got, ref = both(oracle, product, scenes.cube_scene, **kw)
    assert_exact(got, ref, f"cube {kw}")


def test_teapot_ambient(oracle, product):
    """C2 (stand-in mesh): ambient only, no transcendental -> bit-exact; also exercises the bin lists."""
    got, ref = both(oracle, product, scenes.teapot_scene, width=480, height=270, logo_size=256)
    assert_exact(got, ref, "teapot ambient")
    assert (got[..., :3].max(axis=2) > 0).mean() > 0.05


def test_teapot_lit(oracle, product):
    got, ref = both(oracle, product, scenes.teapot_scene, width=480, height=270, logo_size=256, with_light=True)
    n = assert_close(got, ref, "teapot lit")
    assert n <= got.shape[0] * got.shape[1] // 50, f"{n} pixels differ by 1 -- more than log2/exp2 rounding explains"


@pytest.mark.parametrize("n_lights", [1, 16])
def test_map_scene(oracle, product, n_lights):
    """C3 / C4 at reduced resolution: lit 3D + cut-out fence + 2D logo on top."""
    kw = dict(width=640, height=360, logo_size=128, n_lights=n_lights)
    got, ref = both(oracle, product, scenes.map_scene, **kw)
    n = assert_close(got, ref, f"map {n_lights} lights")
    assert n <= got.shape[0] * got.shape[1] // 50
    assert_exact(got[:200, :200], ref[:200, :200], "2D logo rectangle over the 3D frame")  # bit-exact part


def test_map_scene_linear_sampling(oracle, product):
    kw = dict(width=400, height=240, logo_size=128, n_lights=4, sample_mode=B.SAMPLE_LINEAR)
    got, ref = both(oracle, product, scenes.map_scene, **kw)
    assert_close(got, ref, "map linear")


def test_box_grid(oracle, product):
    """C5 in miniature: many small triangles through the bins, Linear sampling, ambient only -> exact."""
    kw = dict(n=24, width=512, height=288)
    got, ref = both(oracle, product, scenes.box_grid_scene, **kw)
    assert_exact(got, ref, "box grid")
    assert (got[..., :3].max(axis=2) > 0).mean() > 0.1


def test_all_light_types_and_sun(oracle, product):
    def build(api):
        cfg = scenes.map_scene(api, width=320, height=180, logo_size=64, n_lights=1)
        sc = cfg.scene
        sc.lights([
            B.Light(B.LIGHT_AMBIENT).with_color((0.1, 0.2, 0.1)).with_intensity(0.5).compile(),
            B.Light(B.LIGHT_AMBIENT_DAYLIGHT).with_color((0.1, 0.1, 0.2)).with_intensity(0.4).with_flicker(0.3).compile(),
            _light(B.LIGHT_SPOT, (7.0, 1.8, 8.0), direction=(0.0, -1.0, 0.3), cone_angle=0.7, end=9.0, start=1.0, intensity=2.0),
            _light(B.LIGHT_AREA, (3.0, 1.0, 12.0), normal=(0.0, 0.0, -1.0), end=6.0, start=1.0, intensity=1.5, width=2.0, height=1.0),
            _light(B.LIGHT_AREA, (12.0, 1.0, 12.0), normal=(-1.0, 0.0, 0.0), end=6.0, start=1.0, intensity=0.7, width=2.0, height=1.0, from_linedef=True),
            _light(B.LIGHT_DAYLIGHT, (7.0, 3.0, 10.0), normal=(0.0, -1.0, 0.0), end=12.0, start=2.0, intensity=0.8),
        ])
        sc.add_dynamic_light(B.Light(B.LIGHT_POINT).with_position((2.0, 1.0, 6.0)).with_color((0.9, 0.3, 0.2)).with_intensity(1.2)
                             .with_start_distance(1.0).with_end_distance(5.0).with_flicker(0.5).compile())
        base = cfg.setup

        def setup():
            return base().sun((0.3, -1.0, 0.2), 0.6).mapmini_add_occluder((0.0, 9.0), (6.0, 15.0), 0.35)

        cfg.setup = setup
        return cfg

    got, ref = scenes.render(build(product)), scenes.render(build(oracle))
    # acosf decides cone membership (`angle > cone_angle`, light.rs:559-580: a hard cut-off, and glibc's and OCML's acosf differ in the
    # last place): a fragment exactly on the cone's edge may fall on the other side.  Allowed: at most 8 such pixels, each of them ON
    # that edge -- i.e. where the oracle's own frame jumps by at least as much between neighbours.  Everything else within 1.
    diff = np.abs(got.astype(np.int16) - ref.astype(np.int16)).max(axis=2)
    bad = np.argwhere(diff > TOLERANCE)
    assert len(bad) <= 8, f"all light types: {len(bad)} pixels differ by more than {TOLERANCE}"
    r = ref.astype(np.int16)
    for y, x in bad:
        y0, y1, x0, x1 = max(y - 1, 0), min(y + 2, r.shape[0]), max(x - 1, 0), min(x + 2, r.shape[1])
        jump = int(np.abs(r[y0:y1, x0:x1] - r[y, x]).max())
        assert jump * 2 >= int(diff[y, x]), f"all light types: pixel (x={x}, y={y}) is off by {int(diff[y, x])} away from any edge of the oracle's frame (jump {jump})"


def _light(kind, pos, direction=(0.0, 0.0, -1.0), cone_angle=0.785, normal=(0.0, 1.0, 0.0), start=1.0, end=2.0, intensity=1.0,
           width=1.0, height=1.0, from_linedef=False):
    l = B.Light(kind).with_position(pos).with_intensity(intensity).with_start_distance(start).with_end_distance(end)
    l.direction, l.cone_angle, l.normal, l.width, l.height, l.from_linedef = direction, cone_angle, normal, width, height, from_linedef
    return l.compile()


def test_chunks_opacity_and_profile_ids(oracle, product):
    """Rows R4/R5: chunk opacity batches, src-over resolve, surface-id skip, chunk occlusion + chunk lights."""
    def build(api):
        scene = api.Scene.empty()
        ch = scene.add_chunk()
        wall = api.Batch3D.from_box(-1.0, -1.0, -0.2, 2.0, 2.0, 0.2).source(B.PixelSource.StaticTileIndex(0)).with_computed_normals().profile_id(7)
        other = api.Batch3D.from_box(-2.5, -0.5, -1.5, 1.0, 1.0, 1.0).source(B.PixelSource.Pixel((40, 200, 90, 255))).with_computed_normals().profile_id(9)
        glass = api.Batch3D.from_box(-0.8, -0.8, 0.6, 1.6, 1.6, 0.05).source(B.PixelSource.Pixel((200, 220, 255, 110))).with_computed_normals().profile_id(7)
        glass2 = api.Batch3D.from_box(-2.6, -0.6, 0.4, 1.2, 1.2, 0.05).source(B.PixelSource.StaticTileIndex(1)).with_computed_normals()
        ch.add_batch3d(wall).add_batch3d(other).add_batch3d_opacity(glass).add_batch3d_opacity(glass2)
        ch.add_occluder((-3.0, -3.0), (-1.2, 3.0), 0.4)
        ch.add_light(B.Light(B.LIGHT_POINT).with_position((0.0, 1.5, 2.0)).with_intensity(2.0).with_start_distance(1.0).with_end_distance(8.0).compile())
        scene.add_d3_static(api.Batch3D.from_box(1.3, -0.5, -0.5, 0.8, 0.8, 0.8).source(B.PixelSource.Pixel((220, 60, 60, 255))).with_computed_normals())
        assets = api.Assets.default().textures([B.Tile.from_texture(scenes.brick_texture(2)), B.Tile.from_texture(scenes.fence_texture(6))])
        cam = api.D3OrbitCamera.new()
        cam.set_parameter_f32("distance", 4.5)
        v, p = cam.matrices(320.0, 200.0)
        return scenes._result(api, scene, assets, lambda: api.Rasterizer.setup(None, v, p).ambient((0.6, 0.6, 0.6, 1.0)), 320, 200, 40, "chunks")

    got, ref = scenes.render(build(product)), scenes.render(build(oracle))
    assert_close(got, ref, "chunk opacity scene")


# ---- properties -------------------------------------------------------------------------------------------
def test_row_bands_equal_full_frame(product):
    """Multi-GPU sharding invariant: rendering row bands separately gives the same bytes as one launch."""
    import ctypes as C

    cfg = scenes.map_scene(product, width=640, height=360, logo_size=64, n_lights=4)
    full = scenes.render(cfg).copy()
    lib = product.lib
    rxr = __import__("rusterix_amd").rxr_abi()
    r = cfg.setup()
    assert lib.rxh_rasterizer_upload(r._h, cfg.scene._h, cfg.width, cfg.height, cfg.tile_size, cfg.assets._h) == 0
    ctx = lib.rxh_context()
    out = np.zeros((cfg.height, cfg.width, 4), np.uint8)
    for (a, b) in [(0, 45), (45, 90), (90, 203), (203, 360)]:  # deliberately not tile aligned
        assert rxr.rxr_render_rows(ctx, a, b) == 0
        assert rxr.rxr_download_rows(ctx, out.ctypes.data_as(C.POINTER(C.c_uint8)), a, b) == 0
    assert_exact(out, full, "row bands vs full frame")


@pytest.mark.parametrize("cull", ["off", "back", "front"])
def test_edges_built_on_the_device_equal_the_hosts(oracle, product, cull):
    """ABI 5: host-projected 3D batches cross the boundary without their Edges records (rxr_batch3d.edges == NULL: one `visible` word per
    triangle and the batch's cull mode instead of 40 bytes per triangle); the device builds the records from the projected vertices with
    the operations of Edges::new behind the winding swap (src/edge.rs:12-24, src/batch/batch3d.rs:706-746).  The frame must equal the one
    rendered from the host's records, bit for bit, and the oracle's -- for every cull mode (front- and back-facing triangles, swapped and
    not), for clipped geometry (appended fan triangles) and for a large streamed scene."""
    mode = {"off": B.CULL_OFF, "back": B.CULL_BACK, "front": B.CULL_FRONT}[cull]

    def build(api, which):
        if which == "cube":       # the camera inside the near range of a big cube: triangles cross the near plane (clipped fans)
            box = api.Batch3D.from_box(-2.0, -2.0, -2.0, 4.0, 4.0, 4.0).cull_mode(mode).with_computed_normals().source(B.PixelSource.StaticTileIndex(0))
            scene = api.Scene.from_static([], [box])
            assets = api.Assets.default().textures([B.Tile.from_texture(scenes.logo_texture(1, 64))])
            cam = api.D3OrbitCamera.new()
            cam.set_parameter_f32("distance", 2.6)
            return scenes._result(api, scene, assets, lambda: api.Rasterizer.setup(None, *cam.matrices(640.0, 400.0)).ambient((1.0, 1.0, 1.0, 1.0)), 640, 400, 40, "cube-near")
        if which == "teapot":
            cfg = scenes.teapot_scene(api, width=640, height=360, logo_size=64)
            return cfg
        return scenes.box_grid_scene(api, n=64, width=1280, height=720)   # 49 152 triangles in 64 batches: the streamed hand-over

    for which in (["cube", "teapot", "grid"] if cull == "off" else ["cube"]):
        ref = scenes.render(build(oracle, which))
        assert product.lib.rxh_get_device_edges() == 1, "the default is the hand-over without Edges records"
        got = scenes.render(build(product, which)).copy()
        product.lib.rxh_set_device_edges(0)
        try:
            with_records = scenes.render(build(product, which)).copy()
        finally:
            product.lib.rxh_set_device_edges(1)
        assert_exact(got, with_records, f"{which}, cull {cull}: Edges built on the device vs the host's records")
        assert_exact(got, ref, f"{which}, cull {cull}: vs oracle")
        assert (got[..., :3].max(axis=2) > 0).mean() > 0.02


def _sparse_scene(api, kind):
    """scenes whose content leaves whole tile rows of the frame empty (rxr_ctx::content_row0 / 1)"""
    if kind == "grid":          # a distant box grid: a band in the middle of the frame, binned, row mode
        cfg = scenes.box_grid_scene(api, n=16, width=640, height=480)
        cam_far = api.D3OrbitCamera.new()
        cam_far.center = (1.6, 0.0, 1.6)
        cam_far.distance = 9.0
        cfg.setup = (lambda c=cam_far: api.Rasterizer.setup(None, *c.matrices(640.0, 480.0)).sample_mode(B.SAMPLE_LINEAR).ambient((1.0, 1.0, 1.0, 1.0)))
        return cfg
    if kind == "cube_and_logo":  # a small cube (3D) and a 2D rectangle low in the frame: the content is the union of the two
        return scenes.cube_scene(api, width=640, height=480, tile_size=40, textured=True, distance=12.0)
    if kind == "nothing":       # 3D mode, every batch behind the camera's back: no content at all
        cfg = scenes.cube_scene(api, width=333, height=211, tile_size=40, textured=True, distance=3.0, rect_size=0.0)  # (a 2D rectangle without pixels)
        cam = api.D3OrbitCamera.new()
        cam.center = (0.0, 500.0, 0.0)
        cam.distance = 1.0
        cfg.setup = lambda c=cam: api.Rasterizer.setup(None, *c.matrices(333.0, 211.0))
        return cfg
    raise ValueError(kind)


@pytest.mark.parametrize("kind", ["grid", "cube_and_logo", "nothing"])
def test_rows_without_content_are_filled_not_rastered(oracle, product, kind, monkeypatch):
    """Rows that no batch box reaches (the rows of the reference's own tiles that pass its batch box test, rasterizer.rs:978-983) are written
    by a fill, the pre-pass and the raster kernel run over the rows in between: the frame equals the oracle's, the frame rendered with the
    clamp switched off (RXR_CONTENT_ROWS=0), and the frame assembled from row bands that cut through content and emptiness alike."""
    import ctypes as C

    from tests.test_gpu_sparse_frames import assert_scratch_clean

    monkeypatch.setenv("RXR_CONTENT_MIN_TILES", "0")   # (the clamps only pay from 8192 empty tiles on: these frames are small)
    cfg = _sparse_scene(product, kind)
    got = scenes.render(cfg).copy()
    assert_scratch_clean(product, f"sparse frame ({kind})")
    ref = scenes.render(_sparse_scene(oracle, kind))
    assert_exact(got, ref, f"sparse frame ({kind}) vs oracle")
    hit_rows = np.nonzero((got[..., :3].max(axis=2) > 0).any(axis=1))[0]
    if kind == "nothing":
        assert len(hit_rows) == 0 and (got[..., 3] == 255).all()
    else:
        assert len(hit_rows) and (hit_rows.min() > 32 or hit_rows.max() < cfg.height - 32), "the scene leaves no rows empty: it tests nothing"
    lib = product.lib
    rxr = __import__("rusterix_amd").rxr_abi()
    info = (C.c_uint32 * 4)()
    assert rxr.rxr_debug_content(C.c_void_p(lib.rxh_context()), info) == 0
    assert info[0] == 1, "the frame's content rows are not known: the test tests nothing"
    if kind == "grid":
        assert 0 < info[1] < info[2] < cfg.height and info[3] == 1, list(info)   # rows above and below, and columns left and right (row spans)
    if kind == "nothing":
        assert info[1] >= info[2], list(info)
    monkeypatch.setenv("RXR_ROW_SPANS", "0")
    no_spans = scenes.render(cfg).copy()
    assert_scratch_clean(product, f"sparse frame ({kind}) without row spans")
    assert rxr.rxr_debug_content(C.c_void_p(lib.rxh_context()), info) == 0 and info[3] == 0
    monkeypatch.delenv("RXR_ROW_SPANS")
    assert_exact(got, no_spans, f"sparse frame ({kind}): row spans on vs off")
    monkeypatch.setenv("RXR_CONTENT_ROWS", "0")
    unclamped = scenes.render(cfg).copy()
    assert_scratch_clean(product, f"sparse frame ({kind}) without the clamp")
    assert rxr.rxr_debug_content(C.c_void_p(lib.rxh_context()), info) == 0 and info[0] == 0 and info[3] == 0
    monkeypatch.delenv("RXR_CONTENT_ROWS")
    assert_exact(got, unclamped, f"sparse frame ({kind}): clamp on vs off")
    r = cfg.setup()
    assert lib.rxh_rasterizer_upload(r._h, cfg.scene._h, cfg.width, cfg.height, cfg.tile_size, cfg.assets._h) == 0
    ctx = lib.rxh_context()
    out = np.full((cfg.height, cfg.width, 4), 7, np.uint8)
    H = cfg.height
    cuts = sorted({0, 5, H // 7, H // 3 + 1, H // 2, (2 * H) // 3 + 3, H - 9, H})
    for a, b in zip(cuts[:-1], cuts[1:]):
        assert rxr.rxr_render_rows(ctx, a, b) == 0
        assert_scratch_clean(product, f"sparse frame ({kind}): band [{a}, {b})")
        assert rxr.rxr_download_rows(ctx, out.ctypes.data_as(C.POINTER(C.c_uint8)), a, b) == 0
    assert_exact(out, got, f"sparse frame ({kind}): row bands vs whole frame")


def test_sparse_frame_into_caller_buffers_and_stripes(product, monkeypatch):
    """the fills of a sparse frame address the CALLER's device buffer (rxr_render_rows_to: `dev_pixels` points at row0 of the band, not at
    row 0 of the frame), and stripe launches (a multi-GPU share) are not clamped at all: bands into separate torch buffers and the
    de-interleaved stripes of three ranks must both give the whole frame"""
    import ctypes as C

    import torch

    monkeypatch.setenv("RXR_CONTENT_MIN_TILES", "0")
    cfg = _sparse_scene(product, "grid")
    whole = scenes.render(cfg).copy()
    lib = product.lib
    rxr = __import__("rusterix_amd").rxr_abi()
    r = cfg.setup()
    assert lib.rxh_rasterizer_upload(r._h, cfg.scene._h, cfg.width, cfg.height, cfg.tile_size, cfg.assets._h) == 0
    ctx = C.c_void_p(lib.rxh_context())
    W, H = cfg.width, cfg.height
    st = torch.cuda.Stream()
    got = np.zeros((H, W, 4), np.uint8)
    for a, b in [(0, 100), (100, 213), (213, 300), (300, H)]:
        buf = torch.full((b - a, W, 4), 9, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()   # (the fill ran on torch's default stream, the render runs on `st`: no implicit order between the two)
        assert rxr.rxr_render_rows_to(ctx, a, b, C.c_void_p(buf.data_ptr()), C.c_void_p(st.cuda_stream)) == 0
        assert rxr.rxr_synchronize(ctx) == 0
        got[a:b] = buf.cpu().numpy()
    assert_exact(got, whole, "sparse frame: bands into caller buffers")
    n_stripes = (H + 15) // 16
    out = np.zeros((n_stripes * 16, W, 4), np.uint8)
    for rank in range(3):
        mine = list(range(rank, n_stripes, 3))
        buf = torch.full((len(mine) * 16, W, 4), 9, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        assert rxr.rxr_render_stripes_to(ctx, rank, 3, C.c_void_p(buf.data_ptr()), C.c_void_p(st.cuda_stream)) == 0
        assert rxr.rxr_synchronize(ctx) == 0
        h = buf.cpu().numpy()
        for j, sidx in enumerate(mine):
            out[sidx * 16:(sidx + 1) * 16] = h[j * 16:(j + 1) * 16]
    assert_exact(out[:H], whole, "sparse frame: stripes of three ranks")


@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_stripes_equal_full_frame(product, world):
    """The multi-GPU sharding primitive on ONE GPU: every rank's interleaved stripes rendered in turn
    (rxr_render_stripes_to), assembled like the all-gather does, must equal the single-launch frame
    byte for byte (1 GPU == N GPU)."""
    import ctypes as C

    import torch

    from rusterix_amd import distributed as D

    cfg = scenes.map_scene(product, width=400, height=250, logo_size=64, n_lights=3)   # 250 rows: ragged last stripe
    full = scenes.render(cfg).copy()
    lib = product.lib
    rxr = __import__("rusterix_amd").rxr_abi()
    r = cfg.setup()
    assert lib.rxh_rasterizer_upload(r._h, cfg.scene._h, cfg.width, cfg.height, cfg.tile_size, cfg.assets._h) == 0
    ctx = lib.rxh_context()
    spr = D.stripes_per_rank(cfg.height, world)
    parts = []
    for rank in range(world):
        band = torch.full((spr * D.TILE_H, cfg.width, 4), 77, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        assert rxr.rxr_render_stripes_to(ctx, rank, world, C.c_void_p(band.data_ptr()), None) == 0
        assert rxr.rxr_synchronize(ctx) == 0
        parts.append(band.cpu().numpy())
    frame = D.assemble_numpy(np.concatenate(parts, axis=0), cfg.height, cfg.width, world)
    assert_exact(frame, full, f"{world}-way stripes vs full frame")


def test_tile_size_invariance(oracle, product):
    """R9: the oracle's output does not depend on tile_size, and equals the GPU's (which ignores it)."""
    frames = []
    for ts in (16, 40, 200):
        cfg = scenes.cube_scene(oracle, width=256, height=160, tile_size=ts, textured=True, distance=3.0, logo_size=64)
        frames.append(scenes.render(cfg).copy())
    assert_exact(frames[0], frames[1], "oracle tile 16 vs 40")
    assert_exact(frames[0], frames[2], "oracle tile 16 vs 200")
    got = scenes.render(scenes.cube_scene(product, width=256, height=160, tile_size=40, textured=True, distance=3.0, logo_size=64))
    assert_exact(got, frames[0], "gpu vs oracle")


def test_frame_size_sequence(oracle, product):
    """Regression: the per-context scratch (bin counters handed back zeroed by the raster kernel) must
    stay consistent when frame sizes shrink and grow without a reallocation in between."""
    for (w, h) in [(640, 360), (160, 96), (480, 270), (96, 64), (640, 360), (333, 211)]:
        got, ref = both(oracle, product, scenes.teapot_scene, width=w, height=h, logo_size=64)
        assert_exact(got, ref, f"teapot {w}x{h} in a size sequence")
        got, ref = both(oracle, product, scenes.box_grid_scene, n=12, width=w, height=h)
        assert_exact(got, ref, f"box grid {w}x{h} in a size sequence")


def test_repeatability(product):
    cfg = scenes.map_scene(product, width=320, height=180, logo_size=64, n_lights=16)
    a = scenes.render(cfg).copy()
    b = scenes.render(cfg).copy()
    assert_exact(a, b, "same frame twice")


def test_full_size_frame_properties(product):
    """BASELINE config C4 at full size (3840x2160, 16 lights): size-independent properties only."""
    cfg = scenes.map_scene(product, width=3840, height=2160, n_lights=16)
    img = scenes.render(cfg)
    assert (img[..., 3] == 255).all()                       # every pixel resolved (rasterizer.rs:420-461)
    assert (img[: 2160 // 3, 300:] == np.array([0, 0, 0, 255], np.uint8)).all(axis=2).mean() > 0.5   # sky is black
    assert img[1500:, :, :3].max() > 60                      # lit floor
    # band invariance at full size through a checksum of checksums
    rows = [zlib.crc32(img[y].tobytes()) for y in range(0, 2160, 135)]
    img2 = scenes.render(cfg)
    assert rows == [zlib.crc32(img2[y].tobytes()) for y in range(0, 2160, 135)]


# ---- error behaviour ---------------------------------------------------------------------------------------
def test_errors_are_reported_not_thrown(product):
    scene = product.Scene.from_static([], [product.Batch3D.from_box(-0.5, -0.5, -0.5, 1, 1, 1)])  # no normals: reference panics
    v, p = product.D3OrbitCamera.new().matrices(64.0, 64.0)
    out = np.zeros(64 * 64 * 4, np.uint8)
    with pytest.raises(B.RasterizeError) as e:
        product.Rasterizer.setup(None, v, p).rasterize(scene, out, 64, 64, 16, product.Assets.default())
    assert e.value.code == B.RXR_ERR_INVALID
    scene = product.Scene.from_static([], [product.Batch3D.from_box(-0.5, -0.5, -0.5, 1, 1, 1).with_computed_normals()
                                           .source(B.PixelSource.StaticTileIndex(3))])  # tile_list[3] panics
    cam = product.D3OrbitCamera.new()
    cam.set_parameter_f32("distance", 3.0)
    v, p = cam.matrices(64.0, 64.0)
    with pytest.raises(B.RasterizeError) as e:
        product.Rasterizer.setup(None, v, p).rasterize(scene, out, 64, 64, 16, product.Assets.default())
    assert e.value.code == B.RXR_ERR_INVALID
    with pytest.raises(B.RasterizeError):
        product.Rasterizer.setup(None, v, p).rasterize(product.Scene.empty(), out, 64, 64, 0, product.Assets.default())


# ---- 2D at scale: binned + per-tile sorted primitive lists ------------------------------------------------
many_rects_scene = scenes.tile_map_2d_scene


@pytest.mark.parametrize("kw", [dict(), dict(width=333, height=211, nx=17, ny=11), dict(stacked=600, nx=12, ny=8), dict(lights=False, lines=False)])
def test_2d_many_rectangles_bit_exact(oracle, product, kw):
    got, ref = both(oracle, product, many_rects_scene, **kw)
    assert_exact(got, ref, f"2D tile map {kw}")
    assert len(np.unique(got.reshape(-1, 4), axis=0)) > 100


def test_2d_many_rectangles_over_3d(oracle, product):
    """2D primitives binned + sorted on top of a lit 3D frame (both pre-passes in one frame)."""
    def build(api):
        cfg = scenes.map_scene(api, width=480, height=300, logo_size=64, n_lights=3)
        over = many_rects_scene(api, width=480, height=300, nx=16, ny=10, lights=False)
        # move the rectangles of `over` into the map scene as dynamic 2D batches: rebuild them here
        rng = np.random.default_rng(5)
        for j in range(10):
            for i in range(16):
                if (i + j) % 2:
                    continue
                cfg.scene.add_d2_dynamic(api.Batch2D.from_rectangle(i * 30.0 + 2.0, j * 30.0 + 1.0, 33.0, 33.0)
                                         .source(B.PixelSource.Pixel(tuple(int(x) for x in rng.integers(0, 256, 3)) + (int(rng.integers(30, 256)),))))
        del over
        return cfg

    got, ref = scenes.render(build(product)), scenes.render(build(oracle))
    assert_close(got, ref, "2D tile map over 3D")


@pytest.mark.parametrize("kind", ["small", "binned", "binned_general", "binned_2d", "binned_sparse"])
def test_pipelined_download_equals_single_launch(product, kind, monkeypatch):
    """rxr_render_download rasters frames of 4 Mpixel and more in four bands behind ONE pre-pass and downloads each band while the next
    renders (include/rxr.h); the caller's buffer must equal render_rows + download_rows byte for byte -- for frames without a pre-pass
    (rounds 1-3), and since round 4 for binned frames: bins by k_blockscan, bins by the general count / scan / fill pipeline, and a binned
    2D pass on top.  binned_sparse: a frame with empty rows and row ends -- only the strips inside the row spans cross PCIe
    (hipMemcpy2DAsync), the host writes the rest of the caller's buffer."""
    import ctypes as C

    if kind == "binned_general":
        monkeypatch.setenv("RXR_BLOCKSCAN", "0")
    if kind == "binned_sparse":
        monkeypatch.setenv("RXR_CONTENT_MIN_TILES", "0")   # (the clamps and the column trim only pay on larger frames)
    if kind == "small":
        cfg = scenes.map_scene(product, width=2304, height=1832, logo_size=64, n_lights=3)   # over the 4 Mpixel threshold; 1832 rows = 114.5 tile rows: ragged bands
    elif kind == "binned_2d":
        cfg = scenes.tile_map_2d_scene(product, width=2304, height=1832, nx=60, ny=40)
    elif kind == "binned_sparse":
        cfg = scenes.box_grid_scene(product, n=40, width=2304, height=1832, distance=22.0)    # the lattice in the middle of the frame
    else:
        cfg = scenes.box_grid_scene(product, n=40, width=2304, height=1832)                   # 19 200 triangles: binned, row mode
    piped = np.full((cfg.height, cfg.width, 4), 7, np.uint8)
    piped[...] = scenes.render(cfg)            # Rasterizer::rasterize -> rxr_render_download
    lib = product.lib
    rxr = __import__("rusterix_amd").rxr_abi()
    r = cfg.setup()
    assert lib.rxh_rasterizer_upload(r._h, cfg.scene._h, cfg.width, cfg.height, cfg.tile_size, cfg.assets._h) == 0
    ctx = lib.rxh_context()
    single = np.zeros((cfg.height, cfg.width, 4), np.uint8)
    assert rxr.rxr_render_rows(ctx, 0, cfg.height) == 0
    assert rxr.rxr_download_rows(ctx, single.ctypes.data_as(C.POINTER(C.c_uint8)), 0, cfg.height) == 0
    assert_exact(piped, single, "pipelined download vs single launch")
    if kind != "binned_2d":
        assert piped[..., 3].min() == 255
    assert (piped[..., :3].max(axis=2) > 0).mean() > (0.01 if kind == "binned_sparse" else 0.05)
    if kind == "binned_sparse":
        info = (C.c_uint32 * 4)()
        assert rxr.rxr_debug_content(C.c_void_p(ctx), info) == 0 and info[0] == 1 and info[3] == 1, list(info)
    # ... and a second pipelined call on the same context (the bins were handed back clean by the banded launches)
    again = scenes.render(cfg)
    assert_exact(again, single, "second pipelined download")


def test_pipelined_download_repairs_a_list_overflow(product, monkeypatch):
    """bins that overflow under the banded raster launches (two slots per bin for k_blockscan): rxr_synchronize sends the frame through the
    general pipeline and renders the whole frame again, and the caller's buffer is downloaded once more -- never the incomplete bands"""
    import ctypes as C

    rxr = __import__("rusterix_amd").rxr_abi()
    cfg = scenes.box_grid_scene(product, n=40, width=2304, height=1832)
    good = scenes.render(cfg).copy()
    before = rxr.rxr_debug_rerenders(C.c_void_p(product.lib.rxh_context()))
    monkeypatch.setenv("RXR_BLOCKSCAN_CAP", "2")   # (read per upload)
    repaired = scenes.render(cfg).copy()
    after = rxr.rxr_debug_rerenders(C.c_void_p(product.lib.rxh_context()))
    assert after > before, "the test scene did not overflow anything: it tests nothing"
    assert_exact(repaired, good, "frame after a repaired overflow vs the same frame with lists that fit")
    assert (good[..., :3].max(axis=2) > 0).mean() > 0.05


@pytest.mark.parametrize("shader", [False, True])
def test_million_triangle_grid_full_size_is_bit_exact(oracle, product, shader):
    """BASELINE.json configs[4] at its FULL size: 289 batches x 289 boxes = 1 002 252 triangles (991 848 after the frustum
    reject), 7680 x 4320, Linear sampling, with and without the per-batch Rusteria program -- against the oracle on all host
    threads (about a second per frame on the GPU box's 256 threads).  No lights: every colour path is exact."""
    kw = dict(n=289, width=7680, height=4320, shader=shader)
    got = scenes.render(scenes.box_grid_scene(product, **kw))
    assert got[..., 3].min() == 255 and (got[..., :3].max(axis=2) > 0).mean() > 0.3
    ref = scenes.render(scenes.box_grid_scene(oracle, **kw))
    diff = (got != ref).any(axis=2)
    assert not diff.any(), f"{int(diff.sum())} of {diff.size} pixels differ; first {np.argwhere(diff)[:3].tolist()}"


@pytest.mark.parametrize("name, builder, kw, tol, max_differing", [
    ("C2 teapot 1920x1080", scenes.teapot_scene, dict(width=1920, height=1080), 0, 0),
    ("C3 map 1920x1080, 1 light", scenes.map_scene, dict(width=1920, height=1080, n_lights=1), 1, 64),
    ("C4 map 3840x2160, 16 lights", scenes.map_scene, dict(width=3840, height=2160, n_lights=16), 1, 256),
])
def test_baseline_configs_at_full_size(oracle, product, name, builder, kw, tol, max_differing):
    """BASELINE.json configs[1..3] at their full sizes against the oracle: bit-exact without lights; with lights nothing off by more
    than 1 and only a handful of pixels off at all.  The pixel counts (64 / 256) are what the library's DEFAULT light-loop mode --
    relaxed, rxr_set_light_math -- needs: it spends BASELINE.json's 1-per-channel tolerance on v_rsq / v_rcp products and leaves 4 of
    2 073 600 (C3) and 112 of 8 294 400 (C4) pixels one step off; exact mode, where only log2f / exp2f of the two math libraries differ,
    leaves 0 and 1 (tests/test_gpu_light_math.py::test_the_bench_frame_in_both_modes bounds it at 16)."""
    got = scenes.render(builder(product, **kw))
    ref = scenes.render(builder(oracle, **kw))
    diff = np.abs(got.astype(np.int16) - ref.astype(np.int16)).max(axis=2)
    assert int(diff.max()) <= tol, f"{name}: max |diff| {int(diff.max())}"
    assert int((diff > 0).sum()) <= max_differing, f"{name}: {int((diff > 0).sum())} pixels differ"


@pytest.mark.parametrize("size", [(1, 1), (1, 37), (37, 1), (2, 2), (15, 17), (16, 16), (17, 15), (33, 31), (4097, 3), (3, 2051)])
@pytest.mark.parametrize("tile_size", [1, 7, 40, 5000])
def test_degenerate_frame_and_tile_sizes(oracle, product, size, tile_size):
    """frames of one pixel, one row, one column, just above and below the device's 16 x 16 tiles, very wide and very tall, with the
    reference's tile_size from 1 to larger than the frame (rasterizer.rs:256-270: step_by(tile_size), the last tiles clipped): the lit
    map (within one step), the teapot and the 2D scene (bit-exact)"""
    w, h = size

    def sized(builder, **kw):
        def build(api):
            cfg = builder(api, width=w, height=h, **kw)
            cfg.tile_size = tile_size
            return cfg
        return build

    got, ref = scenes.render(sized(scenes.map_scene, n_lights=3, logo_size=16)(product)), scenes.render(sized(scenes.map_scene, n_lights=3, logo_size=16)(oracle))
    assert got.shape == (h, w, 4)
    assert_close(got, ref, f"map {w}x{h} tile {tile_size}", max_outliers=0)
    got, ref = scenes.render(sized(scene_2d)(product)), scenes.render(sized(scene_2d)(oracle))
    assert_exact(got, ref, f"2D {w}x{h} tile {tile_size}")
    if w * h <= 20000:
        got, ref = scenes.render(sized(scenes.teapot_scene, logo_size=16)(product)), scenes.render(sized(scenes.teapot_scene, logo_size=16)(oracle))
        assert_exact(got, ref, f"teapot {w}x{h} tile {tile_size}")


@pytest.mark.parametrize("size", [(32768, 3), (3, 32768), (32768, 17)])
def test_frames_at_the_size_limit(oracle, product, size):
    """the largest frame edge the boundary accepts (32768: pixel boxes are 16-bit fields with an exclusive maximum), wide and tall"""
    w, h = size
    got = scenes.render(scenes.map_scene(product, width=w, height=h, n_lights=2, logo_size=16))
    ref = scenes.render(scenes.map_scene(oracle, width=w, height=h, n_lights=2, logo_size=16))
    assert_close(got, ref, f"map {w}x{h}")
    got, ref = both(oracle, product, scene_2d, width=w, height=h)
    assert_exact(got, ref, f"2D {w}x{h}")
    with pytest.raises(B.RasterizeError) as e:
        scenes.render(scene_2d(product, width=32769 if w > h else 3, height=3 if w > h else 32769))
    assert e.value.code == B.RXR_ERR_INVALID
