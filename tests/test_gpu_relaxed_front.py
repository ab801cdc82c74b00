"""The front half of a relaxed fragment (shade3d_begin / shade3d_end<LV, true>, rusterix_amd/csrc/rxr_kernels.hip): the screen-to-world
chain with 2 / width and -2 / height rounded by the host (RasterParams.ndc_sx / ndc_sy, rxr_upload_frame) and a reciprocal product for
the perspective divide, the alpha byte taken from the texel (both modes) -- against the CPU oracle.  Every case: relaxed mode within 1
per 8-bit channel, at most 4 + n / 2000 pixels off at all (the bar of tests/test_gpu_light_math.py), and the alpha plane equal to the
oracle's.

The frames are small on purpose: 333 x 187 is neither a power of two (2 / width and 2 / height are rounded numbers) nor a multiple of
the 16-pixel tile (edge tiles); 64 x 48 is the smallest frame with several tiles in a row."""
import numpy as np
import pytest

from rusterix_amd import binding as B
from rusterix_amd import scenes
from tests.routes import last_raster_kernel

pytestmark = pytest.mark.gpu

TOLERANCE = 1  # per 8-bit channel (BASELINE.json north_star, lit 3D paths)
NAN, INF, FLT_MAX = float("nan"), float("inf"), 3.4028234663852886e38


@pytest.fixture()
def light_math(product, monkeypatch):
    monkeypatch.delenv("RXR_LIGHT_MATH", raising=False)
    monkeypatch.delenv("RXR_RL_FLIP_GUARD", raising=False)

    def choose(exact):
        product.lib.rxh_set_light_math_exact(1 if exact else 0)

    yield choose
    product.lib.rxh_set_light_math_exact(0)  # the default


def channel_diff(a, b):
    return np.abs(a.astype(np.int16) - b.astype(np.int16)).max(axis=2)


def assert_relaxed_bar(got, ref, what):
    n = ref.shape[0] * ref.shape[1]
    d = channel_diff(got, ref)
    off = int((d > 0).sum())
    print(f"{what}: {off} of {n} pixels differ from the oracle, max {int(d.max())}")
    assert int(d.max()) <= TOLERANCE, f"{what}: off by {int(d.max())}; first at {np.argwhere(d > TOLERANCE)[:2].tolist()}"
    assert off <= 4 + n // 2_000, f"{what}: {off} of {n} pixels differ from the oracle"
    assert np.array_equal(got[..., 3], ref[..., 3]), f"{what}: the alpha plane"


def assert_exact_bar(got, ref, what):
    """exact mode against the oracle as tests/test_gpu_light_math.py asks it: only the two math libraries' log2f / exp2f may differ"""
    n = ref.shape[0] * ref.shape[1]
    d = channel_diff(got, ref)
    assert int(d.max()) <= TOLERANCE and int((d > 0).sum()) <= 2 + n // 50_000, f"{what}: exact mode, {int((d > 0).sum())} of {n} pixels differ, max {int(d.max())}"
    assert np.array_equal(got[..., 3], ref[..., 3]), f"{what}: the alpha plane"


@pytest.mark.parametrize("width,height", [(333, 187), (64, 48)])
def test_the_lit_map_at_awkward_frame_sizes(oracle, product, light_math, width, height):
    kw = dict(width=width, height=height, logo_size=16, n_lights=16, rect_size=8.0)
    ref = scenes.render(scenes.map_scene(oracle, **kw)).copy()
    assert int((ref[..., :3].max(axis=2) > 0).sum()) > width * height // 10, "the scene shows nothing"
    light_math(False)
    relaxed = scenes.render(scenes.map_scene(product, **kw)).copy()
    assert last_raster_kernel(product).endswith("_rl"), last_raster_kernel(product)
    assert_relaxed_bar(relaxed, ref, f"map, 16 lights, {width} x {height}")


ALPHAS = (0, 1, 127, 254, 255)


def cutout_texture():
    """8 x 8 texels, saturated green, alpha bytes 0 / 1 / 127 / 254 / 255 in turn (every byte in every row and column)"""
    img = np.zeros((8, 8, 4), np.uint8)
    img[..., 1] = 255
    yy, xx = np.mgrid[0:8, 0:8]
    img[..., 3] = np.array(ALPHAS, np.uint8)[(xx + 2 * yy) % 5]
    return B.Texture(img.reshape(-1), 8, 8)


def cutout_in_front_of_a_wall(api, with_cutout=True):
    """a wall at z = 6 and, two units in front of it, a quad whose texture is mostly holes; one point light between camera and quad"""
    wall = (scenes._batch_of_quads(api, [scenes._quad_wall(9, 6, -1, 6, 4.0)]).source(B.PixelSource.StaticTileIndex(0))
            .repeat_mode(B.REPEAT_REPEAT_XY).cull_mode(B.CULL_OFF).with_computed_normals())
    batches = [wall]
    if with_cutout:
        batches.append(scenes._batch_of_quads(api, [scenes._quad_wall(6, 4, 2, 4, 3.0)]).source(B.PixelSource.StaticTileIndex(1))
                       .repeat_mode(B.REPEAT_REPEAT_XY).cull_mode(B.CULL_OFF).with_computed_normals())
    scene = api.Scene.from_static([], batches).background(api.VGrayGradientShader())
    scene.lights([B.Light(B.LIGHT_POINT).with_position((4.5, 2.0, 1.5)).with_color((1.0, 0.9, 0.8)).with_intensity(2.0)
                  .with_start_distance(1.0).with_end_distance(12.0).compile()])
    assets = api.Assets.default().textures([B.Tile.from_texture(scenes.brick_texture(2)), B.Tile.from_texture(cutout_texture())])
    cam = api.D3FirstPCamera.new()
    cam.position = (4.0, 1.5, 0.0)
    cam.center = (4.0, 1.5, 1.0)

    def setup():
        v, p = cam.matrices(64.0, 64.0)
        return api.Rasterizer.setup(None, v, p).ambient((0.2, 0.2, 0.2, 1.0))

    return scenes._result(api, scene, assets, setup, 64, 64, 40, "cut-out in front of a wall")


def test_a_cutout_batch_keeps_the_texels_alpha_byte(oracle, product, light_math):
    """only texels of alpha 255 are written by the opaque pass (rasterizer.rs:1408); 254 is not.  The kernels read that byte from the
    texel instead of encoding texel / 255 again: coverage and alpha plane stay the oracle's in both modes"""
    ref = scenes.render(cutout_in_front_of_a_wall(oracle)).copy()
    bare = scenes.render(cutout_in_front_of_a_wall(oracle, with_cutout=False)).copy()
    green = (ref[..., 1].astype(np.int16) - ref[..., 0].astype(np.int16)) > 40  # (the wall is brick: red over green)
    assert green.any() and not ((bare[..., 1].astype(np.int16) - bare[..., 0].astype(np.int16)) > 40).any(), "the cut-out does not show"
    # the quad covers a block of pixels of which only the alpha-255 texels (a fifth) are written: holes inside its bounding box
    ys, xs = np.nonzero(green)
    box = green[ys.min():ys.max() + 1, xs.min():xs.max() + 1]
    assert 0.05 < box.mean() < 0.5, f"{box.mean():.2f} of the quad's box is written: the holes do not show"
    for exact in (True, False):
        light_math(exact)
        got = scenes.render(cutout_in_front_of_a_wall(product)).copy()
        assert last_raster_kernel(product).endswith("_rl") != exact, last_raster_kernel(product)
        what = f"cut-out, exact={exact}"
        (assert_exact_bar if exact else assert_relaxed_bar)(got, ref, what)
        assert np.array_equal(got[..., 3], ref[..., 3]), f"{what}: the alpha plane"
        got_green = (got[..., 1].astype(np.int16) - got[..., 0].astype(np.int16)) > 40
        assert np.array_equal(got_green, green), f"{what}: coverage differs at {np.argwhere(got_green != green)[:3].tolist()}"


def poisoned_projection(api, index, value):
    """the lit map (one point light) with ONE entry of the projection matrix replaced on its way into Rasterizer::setup
    (index "all": every entry multiplied by `value`)"""
    cfg = scenes.map_scene(api, width=160, height=96, n_lights=1, logo_size=16, rect_size=8.0)
    base = cfg.setup

    def setup():
        orig = api.Rasterizer.setup

        def patched(m2d, v, p):
            p = np.array(p, np.float32).copy()
            if index == "all":
                p *= np.float32(value)
            elif index is not None:
                p[index] = value
            return orig(m2d, v, p)

        api.Rasterizer.setup = staticmethod(patched)
        try:
            return base()
        finally:
            api.Rasterizer.setup = staticmethod(orig)

    cfg.setup = setup
    return cfg


def test_a_matrix_outside_the_window_falls_back(oracle, product, light_math):
    """an infinite, a NaN and a largest-float entry in the projection matrix: its inverse holds entries that are not finite or outside
    the division window -- the wave's w fails the window check and the wave takes the exact sequences -- and the frame stays the
    oracle's within the bar"""
    clean = scenes.render(poisoned_projection(oracle, None, 0.0)).copy()
    light_math(False)
    changed = 0
    for index, value in ((5, INF), (0, NAN), (14, FLT_MAX)):
        ref = scenes.render(poisoned_projection(oracle, index, value)).copy()
        changed += int(not np.array_equal(ref, clean))
        got = scenes.render(poisoned_projection(product, index, value)).copy()
        assert_relaxed_bar(got, ref, f"proj[{index}] = {value}")
    assert changed >= 2, "the poison does not arrive"
    # those three frames lose their 3D part altogether.  A fourth keeps it: the whole matrix times 2^-60 projects every vertex where it
    # was (clip coordinates and w scale alike) while the inverse's entries, 2^60 times larger, leave the window -- every lit fragment
    # of this frame is shaded through the fallback
    ref = scenes.render(poisoned_projection(oracle, "all", 2.0 ** -60)).copy()
    assert int((ref[..., :3].max(axis=2) > 0).sum()) > ref.shape[0] * ref.shape[1] // 10, "the scaled projection shows nothing"
    got = scenes.render(poisoned_projection(product, "all", 2.0 ** -60)).copy()
    assert last_raster_kernel(product).endswith("_rl")
    assert_relaxed_bar(got, ref, "proj * 2^-60")
    got = scenes.render(poisoned_projection(product, None, 0.0)).copy()  # ... and the next clean frame is the clean frame
    assert last_raster_kernel(product).endswith("_rl")
    assert_relaxed_bar(got, clean, "the clean frame after the poisoned ones")


def test_an_occluder_switches_the_relaxed_world_position_off(oracle, product, light_math):
    """get_occlusion compares the world position with the occluders' boxes: with one in the frame the relaxed kernels form the exact
    position (P.any_occluders), and the exact kernels are untouched"""
    def build(api):
        cfg = scenes.map_scene(api, width=160, height=96, n_lights=16, logo_size=16, rect_size=8.0)
        base = cfg.setup
        cfg.setup = lambda: base().mapmini_add_occluder((0.0, 9.0), (6.0, 15.0), 0.35)
        return cfg

    ref = scenes.render(build(oracle)).copy()
    plain = scenes.render(scenes.map_scene(oracle, width=160, height=96, n_lights=16, logo_size=16, rect_size=8.0)).copy()
    assert not np.array_equal(ref, plain), "the occluder darkens nothing"
    light_math(False)
    relaxed = scenes.render(build(product)).copy()
    assert last_raster_kernel(product).endswith("_rl"), last_raster_kernel(product)
    assert_relaxed_bar(relaxed, ref, "map with an occluder, relaxed")
    light_math(True)
    exact = scenes.render(build(product)).copy()
    assert not last_raster_kernel(product).endswith("_rl"), last_raster_kernel(product)
    assert_exact_bar(exact, ref, "map with an occluder")
