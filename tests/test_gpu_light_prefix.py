"""The prefix loop of the relaxed light loop (shade3d_lights<LV, true>, rusterix_amd/csrc/rxr_kernels.hip): the leading run of lights with
a LightFast record is walked by a loop of its own, and the first light without a record -- or whose squared distance leaves the
exact-math window for a fragment -- and everything behind it go through the general loop.  RXR_LIGHT_PREFIX=0 (read per upload) sends
every light through the general loop, which is the parent's code.

For light lists that put the seam between the two loops at every place it can fall:
  * the relaxed frame with the prefix loop equals the relaxed frame under RXR_LIGHT_PREFIX=0, byte for byte;
  * both lie within one step per channel of the CPU oracle (the bar of tests/test_gpu_light_math.py for relaxed frames);
  * the exact-mode frame of the same list is the oracle's frame.

Frames: one lit quad facing the camera at 64 x 48 and 48 x 64 (12 tiles of 16 x 16; the quad leaves tiles empty and cuts through
others, so some waves hold no fragment and some hold a few) and the map scene at 64 x 48.

The light "on a fragment" stands on the quad's plane (the floor, in the map) where a pixel centre's ray meets it, rounded to float: the
nearest fragment is within a few ulp of it, the squared distance as small as a scene can make it.  Whether it falls below 2^-80 for a
fragment, so that the window test ends the run there, cannot be read back from a frame; the seam in the middle of a run is pinned by
the lights without a record."""
import math

import numpy as np
import pytest

from rusterix_amd import binding as B
from rusterix_amd import scenes
from tests.routes import last_raster_kernel
from tests.test_gpu_light_math import chunk_level_map, lit_box_grid
from tests.test_gpu_parity import _light

pytestmark = pytest.mark.gpu

TILE = 16
MISS = np.array([0, 0, 0, 255], np.uint8)
QUAD = (0.8, 0.7)     # half extents of the quad in the plane z = 0
CAM_Z = 2.2


# ---- the two scenes; a light position is given in the unit cube and placed in front of the scene's surfaces ---------------------------
def quad_cfg(api, width, height, lights):
    hx, hy = QUAD
    v = np.array([(-hx, -hy, 0, 1), (hx, -hy, 0, 1), (hx, hy, 0, 1), (-hx, hy, 0, 1)], np.float32)
    quad = (api.Batch3D.new(v, np.array([(0, 1, 2), (0, 2, 3)], np.uint32), np.array([(0, 0), (2, 0), (2, 1), (0, 1)], np.float32))
            .cull_mode(B.CULL_OFF).source(B.PixelSource.StaticTileIndex(scenes.MAP_TILES["brickwall"])).repeat_mode(B.REPEAT_REPEAT_XY)
            .with_computed_normals())
    scene = api.Scene.from_static([], [quad]).background(api.VGrayGradientShader())
    scene.lights(lights)
    assets = scenes.map_assets(api, 16)
    cam = api.D3FirstPCamera.new()
    cam.position = (0.0, 0.0, CAM_Z)
    cam.center = (0.0, 0.0, 0.0)

    def setup():
        view, proj = cam.matrices(float(width), float(height))
        return api.Rasterizer.setup(None, view, proj).ambient((0.05, 0.05, 0.05, 1.0))

    return scenes._result(api, scene, assets, setup, width, height, 40, "lit quad")


def quad_place(u, v, w):
    return (-QUAD[0] + 2 * QUAD[0] * u, -QUAD[1] + 2 * QUAD[1] * v, 0.25 + 0.9 * w)


def quad_on_fragment(width, height):
    """where the ray of the pixel centre right of and below the frame's middle meets the plane z = 0 (vertical field of view 75 degrees)"""
    t = math.tan(math.radians(75.0) / 2)
    x_ndc, y_ndc = 2 * (width // 2 + 0.5) / width - 1, 1 - 2 * (height // 2 + 0.5) / height
    return (float(np.float32(x_ndc * t * CAM_Z * width / height)), float(np.float32(y_ndc * t * CAM_Z)), 0.0)


def map_cfg(api, width, height, lights):
    cfg = scenes.map_scene(api, width=width, height=height, n_lights=1, logo_size=16, rect_size=8.0)
    cfg.scene.lights(lights)
    return cfg


def map_place(u, v, w):
    return (3.0 + 6.0 * u, 0.3 + 1.4 * v, 6.0 + 7.0 * w)


SCENES = {
    "quad 64 x 48": (lambda api, lights: quad_cfg(api, 64, 48, lights), quad_place, quad_on_fragment(64, 48)),
    "quad 48 x 64": (lambda api, lights: quad_cfg(api, 48, 64, lights), quad_place, quad_on_fragment(48, 64)),
    "map 64 x 48": (lambda api, lights: map_cfg(api, 64, 48, lights), map_place, (6.5, 0.0, 8.0)),
}


# ---- light lists: kind, position in the unit cube -------------------------------------------------------------------------------------
def _spread(n, seed):
    rng = np.random.default_rng(seed)
    return [tuple(float(x) for x in rng.random(3)) for _ in range(n)]


def fast(n, seed=5):
    return [("point", p) for p in _spread(n, seed)]


def with_slow_at(n, where, kind):
    out = fast(n, seed=11)
    out[where] = (kind, out[where][1])
    return out


LISTS = {
    "no light": [],
    "1 fast": fast(1),
    "5 fast": fast(5),
    "63 fast": fast(63),
    "64 fast": fast(64),
    "65 fast": fast(65),
    "130 fast": fast(130),
    "none with a record: spot, area, a point light with start == end": [("spot", (0.3, 0.5, 0.8)), ("area", (0.7, 0.4, 0.6)), ("point, start == end", (0.5, 0.6, 0.5))],
    "none with a record: a point light beyond the 1e9 guard sends the frame to the exact loop": fast(3) + [("point, far", (0.5, 0.5, 0.5))],
    "a spot light first": with_slow_at(6, 0, "spot"),
    "an area light in the middle": with_slow_at(7, 3, "area"),
    "a point light with start == end in the middle": with_slow_at(7, 4, "point, start == end"),
    "a spot light last": with_slow_at(6, 5, "spot"),
    "lights without a record at 0, 63, 64 and 129 of 130": [(("spot" if i in (0, 63, 64, 129) else "point"), p) for i, p in enumerate(_spread(130, 17))],
    "a light on a fragment in the middle": fast(3, seed=23) + [("on a fragment", None)] + fast(3, seed=29),
    "a light on a fragment first and last": [("on a fragment", None)] + fast(4, seed=31) + [("on a fragment", None)],
}


def build_lights(spec, place, on_fragment):
    n = max(len(spec), 1)
    intensity = min(1.5, 12.0 / n)   # (many lights: dim ones, the sum stays inside the byte range)
    out = []
    for k, (kind, p) in enumerate(spec):
        pos = on_fragment if kind == "on a fragment" else place(*p)
        col = (1.0 - 0.4 * ((k * 7) % 5) / 4, 0.6 + 0.4 * ((k * 3) % 4) / 3, 0.5 + 0.5 * ((k * 5) % 7) / 6)
        if kind in ("point", "on a fragment"):
            l = (B.Light(B.LIGHT_POINT).with_position(pos).with_color(col).with_intensity(intensity).with_start_distance(0.4).with_end_distance(3.5)
                 .with_flicker(0.3 if k % 4 == 1 else 0.0).compile())
        elif kind == "point, start == end":
            l = B.Light(B.LIGHT_POINT).with_position(pos).with_color(col).with_intensity(intensity).with_start_distance(2.5).with_end_distance(2.5).compile()
        elif kind == "point, far":
            l = (B.Light(B.LIGHT_POINT).with_position((pos[0] + 2.0e9, pos[1], pos[2])).with_color(col).with_intensity(intensity).with_start_distance(0.4)
                 .with_end_distance(3.5).compile())
        elif kind == "spot":
            l = _light(B.LIGHT_SPOT, pos, direction=(0.1, -0.2, -1.0), cone_angle=1.2, start=0.4, end=3.5, intensity=intensity)
        else:
            assert kind == "area", kind
            l = _light(B.LIGHT_AREA, pos, normal=(0.0, 0.0, -1.0), start=0.4, end=3.5, intensity=intensity, width=1.0, height=0.6)
        out.append(l)
    return out


def channel_diff(a, b):
    return np.abs(a.astype(np.int16) - b.astype(np.int16)).max(axis=2)


def assert_same(got, want, what):
    d = (got != want).any(axis=2)
    assert not d.any(), f"{what}: {int(d.sum())} pixels differ; first {np.argwhere(d)[:3].tolist()}: {got[tuple(np.argwhere(d)[0])].tolist()} against {want[tuple(np.argwhere(d)[0])].tolist()}"


def on_and_off(monkeypatch, make):
    """the frame with the prefix loop and the frame of the same scene uploaded under RXR_LIGHT_PREFIX=0"""
    with monkeypatch.context() as m:
        m.setenv("RXR_LIGHT_PREFIX", "0")
        off = scenes.render(make()).copy()
    return scenes.render(make()).copy(), off


@pytest.mark.parametrize("lights", list(LISTS))
@pytest.mark.parametrize("scene", list(SCENES))
def test_the_seam_between_the_two_loops(oracle, product, monkeypatch, scene, lights):
    make, place, on_fragment = SCENES[scene]
    ref = scenes.render(make(oracle, build_lights(LISTS[lights], place, on_fragment))).copy()
    monkeypatch.setenv("RXR_LIGHT_MATH", "relaxed")
    on, off = on_and_off(monkeypatch, lambda: make(product, build_lights(LISTS[lights], place, on_fragment)))
    kernel = last_raster_kernel(product)
    if "1e9 guard" in lights:   # (rxr_upload_frame sends the frame to the exact loop)
        assert kernel == "k_raster", kernel
    elif LISTS[lights]:
        assert kernel == "k_raster_rl", kernel
    assert_same(on, off, f"{scene}, {lights}: relaxed, prefix loop against RXR_LIGHT_PREFIX=0")
    d = channel_diff(on, ref)
    print(f"{scene}, {lights}: relaxed frame, {int((d > 0).sum())} pixels a step from the oracle, max {int(d.max())}")
    assert int(d.max()) <= 1, f"{scene}, {lights}: the relaxed frame is {int(d.max())} steps from the oracle"
    monkeypatch.setenv("RXR_LIGHT_MATH", "exact")
    exact = scenes.render(make(product, build_lights(LISTS[lights], place, on_fragment))).copy()
    assert last_raster_kernel(product) == "k_raster"
    assert_same(exact, ref, f"{scene}, {lights}: exact mode against the oracle")


@pytest.mark.parametrize("scene", ["quad 64 x 48", "quad 48 x 64"])
def test_the_quad_leaves_waves_without_a_fragment_and_waves_with_a_few(oracle, scene):
    make, place, on_fragment = SCENES[scene]
    ref = scenes.render(make(oracle, build_lights(LISTS["5 fast"], place, on_fragment)))
    hit = (ref != MISS).any(axis=2)
    tiles = hit.reshape(hit.shape[0] // TILE, TILE, hit.shape[1] // TILE, TILE).sum(axis=(1, 3))
    assert tiles.size == 12 and (tiles == 0).any() and ((tiles > 0) & (tiles < TILE * TILE)).any(), tiles.tolist()
    dark = scenes.render(make(oracle, []))
    assert int((ref[..., :3].astype(int).sum(axis=2) > dark[..., :3].astype(int).sum(axis=2) + 30).sum()) > hit.sum() // 4, "the lights reach nothing"


@pytest.mark.parametrize("name,build,kernel", [("lit box grid", lit_box_grid, "k_raster_rows_rl"), ("map behind the grid background", chunk_level_map, "k_raster_chunk_rl")])
def test_the_binned_and_the_chunk_level_kernels_carry_the_loop_too(product, monkeypatch, name, build, kernel):
    monkeypatch.setenv("RXR_LIGHT_MATH", "relaxed")
    on, off = on_and_off(monkeypatch, lambda: build(product))
    assert last_raster_kernel(product) == kernel
    assert_same(on, off, f"{name}: prefix loop against RXR_LIGHT_PREFIX=0")
