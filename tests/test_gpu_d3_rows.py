"""Small host-projected frames: rxr_upload_frame finds the tile rows that any 3D triangle can reach (rxr_tri_tile_rows over the set-up
records it has just built, rusterix_amd/csrc/rxr_device.h) and k_raster[_rl] skip the 3D passes of the workgroups outside them
(raster_tile, rxr_kernels.hip): such a tile is the miss colour plus whatever the 2D pass draws.

Every frame here is compared byte for byte with the SAME context's frame after an upload under RXR_D3_ROWS=0 (read per upload), in both
light modes; rxr_debug_d3_rows (binding: api.d3_rows()) proves that a range was found and which.  Exact light mode is compared with the
oracle as well; relaxed mode only with the switch-off frame (its distance to the oracle belongs to tests/test_gpu_light_math.py).

The frames are small: 64 x 48 (3 tile rows), 48 x 64, 64 x 80, 333 x 187 (the height is no multiple of the tile) and 640 x 360."""
import ctypes as C

import numpy as np
import pytest

import rusterix_amd
from rusterix_amd import binding as B
from rusterix_amd import scenes
from tests.test_gpu_host_setup import STAGE_TRIS, ctx_of, records, triangles_scene, upload
from tests.test_gpu_routes import knobs
from tests.test_gpu_special_inputs import build as special_build

pytestmark = pytest.mark.gpu

TILE = 16
MISS = np.array([0, 0, 0, 255], np.uint8)
RECT = 8   # side of the map scene's 2D logo rectangle here: inside the first tile, which the map's 3D part never reaches


def on_and_off(product, monkeypatch, make):
    """(frame, range) with the row range in use and (frame, range) of the same scene uploaded under RXR_D3_ROWS=0, same context"""
    with monkeypatch.context() as m:
        m.setenv("RXR_D3_ROWS", "0")
        off = scenes.render(make()).copy()
        off_rows = product.d3_rows()
    on = scenes.render(make()).copy()
    return on, product.d3_rows(), off, off_rows


def assert_same(got, want, what):
    d = (got != want).any(axis=2)
    assert not d.any(), f"{what}: {int(d.sum())} pixels differ; first {np.argwhere(d)[:3].tolist()}: {got[tuple(np.argwhere(d)[0])].tolist()} against {want[tuple(np.argwhere(d)[0])].tolist()}"


def rows_with_3d(frame, rect):
    """tile rows with a pixel outside the 2D rectangle's box [0, rect)^2 that is not the miss colour"""
    hit = (frame != MISS).any(axis=2)
    hit[:rect, :rect] = False
    return sorted({int(y) // TILE for y in np.nonzero(hit.any(axis=1))[0]})


# ---- the map scene (the flagship frame's scene) ------------------------------------------------------------------------------------
MAP_SIZES = [(64, 48), (333, 187), (640, 360)]
_oracle_frames = {}


def map_cfg(api, width, height):
    return scenes.map_scene(api, width=width, height=height, n_lights=16, logo_size=16, rect_size=float(RECT))


def oracle_map(oracle, width, height):
    if (width, height) not in _oracle_frames:
        frame = scenes.render(map_cfg(oracle, width, height)).copy()
        frame.setflags(write=False)
        _oracle_frames[width, height] = frame
    return _oracle_frames[width, height]


@pytest.mark.parametrize("light_math", ["exact", "relaxed"])
@pytest.mark.parametrize("width,height", MAP_SIZES)
def test_map_scene(oracle, product, monkeypatch, width, height, light_math):
    monkeypatch.setenv("RXR_LIGHT_MATH", light_math)
    on, rows, off, off_rows = on_and_off(product, monkeypatch, lambda: map_cfg(product, width, height))
    assert off_rows is None, f"RXR_D3_ROWS=0 must report all rows: {off_rows}"
    assert rows is not None, "no range was found for a small host-projected frame"
    n_rows = (height + TILE - 1) // TILE
    assert 0 < rows[0] < rows[1] <= n_rows, f"the room's walls end below the first tile row: the skip did not happen ({rows} of {n_rows} rows)"
    assert_same(on, off, f"map {width} x {height}, {light_math}")
    drawn = rows_with_3d(off, RECT)
    print(f"map {width} x {height}, {light_math}: range {rows}, rows with 3D pixels {drawn[:1]}..{drawn[-1:]} of {n_rows}")
    assert drawn and all(rows[0] <= r < rows[1] for r in drawn), f"rows {drawn} hold 3D pixels, the range is {rows}"
    # (the 2D rectangle lies wholly inside skipped rows, as the logo of the 4K frame does: it is drawn over the miss colour)
    assert RECT <= rows[0] * TILE and (on[:RECT, :RECT] != MISS).any(axis=2).all(), "the 2D rectangle over the skipped tile is missing"
    assert (on[:rows[0] * TILE, RECT:] == MISS).all() and (on[RECT:rows[0] * TILE, :RECT] == MISS).all()
    if light_math == "exact":
        ref = oracle_map(oracle, width, height)
        d = (on != ref).any(axis=2)
        print(f"map {width} x {height}, exact: {int(d.sum())} pixels differ from the oracle")
        assert_same(on, ref, f"map {width} x {height}, exact mode against the oracle")


# ---- triangles placed on the screen ------------------------------------------------------------------------------------------------
def placed_scene(api, width, height, triangles, rect=None, opacity=(), cull=B.CULL_OFF):
    """triangles given in PIXEL coordinates ([[x, y]] * 3 each), unprojected through the camera's matrices at a fixed depth; the ones
    whose index is in `opacity` go to a chunk's opacity list; `rect` = (x, y, w, h): a 2D rectangle on top"""
    cam = api.D3OrbitCamera.new()
    cam.set_parameter_f32("distance", 3.0)
    v, p = cam.matrices(float(width), float(height))
    proj = p.reshape(4, 4).T.astype(np.float64)   # (column-major: m[c * 4 + r])
    inv_view = np.linalg.inv(v.reshape(4, 4).T.astype(np.float64))
    scene = api.Scene.empty()
    chunk = scene.add_chunk() if opacity else None
    for k, tri in enumerate(triangles):
        world = []
        for (x, y) in tri:
            d = 2.0 - 0.05 * k   # depth in view space (later triangles nearer)
            q = inv_view @ np.array([(2.0 * x / width - 1.0) * d / proj[0, 0], (1.0 - 2.0 * y / height) * d / proj[1, 1], -d, 1.0])
            world.append(list(q[:3]) + [1.0])
        b = api.Batch3D.new(np.array(world, np.float32), np.array([[0, 1, 2]], np.uint32), np.array([[0, 0], [1, 0], [0, 1]], np.float32))
        b = b.with_computed_normals().cull_mode(cull)
        b.source(B.PixelSource.Pixel((200, 120, 40, 255)) if k not in opacity else B.PixelSource.StaticTileIndex(0)).repeat_mode(B.REPEAT_REPEAT_XY)
        if k in opacity:
            chunk.add_batch3d_opacity(b)
        else:
            scene.add_d3_static(b)
    if rect is not None:
        scene.add_d2_static(api.Batch2D.from_rectangle(*[float(c) for c in rect]).source(B.PixelSource.Pixel((250, 250, 10, 255))))
    assets = api.Assets.default().textures([B.Tile.from_texture(scenes.noise_texture(77, 8, 8))])

    def setup():
        return api.Rasterizer.setup(None, v, p).ambient((1.0, 1.0, 1.0, 1.0))

    return scenes._result(api, scene, assets, setup, width, height, 40, "placed triangles")


@pytest.mark.parametrize("light_math", ["exact", "relaxed"])
def test_one_triangle_in_the_middle_tile_row(oracle, product, monkeypatch, light_math):
    monkeypatch.setenv("RXR_LIGHT_MATH", light_math)
    tri = [[[10.0, 18.0], [40.0, 20.0], [22.0, 30.0]]]   # pixel rows 18 .. 30: tile row 1 of four
    on, rows, off, off_rows = on_and_off(product, monkeypatch, lambda: placed_scene(product, 48, 64, tri))
    assert off_rows is None and rows == (1, 2), (rows, off_rows)
    assert_same(on, off, "one triangle")
    assert (on[16:32] != MISS).any(), "the triangle is not drawn"
    assert (on[:16] == MISS).all() and (on[32:] == MISS).all(), "rows 0, 2 and 3 are not the miss colour"
    assert_same(on, scenes.render(placed_scene(oracle, 48, 64, tri)), "one triangle against the oracle")


def test_no_visible_triangle(product, monkeypatch):
    """the triangle culled (one of the two cull modes hides it, whichever way it faces): an empty range, the whole frame is the miss colour
    plus the 2D rectangle"""
    tri = [[[10.0, 18.0], [40.0, 20.0], [22.0, 30.0]]]
    empties = 0
    for cull in (B.CULL_BACK, B.CULL_FRONT):
        on, rows, off, off_rows = on_and_off(product, monkeypatch, lambda: placed_scene(product, 48, 64, tri, rect=(20, 40, 12, 9), cull=cull))
        assert off_rows is None and rows is not None, (rows, off_rows)
        assert_same(on, off, f"cull mode {cull}")
        if rows == (0, 0):
            empties += 1
            outside = np.ones((64, 48), bool)
            outside[39:50, 19:33] = False   # (the rectangle's pixels and one more all round)
            assert (on[outside] == MISS).all(), "nothing visible: a pixel outside the rectangle is not the miss colour"
            assert (on[41:48, 21:31] != MISS).any(axis=2).all(), "nothing visible: the 2D rectangle is missing"
        else:
            assert rows == (1, 2), rows
    assert empties == 1, "one cull mode must hide the triangle and the other show it"


@pytest.mark.parametrize("light_math", ["exact", "relaxed"])
def test_a_frame_with_an_opacity_list_batch(oracle, product, monkeypatch, light_math):
    """an opaque triangle in tile row 2 and a translucent one of a chunk's opacity list over rows 1 and 2: the range is the union"""
    monkeypatch.setenv("RXR_LIGHT_MATH", light_math)
    tris = [[[6.0, 36.0], [44.0, 34.0], [20.0, 46.0]], [[12.0, 20.0], [30.0, 22.0], [25.0, 44.0]]]
    make = lambda api: placed_scene(api, 48, 64, tris, opacity=(1,))  # noqa: E731
    on, rows, off, off_rows = on_and_off(product, monkeypatch, lambda: make(product))
    assert off_rows is None and rows == (1, 3), (rows, off_rows)
    assert_same(on, off, "opacity-list batch")
    assert (on[16:32] != MISS).any() and (on[:16] == MISS).all() and (on[48:] == MISS).all()
    assert_same(on, scenes.render(make(oracle)), "opacity-list batch against the oracle")


@pytest.mark.parametrize("light_math", ["exact", "relaxed"])
def test_poisoned_triangles(product, monkeypatch, light_math):
    """NaN, +-inf and huge numbers in one coordinate of a triangle after the other (tests/test_gpu_special_inputs.py): a NaN coefficient
    never rejects, so the tile rows of such a triangle's pixel box are inside the range; the frame does not change"""
    monkeypatch.setenv("RXR_LIGHT_MATH", light_math)
    make = lambda: special_build(product, B.SAMPLE_LINEAR, B.REPEAT_REPEAT_XY, False)  # noqa: E731
    on, rows, off, off_rows = on_and_off(product, monkeypatch, make)
    assert off_rows is None and rows is not None
    assert_same(on, off, "poisoned triangles")
    keep = upload(product, make())
    _, n, setup, _, _, _ = records(product)
    coef = setup[:, :9].view(np.float32)
    poisoned = 0
    for t in range(n):
        by = int(setup[t, 21])
        if np.isnan(coef[t]).any() and (by & 0xFFFF) < (by >> 16):
            poisoned += 1
            assert rows[0] <= (by & 0xFFFF) // TILE and ((by >> 16) + TILE - 1) // TILE <= rows[1], f"triangle {t}: box rows {by & 0xFFFF}..{by >> 16}, range {rows}"
    print(f"poisoned triangles: {poisoned} records with a NaN coefficient and a pixel box, range {rows}")
    assert poisoned > 0
    del keep


# ---- bands and stripes: the kernel's tile-row arithmetic ---------------------------------------------------------------------------
def render_rows(product, cfg, row0, row1):
    import torch

    rxr = rusterix_amd.rxr_abi()
    keep = upload(product, cfg)
    ctx = ctx_of(product)
    buf = torch.full((row1 - row0, cfg.width, 4), 9, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert rxr.rxr_render_rows_to(ctx, row0, row1, C.c_void_p(buf.data_ptr()), None) == 0, rxr.rxr_last_error(ctx)
    assert rxr.rxr_synchronize(ctx) == 0, rxr.rxr_last_error(ctx)
    del keep
    return buf.cpu().numpy()


@pytest.mark.parametrize("light_math", ["exact", "relaxed"])
def test_a_band_that_is_not_on_tile_rows(product, monkeypatch, light_math):
    monkeypatch.setenv("RXR_LIGHT_MATH", light_math)
    whole = scenes.render(map_cfg(product, 64, 48)).copy()
    assert product.d3_rows() is not None and product.d3_rows()[0] > 0
    band = render_rows(product, map_cfg(product, 64, 48), 5, 43)
    assert_same(band, whole[5:43], "rows 5..43 against the whole frame's")
    with monkeypatch.context() as m:
        m.setenv("RXR_D3_ROWS", "0")
        assert_same(band, render_rows(product, map_cfg(product, 64, 48), 5, 43), "rows 5..43 against the switch-off band")
    on_tiles = render_rows(product, map_cfg(product, 64, 48), 16, 48)
    assert_same(on_tiles, whole[16:48], "rows 16..48 against the whole frame's")


@pytest.mark.parametrize("n_ranks", [2, 3])
def test_compact_stripes_equal_the_whole_frame_s_slices(product, monkeypatch, n_ranks):
    """rxr_render_stripes_batch: launch tile row l is frame tile row first + l * stride, written to compact row l"""
    import torch

    monkeypatch.setenv("RXR_LIGHT_MATH", "relaxed")
    rxr = rusterix_amd.rxr_abi()
    W, H = 64, 80
    whole = scenes.render(map_cfg(product, W, H)).copy()
    rows = product.d3_rows()
    assert rows is not None and rows[0] > 0, rows
    keep = upload(product, map_cfg(product, W, H))
    ctx = ctx_of(product)
    n_stripes = (H + TILE - 1) // TILE
    for rank in range(n_ranks):
        mine = list(range(rank, n_stripes, n_ranks))
        frames = 2
        buf = torch.full((frames, len(mine) * TILE, W, 4), 9, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        assert rxr.rxr_render_stripes_batch(ctx, rank, n_ranks, frames, C.c_void_p(buf.data_ptr()), len(mine) * TILE * W * 4, None) == 0, rxr.rxr_last_error(ctx)
        assert rxr.rxr_synchronize(ctx) == 0, rxr.rxr_last_error(ctx)
        got = buf.cpu().numpy()
        for k in range(frames):
            for j, s in enumerate(mine):
                assert_same(got[k, j * TILE:(j + 1) * TILE], whole[s * TILE:(s + 1) * TILE], f"rank {rank} of {n_ranks}, frame {k}, stripe {s}")
    del keep


# ---- frames that keep "all rows" ---------------------------------------------------------------------------------------------------
def test_frames_without_host_records_report_all_rows(product, monkeypatch):
    """more than RXR_STAGE_TRIS triangles (binned), a device-projected small frame and RXR_HOST_SETUP=0: no range, the same frames"""
    on, rows, off, _ = on_and_off(product, monkeypatch, lambda: triangles_scene(product, STAGE_TRIS + 1))
    assert rows is None, rows
    assert_same(on, off, "129 triangles")
    want = scenes.render(map_cfg(product, 64, 48)).copy()
    assert product.d3_rows() is not None
    product.lib.rxh_set_device_projection(1)
    try:
        on, rows, off, _ = on_and_off(product, monkeypatch, lambda: map_cfg(product, 64, 48))
    finally:
        product.lib.rxh_set_device_projection(0)
    assert rows is None, rows
    assert_same(on, off, "device-projected map")
    with knobs(product, monkeypatch, ctx_env={"RXR_HOST_SETUP": "0"}):
        on, rows, off, _ = on_and_off(product, monkeypatch, lambda: map_cfg(product, 64, 48))
    assert rows is None, rows
    assert_same(on, off, "RXR_HOST_SETUP=0")
    assert_same(on, want, "RXR_HOST_SETUP=0 against the frame with the range in use")
