"""Sparse frames and the scratch state they leave behind.

A frame whose batch boxes reach only part of the screen is rastered over its row spans (rxr_upload_frame, k_spans_from_meshes): per tile
row the tile columns that the reference's own batch box test lets through (rxr_ref_tile_span).  The workgroups outside a row's span are
never launched or leave at once -- so they do not hand their bins back zeroed, and the invariant "bin_count is all zero between launches"
(rxr_device.h) holds only if the pre-pass never counts a triangle into such a bin.  A batch box is Rect {x: min, width: max - min}; in
float32 `x + width` can round below `max`, and the reference then skips the tile that `max` reaches into while the triangle's pixel box
still covers it.  The scenes below are built to have exactly that: a mesh across the left (top) screen edge whose right (bottom) end lies
one ulp past a tile boundary B.  rxr_debug_scratch reads the words the next launch assumes clear after every frame, BEFORE any later
frame could build on them; only when they are clean does a dense general-pipeline frame follow on the same context."""
import ctypes as C
import functools

import numpy as np
import pytest

import rusterix_amd
from rusterix_amd import binding as B
from rusterix_amd import scenes
from tests.routes import assert_route, last_raster_kernel

W = H = 480
BOUNDARY = 320            # a multiple of 16 (the device's bin tiles) and of every reference tile size below
TILE_SIZES = (16, 40, 64)
SCRATCH_BUFFERS = ("bin_count / blk_cnt", "3D counter set", "2D counter set", "bin2d_count")


# ---- helpers shared with the other sparse-frame tests ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _rxr():
    rxr = rusterix_amd.rxr_abi()
    return rxr


def context_of(product):
    return C.c_void_p(product.lib.rxh_context())


def scratch_state(product):
    """rxr_debug_scratch of the host mirror's context: [non-zero words, buffer, index, value of the first]"""
    out = (C.c_uint32 * 4)()
    assert _rxr().rxr_debug_scratch(context_of(product), out) == 0
    return list(out)


def assert_scratch_clean(product, what):
    s = scratch_state(product)
    assert s[0] == 0, (f"{what}: {s[0]} scratch words that the next launch assumes zero are not; first: {SCRATCH_BUFFERS[s[1]]} "
                       f"word {s[2]} = {s[3]}")


def content_info(product):
    info = (C.c_uint32 * 4)()
    assert _rxr().rxr_debug_content(context_of(product), info) == 0
    return list(info)


def bin_entries(product):
    """rxr_stats.n_bin_entries of the last frame: > 0 iff its 3D triangles went through the general count / scan / fill pipeline"""
    stats = (C.c_uint32 * 8)()   # rxr_stats: three floats, then n_triangles3d, n_triangles2d, n_bin_entries, tiles_x, tiles_y
    assert _rxr().rxr_get_stats(context_of(product), stats) == 0
    return stats[5]


def render_bands(product, cfg, bands):
    """one upload, then rxr_render_rows + rxr_download_rows per band; the scratch state is checked behind every band launch"""
    lib = product.lib
    r = cfg.setup()
    assert lib.rxh_rasterizer_upload(r._h, cfg.scene._h, cfg.width, cfg.height, cfg.tile_size, cfg.assets._h) == 0
    ctx = context_of(product)
    out = np.zeros((cfg.height, cfg.width, 4), np.uint8)
    for a, b in bands:
        assert _rxr().rxr_render_rows(ctx, a, b) == 0
        assert_scratch_clean(product, f"{cfg.name}: band [{a}, {b})")
        assert _rxr().rxr_download_rows(ctx, out.ctypes.data_as(C.POINTER(C.c_uint8)), a, b) == 0
    return out


def set_device_projection(product, on):
    product.lib.rxh_set_device_projection(1 if on else 0)


@pytest.fixture()
def projection(product):
    """set_device_projection(product, on) for the test; host projection again afterwards"""
    yield lambda on: set_device_projection(product, on)
    set_device_projection(product, False)


def assert_exact(got, ref, what):
    if not np.array_equal(got, ref):
        d = np.argwhere((got != ref).any(axis=2))
        y, x = d[0]
        raise AssertionError(f"{what}: {len(d)} pixels differ; first at (x={x}, y={y}): got {got[y, x]} want {ref[y, x]}")


# ---- the boundary scenes (built on the CPU) -------------------------------------------------------------------------------------
# Identity view and projection: a vertex (x, y, -0.5) lands on screen at ((x + 1) * W / 2, (1 - y) * H / 2), so one ulp of a world
# coordinate near the boundary moves the projected one by well under one ulp of B -- a walk by ulps visits every float around B.
def _to_world(sx, sy):
    return np.float32(sx / (W / 2) - 1.0), np.float32(1.0 - sy / (H / 2))


def _edge_mesh(axis, far, near):
    """two small triangles (48 bins at most each: neither goes to the general pipeline's list of large triangles): a sliver from world
    coordinate `far` (off screen) across the left (axis 0) or top (axis 1) screen edge, and one whose tip is at `near` (on screen, by the
    boundary); their pixel rows (columns) are 150..250 of the other axis"""
    along, across = (lambda p: _to_world(p, p)[axis]), (lambda p: _to_world(p, p)[1 - axis])
    a0, a1, a2, b0, b1 = across(198.0), across(200.0), across(202.0), across(190.0), across(210.0)
    inside, back = along(5.0), along(BOUNDARY - 30.0)
    tris = [(far, a0), (inside, a1), (far, a2), (back, b0), (near, a1), (back, b1)]
    z = np.float32(-0.5)   # (in front of the identity camera: the near plane is z = -0.1)
    return [(u, v, z) if axis == 0 else (v, u, z) for u, v in tris]


def _project_one(api, verts):
    v4 = np.concatenate([np.asarray(verts, np.float32), np.ones((len(verts), 1), np.float32)], axis=1)
    b = api.Batch3D.new(v4, np.arange(len(verts), dtype=np.uint32).reshape(-1, 3), np.zeros((len(verts), 2), np.float32))
    scene = api.Scene.from_static([], [b.with_computed_normals().cull_mode(B.CULL_OFF)])
    api.Rasterizer.setup(None, B.Mat4.identity(), B.Mat4.identity()).project(scene, W, H)
    p = scene.projected_batch3d(B.LIST_STATIC, 0)
    return p["projected_vertices"], p["bounding_box"]


def boundary_property(api, verts, axis):
    """(max, lo, extent, fl(lo + extent)) of the projected triangle on `axis`, and whether it is the case we want: the true maximum
    lies in (B, B + 4 ulp] and the reference's `x + width` does not pass B"""
    pv, bb = _project_one(api, verts)
    mx = np.float32(pv[:, axis].max())
    lo, ext = np.float32(bb[1 + axis]), np.float32(bb[3 + axis])
    hi = np.float32(lo + ext)
    ulp = np.spacing(np.float32(BOUNDARY))
    ok = bool(BOUNDARY < mx <= np.float32(BOUNDARY + 4 * ulp) and hi <= BOUNDARY and int(bb[0]) == 1)
    return (mx, lo, ext, hi), ok


@functools.lru_cache(maxsize=None)
def boundary_vertices(axis):
    """walk the far vertices (the rounding of max - min) and the near one (the maximum) by ulps until boundary_property holds"""
    api = rusterix_amd.load()
    sign = np.float32(1.0 if axis == 0 else -1.0)
    far = _to_world(-107.5, -107.5)[axis]   # (across the edge)
    for _ in range(400):
        near = _to_world(BOUNDARY, BOUNDARY)[axis]
        for _ in range(64):
            verts = _edge_mesh(axis, far, near)
            (mx, *_), ok = boundary_property(api, verts, axis)
            if ok:
                return tuple(map(tuple, verts))
            if mx > BOUNDARY + 4 * np.spacing(np.float32(BOUNDARY)):
                break
            near = np.nextafter(near, sign * np.float32(10.0))
        far = np.nextafter(far, sign * np.float32(10.0))
    raise AssertionError(f"no boundary triangle found on axis {axis}")


def _small_triangles(x0, y0, nx, ny, step_x, step_y, size):
    """nx * ny small screen-space triangles from (x0, y0), as world-space vertices"""
    verts = []
    for j in range(ny):
        for i in range(nx):
            sx, sy = x0 + i * step_x, y0 + j * step_y
            for dx, dy in ((0.0, 0.0), (size, 0.0), (0.0, size)):
                verts.append((*_to_world(sx + dx, sy + dy), -0.5))
    return verts


def _batch(api, verts, colour):
    v4 = np.concatenate([np.asarray(verts, np.float32), np.ones((len(verts), 1), np.float32)], axis=1)
    b = api.Batch3D.new(v4, np.arange(len(verts), dtype=np.uint32).reshape(-1, 3), np.zeros((len(verts), 2), np.float32))
    return b.with_computed_normals().cull_mode(B.CULL_OFF).source(B.PixelSource.Pixel(colour))


def boundary_scene(api, axis, tile_size):
    """axis 0: the edge mesh lies in pixel rows 190..210 and ends one ulp right of x = B; a batch of 160 small triangles in rows 350..440
    (tile rows of their own for every tile size, columns left of B) makes the frame bin.  axis 1: the edge mesh lies in columns 190..210
    and ends one ulp below y = B; the small triangles sit in rows 392..460, so that the tile rows from B to 383 lie inside the content
    band with empty spans.  Unlit constant colours: the bar is bit-exact."""
    if axis == 0:
        small = _small_triangles(40.0, 350.0, 16, 10, 15.0, 9.0, 7.0)
    else:
        small = _small_triangles(40.0, 392.0, 20, 8, 20.0, 8.5, 7.0)
    scene = api.Scene.from_static([], [_batch(api, boundary_vertices(axis), (230, 120, 40, 255)), _batch(api, small, (40, 160, 230, 255))])

    def setup():
        return api.Rasterizer.setup(None, B.Mat4.identity(), B.Mat4.identity()).ambient((1.0, 1.0, 1.0, 1.0))

    return scenes._result(api, scene, api.Assets.default(), setup, W, H, tile_size, f"boundary_{'xy'[axis]}_ts{tile_size}")


@pytest.mark.parametrize("axis", [0, 1])
def test_boundary_scenes_round_below_the_tile_boundary(oracle, axis):
    """CPU pin of the scenes the GPU tests rely on: the edge triangle's box, as the host mirror and the oracle project it, ends past B
    while the reference's `x + width` stays at or below B.  If projection arithmetic ever changes, this fails instead of the GPU tests
    quietly testing nothing."""
    prod = rusterix_amd.load()
    verts = boundary_vertices(axis)
    got, ok = boundary_property(prod, verts, axis)
    assert ok, got
    ref, ok_ref = boundary_property(oracle, verts, axis)
    assert ok_ref and [float(v) for v in ref] == [float(v) for v in got], (ref, got)
    # the device's pixel box reaches the 16-pixel tile column (row) from B on, the reference's tiles stop before it
    assert np.ceil(got[0]) == BOUNDARY + 1
    cfg = boundary_scene(prod, axis, 16)
    cfg.setup().project(cfg.scene, W, H)
    assert len(cfg.scene.projected_batch3d(B.LIST_STATIC, 1)["clipped_indices"]) > 128   # (with the edge triangle: a binned frame)
    for ts in TILE_SIZES:
        assert BOUNDARY % ts == 0 and BOUNDARY % 16 == 0


_DENSE = dict(n=12, width=W, height=H)


@functools.lru_cache(maxsize=None)
def _oracle_frame(kind, axis=0, tile_size=16):
    from tests.oracle_api import load_oracle

    o = load_oracle()
    cfg = scenes.box_grid_scene(o, **_DENSE) if kind == "dense" else boundary_scene(o, axis, tile_size)
    return scenes.render(cfg).copy()


@pytest.mark.gpu
@pytest.mark.parametrize("blockscan", ["default", "0"])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("tile_size", TILE_SIZES)
@pytest.mark.parametrize("axis", [0, 1], ids=["x", "y"])
def test_boundary_frames_leave_clean_scratch(product, projection, monkeypatch, axis, tile_size, device, blockscan):
    """The boundary scenes under row spans, whole frame and row bands: after every launch the words the next launch assumes zero are zero
    (checked before anything builds on them); then the frame equals the oracle's and the one without row spans; only then does a dense
    general-pipeline frame follow on the same context and equal the oracle's."""
    monkeypatch.setenv("RXR_CONTENT_MIN_TILES", "0")   # (row spans only pay from 8192 empty tiles on: this frame is small)
    if blockscan == "0":
        monkeypatch.setenv("RXR_BLOCKSCAN", "0")
    ref = _oracle_frame("boundary", axis, tile_size)
    projection(device)
    cfg = boundary_scene(product, axis, tile_size)
    got = scenes.render(cfg).copy()
    assert_scratch_clean(product, cfg.name)
    info = content_info(product)
    assert info[3] == (2 if device else 1), f"the frame did not take its row spans: {info}"
    assert_route(product, "k_raster_rows_sp", cfg.name)
    if blockscan == "0":
        assert bin_entries(product) > 0, "the frame did not go through the general pipeline"
    assert_exact(got, ref, f"{cfg.name} vs oracle")
    assert (got[..., :3].max(axis=2) > 0).mean() > 0.01
    monkeypatch.setenv("RXR_ROW_SPANS", "0")
    no_spans = scenes.render(cfg).copy()
    assert_scratch_clean(product, f"{cfg.name} without row spans")
    assert content_info(product)[3] == 0
    assert_route(product, "k_raster_rows", cfg.name + " without row spans")
    monkeypatch.delenv("RXR_ROW_SPANS")
    assert_exact(got, no_spans, f"{cfg.name}: row spans on vs off")
    bands = render_bands(product, cfg, [(0, 37), (37, BOUNDARY + 10), (BOUNDARY + 10, H)])
    assert_exact(bands, ref, f"{cfg.name}: row bands vs oracle")
    # only now, on clean scratch: a dense frame through the general pipeline on the same context
    monkeypatch.setenv("RXR_BLOCKSCAN", "0")
    projection(False)
    dense = scenes.render(scenes.box_grid_scene(product, **_DENSE)).copy()
    assert_scratch_clean(product, "dense frame")
    assert bin_entries(product) > 0
    assert_exact(dense, _oracle_frame("dense"), "dense general-pipeline frame after the sparse ones")


# ---- seeded sequences of sparse frames ----------------------------------------------------------------------------------------
def sparse_random_frame(api, seed, frame):
    """a random frame of 200..5000 triangles in clusters (test_gpu_fuzz.build's batches, grouped and moved so that the content covers
    part of the frame, some clusters across its edges), a random frame size of 320..960 pixels, tile size, 2D overlay"""
    from tests.test_gpu_fuzz import random_texture

    rng = np.random.default_rng([0x53504152, seed, frame])
    width, height = int(rng.integers(320, 961)), int(rng.integers(320, 961))
    tile_size = int(rng.choice([16, 32, 40, 64, 100]))
    textures = [B.Tile([random_texture(rng, int(rng.integers(1, 24)), int(rng.integers(1, 24)), int(rng.integers(0, 3)))]) for _ in range(3)]
    assets = api.Assets.default().textures(textures)
    scene = api.Scene.empty()
    n_total = int(rng.integers(200, 5001))
    n_batches = int(rng.integers(2, 7))
    cuts = np.sort(rng.integers(1, n_total, n_batches - 1))
    for nt in np.diff(np.concatenate([[0], cuts, [n_total]])):
        nt = max(int(nt), 1)
        centre = np.array([rng.uniform(-3.2, 3.2), rng.uniform(-2.2, 2.2), rng.uniform(-0.5, 0.5)], np.float32)
        spread = float(rng.uniform(0.1, 0.5))
        tri_c = centre + rng.normal(0.0, spread, size=(nt, 1, 3))
        verts = (tri_c + rng.normal(0.0, float(rng.uniform(0.02, 0.15)), size=(nt, 3, 3))).reshape(-1, 3).astype(np.float32)
        v4 = np.concatenate([verts, np.ones((len(verts), 1), np.float32)], axis=1)
        uv = (rng.random((nt * 3, 2)) * 3.0 - 1.0).astype(np.float32)
        b = api.Batch3D.new(v4, np.arange(nt * 3, dtype=np.uint32).reshape(nt, 3), uv).with_computed_normals()
        b.cull_mode(int(rng.integers(0, 3))).repeat_mode(int(rng.integers(0, 4)))
        kind = rng.integers(0, 3)
        if kind == 0:
            b.source(B.PixelSource.Pixel(tuple(int(x) for x in rng.integers(0, 256, 3)) + (255,)))
        else:
            b.source(B.PixelSource.StaticTileIndex(int(rng.integers(0, 3))))
        b.ambient_color(tuple(float(x) for x in rng.random(3) * 0.5))
        (scene.add_d3_static if rng.random() < 0.7 else scene.add_d3_dynamic)(b)
    lights = []
    for _ in range(int(rng.integers(0, 3)) if rng.random() < 0.4 else 0):
        l = B.Light(int(rng.integers(0, 6))).with_position(tuple(float(x) for x in rng.normal(0, 2, 3)))
        l.with_color(tuple(float(x) for x in rng.random(3))).with_intensity(float(rng.uniform(0.2, 3.0)))
        l.with_start_distance(float(rng.uniform(0.2, 2.0))).with_end_distance(float(rng.uniform(2.0, 8.0)))
        l.direction = tuple(float(x) for x in rng.normal(0, 1, 3))
        l.cone_angle = float(rng.uniform(0.2, 1.2))
        lights.append(l.compile())
    scene.lights(lights)
    overlay = int(rng.integers(0, 3))   # 0 none, 1 a few rectangles, 2 enough of them to bin the 2D primitives
    for _ in range((0, 3, 80)[overlay]):
        r = api.Batch2D.from_rectangle(float(rng.integers(0, width)), float(rng.integers(0, height)), float(rng.integers(2, 30)), float(rng.integers(2, 30)))
        r.source(B.PixelSource.Pixel(tuple(int(x) for x in rng.integers(0, 256, 3)) + (255,)))
        scene.add_d2_static(r)
    cam = api.D3OrbitCamera.new()
    cam.set_parameter_f32("distance", float(rng.uniform(4.0, 7.0)))
    cam.azimuth = float(np.float32(np.pi / 2))
    cam.elevation = 0.0
    sample = int(rng.integers(0, 2))
    amb = tuple(float(x) for x in rng.random(4)) if rng.random() < 0.8 else None

    def setup():
        ra = api.Rasterizer.setup(None, *cam.matrices(float(width), float(height))).sample_mode(sample)
        if amb is not None:
            ra.ambient(amb)
        return ra

    cfg = scenes._result(api, scene, assets, setup, width, height, tile_size, f"seq{seed}.{frame}")
    cfg.device = bool(rng.random() < 0.5)
    cfg.blockscan = bool(rng.random() < 0.5)
    return cfg


SEQ_BLOCKS, SEQ_PER_BLOCK = 8, 10   # 80 seeds


@pytest.mark.gpu
@pytest.mark.parametrize("block", range(SEQ_BLOCKS))
def test_sparse_frame_sequences(oracle, product, projection, monkeypatch, block):
    """SEQ_PER_BLOCK seeds, each a sequence of 4..6 random sparse frames on one context (frame size, tile size, host or device projection,
    RXR_BLOCKSCAN and the 2D overlay vary between frames), all under row spans.  After every frame the scratch state is clean, the frame
    equals itself without row spans bit for bit and the oracle within test_gpu_fuzz's bar.  Most frames must really have taken the row
    spans, and many the general pipeline: otherwise the test would pass without testing anything."""
    from tests.test_gpu_fuzz import TOLERANCE

    monkeypatch.setenv("RXR_CONTENT_MIN_TILES", "0")
    frames = with_spans = general = 0
    for seed in range(block * SEQ_PER_BLOCK, (block + 1) * SEQ_PER_BLOCK):
        n_frames = int(np.random.default_rng([0x53455153, seed]).integers(4, 7))
        for k in range(n_frames):
            what = f"seed {seed} frame {k}"
            ref = scenes.render(sparse_random_frame(oracle, seed, k)).copy()
            cfg = sparse_random_frame(product, seed, k)
            if cfg.blockscan:
                monkeypatch.delenv("RXR_BLOCKSCAN", raising=False)
            else:
                monkeypatch.setenv("RXR_BLOCKSCAN", "0")
            projection(cfg.device)
            got = scenes.render(cfg).copy()
            assert_scratch_clean(product, what)
            frames += 1
            with_spans += content_info(product)[3] != 0
            general += bin_entries(product) > 0
            if content_info(product)[3] != 0 and bin_entries(product) > 0:   # (a binned frame under row spans: a kernel that looks them up)
                assert last_raster_kernel(product) in ("k_raster_rows_sp", "k_raster_rows_rl_sp", "k_raster_rows_cut", "k_raster_rows_cut_rl"), what
            monkeypatch.setenv("RXR_ROW_SPANS", "0")
            no_spans = scenes.render(cfg).copy()
            monkeypatch.delenv("RXR_ROW_SPANS")
            assert_scratch_clean(product, what + " without row spans")
            assert_exact(got, no_spans, what + ": row spans on vs off")
            diff = np.abs(got.astype(np.int16) - ref.astype(np.int16)).max(axis=2)
            bad = np.argwhere(diff > TOLERANCE)
            assert len(bad) <= 3, f"{what}: {len(bad)} pixels off by more than {TOLERANCE}; first {bad[:3].tolist()}"
            assert (diff > 0).mean() < 0.02, f"{what}: {(diff > 0).sum()} pixels differ"
    assert with_spans * 2 >= frames, f"only {with_spans} of {frames} frames ran with row spans"
    assert general * 4 >= frames, f"only {general} of {frames} frames went through the general pipeline"
