"""Every raster kernel variant pinned to a parity test that proves it ran.

rxr_launch_raster_grid (rxr_kernels.hip) picks one of twenty raster kernels from the facts rxr_upload.hip's RasterParams phase computes, and
rxr_jit_launch puts two more in front of it.  `rxr_debug_last_raster_kernel` reports the symbol name of the kernel a context launched last;
ROUTES below maps every kernel name to a scene that carries what that instantiation specialises on, the knobs that send it there and the
bar its frame has to meet.  Four kinds of test hang off the one table:

  (a) route-pinned parity: the route is asserted BY NAME, then the frame is compared with the oracle's;
  (b) cross-route identity: one scene through every kernel that can legally draw it, all frames equal (lit: equal within an arithmetic mode);
  (c) seeded fuzz per forced route (build and build_chunks(dense=40) of tests/test_gpu_fuzz.py, build of tests/test_gpu_rows.py);
  (d) a census: the k_raster* definitions of rxr_kernels.hip are exactly the names of the table (no exclusions).

What can be checked without a GPU is: the census's parsing half, that every route scene shows the feature it is for (on the oracle's frame
alone) and that the fuzz seeds can take their routes.  Those tests carry no gpu mark.

RXR_SMALL_MODE and RXR_MIN_KERNEL_LEVEL are read by rxr_create: such cases replace the host mirror's context by a fresh one (created under
the variable, destroyed and replaced again in a `finally`), one at a time, in this process.  The frames here are uploaded through the host
mirror (Rasterizer.rasterize), which owns its context: a context made with rxr_create beside it would never see them, so the mirror's own
is the one that has to be created under the variable.  Dropping it loses nothing a later test relies on -- the mirror forgets what it had
made resident with it (drop_context_locked) and every test uploads its own scene, textures and programs."""
import contextlib
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from rusterix_amd import binding as B
from rusterix_amd import scenes
from rusterix_amd.binding import Program
from tests.routes import assert_route, last_raster_kernel  # noqa: F401

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOLERANCE = 1            # tests/test_gpu_fuzz.py: lit fragments go through log2 / exp2 / rsq
MAX_BEYOND = 3           # ... and a handful of pixels may sit on a rounding boundary
MISS = (0, 0, 0, 255)    # what the 3D pass leaves where no fragment is written
STAGE_TRIS = 128         # RXR_STAGE_TRIS (rxr_device.h): more triangles than this and the frame is binned


# ---- asking which kernel ran ----------------------------------------------------------------------------------------------------
def _recreate_context(product):
    """drops the host mirror's context (rusterix_host.cpp set_devices / set_device); the next frame creates one: rxr_create reads
    RXR_SMALL_MODE, RXR_MIN_KERNEL_LEVEL"""
    product.lib.rxh_set_devices((C.c_int * 2)(0, 0), 2)
    product.lib.rxh_set_device(0)


@contextlib.contextmanager
def knobs(product, monkeypatch, env=None, ctx_env=None):
    """per-frame variables `env` and create-time variables `ctx_env` (a context of its own for the block); everything is put back"""
    with monkeypatch.context() as m:
        for k, v in {**(ctx_env or {}), **(env or {})}.items():
            m.setenv(k, v)
        if ctx_env:
            _recreate_context(product)
        try:
            yield
        finally:
            if ctx_env:
                for k in ctx_env:
                    m.delenv(k, raising=False)
                _recreate_context(product)


def assert_parity(got, ref, tol, what):
    if tol == "exact":
        d = (got != ref).any(axis=2)
        assert not d.any(), f"{what}: {int(d.sum())} pixels differ; first {np.argwhere(d)[:3].tolist()}"
        return
    diff = np.abs(got.astype(np.int16) - ref.astype(np.int16)).max(axis=2)
    print(f"{what}: max |diff| {int(diff.max())}, pixels off by one {int((diff == 1).sum())}, beyond {int((diff > TOLERANCE).sum())}")
    bad = np.argwhere(diff > TOLERANCE)
    assert len(bad) <= MAX_BEYOND, f"{what}: {len(bad)} pixels off by more than {TOLERANCE}; first {bad[:3].tolist()}"


# ---- the scenes -----------------------------------------------------------------------------------------------------------------
def _texture(rng, w, h, holes):
    img = rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8)
    cut = rng.random((h, w)) < 0.45          # (drawn either way: the twin without holes is the same picture but for them)
    img[..., 3] = np.where(cut & holes, 0, 255)
    return B.Texture(img.reshape(-1), w, h)


COLOUR = ["Color", "UV", ("Push", 3.0), "Mul", "Fract", "Mul", ("Push", 1.3), "Mul", "SetColor"]           # exact opcodes only
OPACITY = ["UV", ("Push", 5.0), "Mul", "Fract", ("GetComponents", [0]), ("Push", 0.5), "Gt",
           ("If", [("Push", 1.0), "SetOpacity"], [("Push", 0.4), "SetOpacity"])]                            # decides visibility
CALL = [["Color", "UV", ("FunctionCall", 1, 1, 1), "Mul", "SetColor"], [("LoadLocal", 0), ("Push", 3.0), "Mul", "Fract", ("Push", 1.3), "Mul"]]


def program(kind):
    """'static' | 'static+opacity' | 'calls' | 'calls+opacity': what rxr_upload.hip's kernel levels 2..5 tell apart"""
    if kind is None:
        return None
    opacity = OPACITY if kind.endswith("+opacity") else []
    if kind.startswith("calls"):
        return Program([opacity + CALL[0], CALL[1]])
    return Program([opacity + COLOUR])


def point_lights(rng, n, centre=(0.0, 0.0, 1.2), spread=1.4, end=6.0, huge=False):
    out = []
    for k in range(n):
        pos = tuple(float(c + x) for c, x in zip(centre, rng.uniform(-spread, spread, 3) * (1.0, 0.7, 0.4)))
        l = B.Light(B.LIGHT_POINT).with_position(pos).with_color(tuple(float(x) for x in 0.4 + 0.6 * rng.random(3)))
        l.with_intensity(float(rng.uniform(0.8, 2.0))).with_start_distance(float(rng.uniform(0.3, 1.0))).with_end_distance(float(rng.uniform(0.6, 1.0) * end))
        if huge and k == 0:
            l.with_end_distance(2.0e9)   # beyond the 1e9 window of the fused light term: the whole frame takes the exact loop
        out.append(l.compile())
    return out


def cloud_scene(api, width=203, height=131, n_tris=500, size=0.09, spread=1.2, lights=0, huge_light=False, holes=False, pane=False,
                terrain=False, baked=False, prog=None, wall=True, overlay=True, overlay_at=None, seed=1):
    """A cloud of small triangles (tests.test_gpu_rows.small_triangles) in front of a textured wall, seen through a perspective camera:
    mesh A twice (exact depth ties, texture / colour), mesh B with the texture that has holes when `holes`, mesh C with a profile id (and,
    with `pane`, an opacity-pass pane of that id in front); `terrain` / `baked`: two chunk meshes with the terrain texture sampled by world
    position and a baked shader texture; `prog`: meshes A and B run that program; a textured and a translucent 2D rectangle on top."""
    from tests.test_gpu_rows import small_triangles

    rng = np.random.default_rng([0x52585231, 2222, seed])
    assets = api.Assets.default().textures([B.Tile([_texture(rng, 16, 16, False)]), B.Tile([_texture(rng, 13, 9, holes)]), B.Tile([_texture(rng, 32, 32, False)])])
    scene = api.Scene.empty()
    shader = scene.add_program(program(prog)) if prog else None
    n_triangles = 0

    def mesh(nt, depth=0.5):
        nonlocal n_triangles
        n_triangles += nt
        v4, idx, uv = small_triangles(rng, nt, size, spread, depth)
        return lambda: api.Batch3D.new(v4.copy(), idx.copy(), uv.copy()).with_computed_normals().cull_mode(B.CULL_OFF)

    if wall:
        v = np.array([[-7, -5, -1.9, 1], [7, -5, -1.9, 1], [7, 5, -1.9, 1], [-7, 5, -1.9, 1]], np.float32)
        b = api.Batch3D.new(v, np.array([[0, 1, 2], [0, 2, 3]], np.uint32), np.array([[0, 0], [9, 0], [9, 6], [0, 6]], np.float32)).with_computed_normals().cull_mode(B.CULL_OFF)
        scene.add_d3_static(b.source(B.PixelSource.StaticTileIndex(2)).repeat_mode(B.REPEAT_REPEAT_XY).ambient_color((0.5, 0.5, 0.6)))
        n_triangles += 2
    a = mesh(n_tris)
    n_triangles += n_tris
    for copy, source in enumerate((B.PixelSource.StaticTileIndex(0), B.PixelSource.Pixel((230, 60, 40, 255)))):
        b = a().source(source).repeat_mode(B.REPEAT_REPEAT_XY).ambient_color((0.9, 0.8, 0.7))
        if shader is not None and copy == 0:
            b.shader(shader)
        scene.add_d3_static(b)
    b = mesh(max(n_tris // 2, 1))().source(B.PixelSource.StaticTileIndex(1)).repeat_mode(B.REPEAT_REPEAT_XY).ambient_color((0.7, 0.9, 0.8))
    if shader is not None:
        b.shader(shader)
    scene.add_d3_static(b)
    c = mesh(max(n_tris // 4, 1))().source(B.PixelSource.Pixel((40, 170, 220, 255))).profile_id(3)
    chunk = scene.add_chunk() if (pane or terrain or baked) else None
    if terrain:
        chunk.terrain(_texture(rng, 24, 20, holes), origin=(-2, -1), size=3)
        chunk.terrain_batch3d(mesh(max(n_tris // 4, 1))().source(B.PixelSource.Terrain()))
    if baked:
        s = chunk.add_shader(Program([["Color", "SetColor"]]), _texture(rng, 16, 16, holes))
        chunk.add_batch3d(mesh(max(n_tris // 4, 1))().source(B.PixelSource.Pixel((255, 255, 255, 255))).repeat_mode(B.REPEAT_REPEAT_XY).shader(s))
    if pane:
        # (the opacity batch comes BEFORE the opaque one with the profile id in submission order: chunk batches precede the scene's own)
        p = np.array([[-1.3, -0.8, 1.1, 1], [1.3, -0.8, 1.1, 1], [1.3, 0.8, 1.1, 1], [-1.3, 0.8, 1.1, 1]], np.float32)
        pb = api.Batch3D.new(p, np.array([[0, 1, 2], [0, 2, 3]], np.uint32), np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float32)).with_computed_normals().cull_mode(B.CULL_OFF)
        chunk.add_batch3d_opacity(pb.source(B.PixelSource.Pixel((90, 160, 250, 120))).profile_id(3))
        n_triangles += 2
    scene.add_d3_static(c)
    if lights:
        scene.lights(point_lights(np.random.default_rng([7, seed, lights]), lights, huge=huge_light))
    if overlay:
        # (`overlay_at`: the two rectangles' corners; by default one by the top-left corner and one across the bottom-right corner of the frame)
        (ax, ay), (bx, by) = overlay_at or ((5.0, 7.0), (float(width - 50), float(height - 30)))
        scene.add_d2_static(api.Batch2D.from_rectangle(ax, ay, 37.0, 23.0).source(B.PixelSource.StaticTileIndex(0)).repeat_mode(B.REPEAT_REPEAT_XY))
        scene.add_d2_static(api.Batch2D.from_rectangle(bx, by, 60.0, 40.0).source(B.PixelSource.Pixel((250, 240, 30, 140))))
    cam = api.D3OrbitCamera.new()
    cam.set_parameter_f32("distance", 3.0)
    cam.azimuth = float(np.float32(np.pi / 2))
    cam.elevation = 0.1

    def setup():
        v, p = cam.matrices(float(width), float(height))
        return api.Rasterizer.setup(None, v, p).ambient((0.7, 0.65, 0.6, 1.0))

    return scenes._result(api, scene, assets, setup, width, height, 40, "route-cloud", n_triangles=n_triangles, n_lights=lights)


SPARSE_W, SPARSE_H = 250, 150            # 16 x 10 tiles, the last column and row partial
SPAN_END_A, SPAN_END_B = 16 * 9, 16 * 13


def sparse_span_ends(width=SPARSE_W):
    """the tile boundaries the two sheets of sparse_scene end next to, for a frame `width` pixels wide: (144, 208) at the default 250"""
    return 16 * int(9 * width / SPARSE_W), 16 * int(13 * width / SPARSE_W)


def sparse_scene(api, lights=0, overlay=True, width=SPARSE_W, height=SPARSE_H):
    """Identity view and projection (a vertex (x, y, z) lands at ((x + 1) W / 2, (1 - y) H / 2)): two sheets of small triangles.  Sheet A
    fills pixel rows 4..60 and ends one pixel LEFT of the tile boundary x = 144, sheet B fills rows 84..148 and ends one pixel RIGHT of
    x = 208; tile row 4 (pixels 64..79) is reached by nothing.  Under row spans the raster grid of rows 0..3 ends at column 9 and that of
    rows 5..9 at column 14.  Every sheet is two layers of different depths, layer 0 of sheet A submitted twice (exact ties).
    `width`, `height`: every pixel position above scaled by width / 250 and height / 150 (the same number of triangles, each as much
    larger), but for the two sheet ends, which stay one pixel left and right of a tile boundary (sparse_span_ends); the defaults give the
    250 x 150 scene float for float (every factor is then 1.0)."""
    W, H = width, height
    kx, ky = W / SPARSE_W, H / SPARSE_H
    end_a, end_b = sparse_span_ends(W)
    rng = np.random.default_rng([0x52585231, 3333])
    scene = api.Scene.empty()
    assets = api.Assets.default().textures([B.Tile([_texture(rng, 16, 16, False)])])
    n_triangles = 0

    def sheet(x0, y0, x1, y1, step, shift, z_lo):
        verts = []
        xs, ys = np.arange(x0, x1, step * kx), np.arange(y0, y1, step * ky)
        for sy in ys:
            for sx in xs:
                z = float(rng.uniform(z_lo, z_lo + 0.2))
                ax, ay = min(sx + shift * kx, x1), min(sy + shift * ky, y1)
                bx, by = min(sx + (shift + step) * kx, x1), min(sy + (shift + step) * ky, y1)
                for px, py in ((ax, ay), (bx, ay), (ax, by), (bx, ay), (bx, by), (ax, by)):
                    verts.append((px / (W / 2) - 1.0, 1.0 - py / (H / 2), z))
        v = np.asarray(verts, np.float32)
        v4 = np.concatenate([v, np.ones((len(v), 1), np.float32)], axis=1)
        uv = (rng.random((len(v), 2)) * 2.0).astype(np.float32)
        return lambda: api.Batch3D.new(v4.copy(), np.arange(len(v), dtype=np.uint32).reshape(-1, 3), uv.copy()).with_computed_normals().cull_mode(B.CULL_OFF), len(v) // 3

    for first, (x0, y0, x1, y1) in ((True, (10.0 * kx, 4.0 * ky, end_a - 1.0, 60.0 * ky)), (False, (100.0 * kx, 84.0 * ky, end_b + 1.0, 148.0 * ky))):
        for layer, (shift, z_lo) in enumerate(((0.0, -0.6), (3.0, -0.9))):
            make, nt = sheet(x0, y0, x1, y1, 7.0, shift, z_lo)
            copies = 2 if (layer == 0 and first) else 1
            for c in range(copies):
                src = B.PixelSource.StaticTileIndex(0) if c == 0 else B.PixelSource.Pixel((220, 50, 60, 255))
                scene.add_d3_static(make().source(src).repeat_mode(B.REPEAT_REPEAT_XY).ambient_color((0.8, 0.9, 0.7)))
                n_triangles += nt
    if lights:
        scene.lights(point_lights(np.random.default_rng([9, lights]), lights, centre=(-0.1, 0.0, -0.2), spread=0.9, end=2.5))
    if overlay:
        scene.add_d2_static(api.Batch2D.from_rectangle(20.0 * kx, 10.0 * ky, 41.0 * kx, 27.0 * ky).source(B.PixelSource.Pixel((250, 240, 30, 140))))
        scene.add_d2_static(api.Batch2D.from_rectangle(120.0 * kx, 100.0 * ky, 33.0 * kx, 21.0 * ky).source(B.PixelSource.StaticTileIndex(0)))

    def setup():
        return api.Rasterizer.setup(None, B.Mat4.identity(), B.Mat4.identity()).ambient((0.6, 0.6, 0.6, 1.0))

    return scenes._result(api, scene, assets, setup, W, H, 16, "route-sparse", n_triangles=n_triangles)


# ---- the route table ------------------------------------------------------------------------------------------------------------
# kernel name -> (scene builder taking `api` and twin arguments, per-frame knobs, create-time knobs, tolerance class, feature).  `feature`
# names the twin whose oracle frame must differ from the scene's (what the instantiation specialises on must show in the picture).
def _route(build, env=None, ctx_env=None, tol="exact", feature=None, **kw):
    return dict(build=functools.partial(build, **kw), env=env or {}, ctx_env=ctx_env or {}, tol=tol, feature=feature, kw=kw)


SMALL = dict(n_tris=28, size=0.45)       # 2 + 28 * 2 + 14 + 7 = 79 triangles: one staging round, no binning
INTERP = {"RXR_SHADER_JIT": "0"}
SPANS = {"RXR_CONTENT_MIN_TILES": "0"}   # (row spans only pay from 8192 empty tiles on: these frames are small)
CUT = dict(holes=True, pane=True)
CHUNK = dict(terrain=True, baked=True)

ROUTES = {
    "k_raster": _route(cloud_scene, **SMALL, width=171, height=107),
    "k_raster_rl": _route(cloud_scene, **SMALL, width=171, height=107, lights=2, tol="lit", feature="lights"),
    "k_raster_fused": _route(cloud_scene, **SMALL, width=171, height=107, lights=1, ctx_env={"RXR_SMALL_MODE": "1"}, tol="lit", feature="lights"),
    "k_raster_rows": _route(cloud_scene),
    "k_raster_rows_rl": _route(cloud_scene, lights=5, tol="lit", feature="lights"),
    "k_raster_rows_sp": _route(sparse_scene, env=SPANS, feature="sparse"),
    "k_raster_rows_rl_sp": _route(sparse_scene, env=SPANS, lights=3, tol="lit", feature="sparse+lights"),
    "k_raster_rows_cut": _route(cloud_scene, **CUT, width=219, height=140, feature="holes"),
    "k_raster_rows_cut_rl": _route(cloud_scene, **CUT, width=219, height=140, lights=7, tol="lit", feature="holes+lights"),
    "k_raster_pair": _route(cloud_scene, env={"RXR_PAIR_TILES": "1"}, holes=True, feature="odd rows"),          # 131 rows: 9 tile rows
    "k_raster_pair_rl": _route(cloud_scene, env={"RXR_PAIR_TILES": "1"}, height=99, lights=1, tol="lit", feature="odd rows+lights"),   # 7 tile rows
    "k_raster_chunk": _route(cloud_scene, **CHUNK, width=187, height=123, feature="chunk"),
    "k_raster_chunk_rl": _route(cloud_scene, **CHUNK, width=187, height=123, lights=16, tol="lit", feature="chunk+lights"),
    "k_raster_chunk_cut": _route(cloud_scene, **CHUNK, **CUT, width=187, height=123, feature="chunk+holes"),
    "k_raster_chunk_cut_rl": _route(cloud_scene, **CHUNK, **CUT, width=187, height=123, lights=12, tol="lit", feature="chunk+holes+lights"),
    "k_raster_vm": _route(cloud_scene, env=INTERP, prog="calls+opacity", lights=2, tol="lit", feature="program+lights"),
    "k_raster_vm_s": _route(cloud_scene, env=INTERP, prog="static+opacity", feature="program"),
    "k_raster_vm_sv": _route(cloud_scene, env=INTERP, prog="static", terrain=True, lights=3, tol="lit", feature="program+chunk+lights"),   # (frame_needs_chunk_paths)
    "k_raster_vm_p": _route(cloud_scene, env=INTERP, prog="static", feature="program"),
    "k_raster_vm_v": _route(cloud_scene, env=INTERP, prog="calls", holes=True, feature="program+holes"),
    "k_raster_jit": _route(cloud_scene, env={"RXR_SHADER_JIT": "1"}, prog="static", feature="program"),
    "k_raster_jit_cut": _route(cloud_scene, env={"RXR_SHADER_JIT": "1"}, prog="static", holes=True, lights=4, tol="lit", feature="program+holes+lights"),
}
# no route is excluded: every kernel of the default build is reachable (the census below fails on a kernel without an entry)
EXCLUDED = {}

TWINS = {"lights": dict(lights=0), "holes": dict(holes=False), "chunk": dict(terrain=False, baked=False), "program": dict(prog=None)}


@functools.lru_cache(maxsize=None)
def _oracle_frame(name, twin=None, overlay=True):
    from tests.oracle_api import load_oracle

    r = ROUTES[name]
    kw = dict(r["kw"], overlay=overlay)
    if twin:
        kw.update({k: v for k, v in TWINS[twin].items() if k in kw or r["build"].func is cloud_scene})
    return scenes.render(r["build"].func(load_oracle(), **kw)).copy()


# ---- (d) census, and what the oracle alone can say about the scenes ---------------------------------------------------------------
def kernels_in_source():
    text = open(os.path.join(ROOT, "rusterix_amd", "csrc", "rxr_kernels.hip")).read()
    return set(re.findall(r'^extern "C" __global__ void [^\n{]*?\b(k_raster\w*)\(RasterParams', text, flags=re.M))   # (the #if twins share a name)


def test_census_every_raster_kernel_has_a_route():
    names = kernels_in_source()
    assert len(names) == 22 and "k_raster_jit_cut" in names and "k_raster" in names, sorted(names)
    assert not EXCLUDED
    assert names == set(ROUTES), f"without a route-pinned test: {sorted(names - set(ROUTES))}; routes without a kernel: {sorted(set(ROUTES) - names)}"


def test_the_dispatcher_names_its_kernels_in_one_place():
    """every raster launch of rxr_launch_raster_grid goes through RXR_RASTER, which returns the launched kernel's own token as the name"""
    text = open(os.path.join(ROOT, "rusterix_amd", "csrc", "rxr_kernels.hip")).read()
    body = text[text.index('extern "C" const char *rxr_launch_raster_grid(const RasterParams *P, uint32_t grid_x, hipStream_t s) {'):]
    body = body[:body.index("#undef RXR_RASTER")]
    assert set(re.findall(r"RXR_RASTER\((k_raster\w*),", body)) == set(ROUTES) - {"k_raster_jit", "k_raster_jit_cut"}
    assert not re.findall(r"RXR_LAUNCH\(k_raster", body) and '"k_raster' not in body
    assert "rxr_debug_last_raster_kernel" not in open(os.path.join(ROOT, "include", "rxr.h")).read()   # test-only: not part of the ABI


@pytest.mark.parametrize("name", sorted(ROUTES))
def test_route_scene_shows_what_its_kernel_is_for(name):
    """on the oracle's frame alone: partial edge tiles, at least a fifth of the frame covered by 3D fragments, and the route's feature"""
    r = ROUTES[name]
    frame = _oracle_frame(name)
    h, w = frame.shape[:2]
    assert w % 16 and h % 16 and w <= 256 and h <= 160
    bare = _oracle_frame(name, overlay=False)
    covered = (bare != np.array(MISS, np.uint8)).any(axis=2).mean()
    assert covered >= 0.2, f"{name}: 3D fragments cover {covered:.1%} of the frame"
    assert (frame != bare).any(axis=2).mean() > 0.01, "the 2D overlay does not show"
    from tests.oracle_api import load_oracle

    cfg = r["build"](load_oracle())
    small = name in ("k_raster", "k_raster_rl", "k_raster_fused")
    assert (cfg.n_triangles <= STAGE_TRIS) == small, f"{name}: {cfg.n_triangles} triangles"
    for part in (r["feature"] or "").split("+"):
        if part in TWINS:
            changed = (frame != _oracle_frame(name, twin=part)).any(axis=2).mean()
            assert changed > 0.01, f"{name}: without its {part} the frame changes in {changed:.2%} of the pixels only"
        elif part == "odd rows":
            assert ((h + 15) // 16) % 2 == 1
        elif part == "sparse":
            rows = [(bare[y:y + 16] != np.array(MISS, np.uint8)).any() for y in range(0, h, 16)]
            assert not rows[4] and rows[3] and rows[5], rows
            # geometry one pixel either side of a span end: sheet A stops short of x = 144, sheet B reaches past x = 208
            hit = (bare != np.array(MISS, np.uint8)).any(axis=2)
            assert hit[4:60, SPAN_END_A - 2].any() and not hit[4:60, SPAN_END_A:].any()
            assert hit[84:148, SPAN_END_B].any() and not hit[84:148, SPAN_END_B + 1:].any()
    if "holes" in (r["feature"] or ""):
        # pixels where what lies behind shows through a hole: the cut-out mesh's own colours are gone there, the frame is not the miss colour
        solid = _oracle_frame(name, twin="holes")
        through = (frame != solid).any(axis=2) & (frame != np.array(MISS, np.uint8)).any(axis=2)
        assert through.mean() > 0.005


# ---- (a) route-pinned parity ------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", sorted(ROUTES))
def test_route_pinned_parity(product, monkeypatch, name):
    r = ROUTES[name]
    ref = _oracle_frame(name)
    with knobs(product, monkeypatch, r["env"], r["ctx_env"]):
        got = scenes.render(r["build"](product)).copy()
        assert_route(product, name, name)
    assert_parity(got, ref, r["tol"], name)


@gpu
@pytest.mark.parametrize("name", ["k_raster_rl", "k_raster_rows_rl", "k_raster_rows_cut_rl", "k_raster_chunk_rl"])
def test_a_light_beyond_the_window_demotes_the_frame_to_the_exact_kernel(oracle, product, monkeypatch, name):
    """a light parameter beyond 1e9 (here: an end distance of 2e9) sends the frame to the kernel without the relaxed light loop"""
    r = ROUTES[name]
    build = functools.partial(r["build"], huge_light=True)
    with knobs(product, monkeypatch, r["env"], r["ctx_env"]):
        got = scenes.render(build(product)).copy()
        assert_route(product, name[:-3], f"{name} with a light beyond the window")
    assert_parity(got, scenes.render(build(oracle)), "lit", name + " demoted")


# ---- (b) cross-route identity -----------------------------------------------------------------------------------------------------
LADDER = [   # (expected kernel in exact arithmetic / without lights, per-frame knobs, create-time knobs, takes the relaxed light loop)
    ("k_raster", {"RXR_NO_ROWS": "1"}, {}, True),
    ("k_raster_rows", {}, {}, True),
    ("k_raster_pair", {"RXR_PAIR_TILES": "1"}, {}, True),
    ("k_raster_rows_cut", {"RXR_FORCE_SPLIT_ROUNDS": "1"}, {}, True),
    ("k_raster_rows_sp", SPANS, {}, True),
    ("k_raster_chunk", {}, {"RXR_MIN_KERNEL_LEVEL": "1"}, True),
    ("k_raster_vm", {}, {"RXR_MIN_KERNEL_LEVEL": "2"}, False),
]


def ladder_scene(api, lights=0):
    """more than 128 small triangles in the middle of the frame (the row spans leave the margins out), no wall, no cut-outs, no chunks.  The 2D
    rectangles lie inside the cloud's box: the row spans take the UNION box of the 2D primitives (rxr_upload.hip d2_box), and two rectangles
    in opposite corners of the frame would make every span the whole row."""
    return cloud_scene(api, width=235, height=147, n_tris=420, size=0.13, spread=0.55, lights=lights, wall=False, seed=5,
                       overlay_at=((60.0, 40.0), (100.0, 70.0)))


def rl_name(name):
    return {"k_raster": "k_raster_rl", "k_raster_rows_sp": "k_raster_rows_rl_sp"}.get(name, name + "_rl")


@gpu
def test_unlit_scene_is_the_same_frame_through_every_route(oracle, product, monkeypatch):
    ref = scenes.render(ladder_scene(oracle)).copy()
    assert (ref != np.array(MISS, np.uint8)).any(axis=2).mean() > 0.15
    for name, env, ctx_env, _ in LADDER:
        with knobs(product, monkeypatch, env, ctx_env):
            got = scenes.render(ladder_scene(product)).copy()
            assert_route(product, name, f"ladder {env or ctx_env or 'default'}")
        assert_parity(got, ref, "exact", f"unlit ladder through {name}")


@gpu
def test_lit_scene_is_the_same_frame_through_every_route_of_an_arithmetic_mode(oracle, product, monkeypatch):
    ref = scenes.render(ladder_scene(oracle, lights=4)).copy()
    assert (ref != scenes.render(ladder_scene(oracle))).any(axis=2).mean() > 0.03, "the lights change nothing"
    frames = {"exact": {}, "relaxed": {}}
    for mode in ("exact", "relaxed"):
        for name, env, ctx_env, takes_relaxed in LADDER:
            if mode == "relaxed" and not takes_relaxed:
                continue
            expected = rl_name(name) if mode == "relaxed" else name
            with knobs(product, monkeypatch, dict(env, RXR_LIGHT_MATH=mode), ctx_env):
                frames[mode][expected] = scenes.render(ladder_scene(product, lights=4)).copy()
                assert_route(product, expected, f"lit ladder, {mode}")
    for mode, by_name in frames.items():
        first_name, first = next(iter(by_name.items()))
        for name, frame in by_name.items():
            assert_parity(frame, first, "exact", f"{mode}: {name} against {first_name}")
        assert_parity(first, ref, "lit", f"{mode} against the oracle")
    # (every frame of a mode equals that mode's first, asserted above: the bound between rows and rows_rl is the bound between any two routes)
    between = np.abs(frames["exact"]["k_raster_rows"].astype(np.int16) - frames["relaxed"]["k_raster_rows_rl"].astype(np.int16))
    assert int(between.max()) <= TOLERANCE, f"the two arithmetic modes differ by {int(between.max())}"


# ---- (c) seeded fuzz per forced route ---------------------------------------------------------------------------------------------
def recording(api):
    """`api` with Scene / Chunk / Batch3D that note what a generator submits: per 3D batch its triangles, list, source kind, profile id and
    shader; per chunk which shaders are baked; the lights.  cfg.scene.facts() sums that up: the counts cannot_take decides from."""
    import types

    class Batch3D(api.Batch3D):
        @staticmethod
        def new(vertices, indices, uvs):
            b = api.Batch3D.new(vertices, indices, uvs)
            b.__class__ = Batch3D
            b.rec = dict(tris=len(indices), off=False, profile=False, shader=None, list=None, chunk=None)
            return b

        def source(self, src):
            self.rec["off"] = src is B.PixelSource.Off or src.kind == B.PixelSource.Off.kind
            return super().source(src)

        def profile_id(self, pid):
            self.rec["profile"] = True
            return super().profile_id(pid)

        def shader(self, idx):
            self.rec["shader"] = idx
            return super().shader(idx)

    class Chunk(api.Chunk):
        def _note(self, b, kind):
            b.rec.update(list=kind, chunk=self)
            self._scene.batches.append(b.rec)

        def add_batch3d(self, b):
            self._note(b, "opaque")
            return super().add_batch3d(b)

        def add_batch3d_opacity(self, b):
            self._note(b, "opacity")
            return super().add_batch3d_opacity(b)

        def terrain_batch3d(self, b):
            self._note(b, "opaque")
            return super().terrain_batch3d(b)

        def add_shader(self, program, baked_texture=None, **kw):
            self.baked.append(baked_texture is not None)
            return super().add_shader(program, baked_texture, **kw)

    class Scene(api.Scene):
        @staticmethod
        def empty():
            s = Scene()
            s.batches, s.n_lights = [], 0
            return s

        def add_chunk(self):
            c = super().add_chunk()
            c.__class__ = Chunk
            c.baked = []
            return c

        def add_d3_static(self, b):
            b.rec.update(list="opaque")
            self.batches.append(b.rec)
            return super().add_d3_static(b)

        def add_d3_dynamic(self, b):
            b.rec.update(list="opaque")
            self.batches.append(b.rec)
            return super().add_d3_dynamic(b)

        def lights(self, lights):
            self.n_lights += len(lights)
            return super().lights(lights)

        def facts(self):
            """active: 3D batches with triangles and a source; triangles: theirs; programs: batches whose program would run (a chunk
            shader that is not baked in the opaque pass, any chunk shader in the opacity pass: rasterizer.rs:1226-1304, :1642-1667)"""
            live = [r for r in self.batches if r["tris"] and not r["off"]]
            runs = [r for r in live if r["shader"] is not None and r["chunk"] is not None and r["shader"] < len(r["chunk"].baked)
                    and (r["list"] == "opacity" or not r["chunk"].baked[r["shader"]])]
            return dict(active=len(live), triangles=sum(r["tris"] for r in live), lights=self.n_lights, programs=len(runs),
                        profiled=sum(r["profile"] for r in live), opacity=sum(r["list"] == "opacity" for r in live))

    return types.SimpleNamespace(**{**vars(api), "Scene": Scene, "Chunk": Chunk, "Batch3D": Batch3D})


def _soup(api, seed):
    from tests.test_gpu_fuzz import build

    return build(recording(api), seed, 163 + 16 * (seed % 3), 101 + 7 * (seed % 4))


def _chunks(api, seed):
    from tests.test_gpu_fuzz import build_chunks

    return build_chunks(recording(api), seed, 171, 107, dense=40)


def _rows(variant):
    def build(api, seed):
        from tests.test_gpu_rows import build as rows_build

        return rows_build(recording(api), seed, 203 + 16 * (seed % 3), 131 + 9 * (seed % 3), variant)
    return build


INTERP_DYNAMIC = {"RXR_SHADER_JIT": "0", "RXR_VM_NO_STATIC": "1"}
# forced route -> (generator, per-frame knobs, create-time knobs, seeds, bar).  tests.test_gpu_fuzz.build: 1..4 soups of 1..39 triangles across
# the near plane, 0..5 lights of every type, no chunks, no programs -- the small-frame kernels.  build_chunks(dense=40): chunks with terrain
# and baked textures, opacity lists, profile ids, programs, 0..2 point lights, hundreds of triangles -- the binned chunk and interpreter
# kernels; which of them a frame takes by itself depends on what is on screen, so the knobs pin what the generator's counts cannot:
# RXR_NO_SPLIT_ROUNDS / RXR_FORCE_SPLIT_ROUNDS the cut variant, RXR_LIGHT_MATH the arithmetic, RXR_VM_NO_STATIC + RXR_VM_VIS_CALLS the
# interpreter level.  tests.test_gpu_rows.build: 2..4 unlit meshes of 150..699 small triangles (its own bar: exact).
# The seeds were picked on the CPU from the generators' counts (test_fuzz_seeds_can_take_their_routes): at most 2 of 8 cannot take the route.
FUZZ = {
    "k_raster": (_soup, {"RXR_LIGHT_MATH": "exact"}, {}, (301, 302, 304, 306, 307, 308, 309, 310), "lit"),
    "k_raster_rl": (_soup, {}, {}, (351, 355, 356, 357, 358, 359, 360, 363), "lit"),
    "k_raster_fused": (_soup, {}, {"RXR_SMALL_MODE": "1"}, (400, 401, 402, 404, 405, 406, 408, 409), "lit"),
    "k_raster_chunk_rl": (_soup, {}, {"RXR_MIN_KERNEL_LEVEL": "1"}, (450, 454, 455, 456, 457, 459, 460, 461), "lit"),
    "k_raster_chunk": (_chunks, {"RXR_SHADER_JIT": "0", "RXR_NO_SPLIT_ROUNDS": "1", "RXR_LIGHT_MATH": "exact"}, {"RXR_MIN_KERNEL_LEVEL": "1"},
                       (401, 406, 408, 413, 421, 423, 424, 425), "lit"),
    "k_raster_chunk_cut_rl": (_chunks, {"RXR_SHADER_JIT": "0", "RXR_FORCE_SPLIT_ROUNDS": "1"}, {"RXR_MIN_KERNEL_LEVEL": "1"},
                              (503, 511, 516, 517, 522, 525, 528, 530), "lit"),
    "k_raster_vm": (_chunks, dict(INTERP_DYNAMIC, RXR_VM_VIS_CALLS="1"), {"RXR_MIN_KERNEL_LEVEL": "2"}, (420, 421, 422, 423, 424, 425, 426, 427), "lit"),
    "k_raster_vm_v": (_chunks, INTERP_DYNAMIC, {}, (600, 601, 605, 607, 609, 611, 612, 614), "lit"),
    "k_raster_rows": (_rows("plain"), {}, {}, range(10, 18), "exact"),
    "k_raster_rows_cut": (_rows("mixed"), {}, {}, range(10, 18), "exact"),
    "k_raster_pair": (_rows("ties"), {"RXR_PAIR_TILES": "1"}, {}, range(10, 18), "exact"),
    "k_raster_chunk_cut": (_rows("cutout"), {}, {"RXR_MIN_KERNEL_LEVEL": "1"}, range(10, 18), "exact"),
}
SMALL_ROUTES = ("k_raster", "k_raster_rl", "k_raster_fused", "k_raster_chunk_rl")   # (k_raster_chunk_rl: here fed with small frames)


def cannot_take(route, facts):
    """the reason why a scene with these counts (recording.facts) cannot take `route` (None: it can).  Clipping at the near plane can make
    two triangles of one, and a batch off screen is dropped: a frame is counted as small up to 64 submitted triangles and as binned from
    256 on; what lies in between is not used for a route that depends on the side."""
    if facts["active"] == 0:
        return "no 3D batch active"
    if route in SMALL_ROUTES and facts["triangles"] > STAGE_TRIS // 2:
        return f"{facts['triangles']} triangles: may pass the small-scene threshold once clipped"
    if route not in SMALL_ROUTES and route != "k_raster_vm" and facts["triangles"] < 2 * STAGE_TRIS:
        return f"{facts['triangles']} triangles: too few to be sure of the small-scene threshold"
    if route.endswith("_rl") and facts["lights"] == 0:
        return "no lights"
    if route.startswith("k_raster_chunk") and facts["programs"]:
        return f"{facts['programs']} batches run a program: an interpreter kernel's frame"
    if route == "k_raster_vm_v" and facts["programs"] < 2:
        return "fewer than two batches run a program (one may be off screen)"
    return None


def _fuzz_cases():
    return [pytest.param(route, seed, id=f"{route}-{seed}") for route, (_, _, _, seeds, _) in FUZZ.items() for seed in seeds]


def test_fuzz_seeds_can_take_their_routes(oracle):
    for route, (build, _, _, seeds, _) in FUZZ.items():
        why = {seed: cannot_take(route, build(oracle, seed).scene.facts()) for seed in seeds}
        skipped = {s: w for s, w in why.items() if w}
        assert len(why) == 8 and len(skipped) <= 2, f"{route}: {skipped}"


@gpu
@pytest.mark.parametrize("route, seed", _fuzz_cases())
def test_fuzz_through_a_forced_route(oracle, product, monkeypatch, route, seed):
    build, env, ctx_env, _, bar = FUZZ[route]
    cfg = build(product, seed)
    why = cannot_take(route, cfg.scene.facts())
    if why:
        pytest.skip(f"{route} seed {seed}: {why}")
    ref = scenes.render(build(oracle, seed)).copy()
    with knobs(product, monkeypatch, env, ctx_env):
        got = scenes.render(cfg).copy()
        assert_route(product, route, f"{route} seed {seed}")
    assert_parity(got, ref, bar, f"{route} seed {seed}")
