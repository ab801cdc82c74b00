"""Resident chunk textures on the GPU (include/rxr.h: rxr_set_chunk_textures, rxr_update_chunk_textures(_to), rxr_read_chunk_texture;
kernel k_chunk_tex_commit in rusterix_amd/csrc/rxr_chunk_tex.hip).

The pool: every byte and every flag against numpy, through both forms, at the sizes and positions at which the kernel changes path
(derived from the constants it exports).  Refusals change nothing.  Frames: a frame whose chunk textures are resident is BYTE-IDENTICAL
to the frame that carries them (which the existing tests hold to the oracle) and is drawn by the same kernel.  The mirror:
Scene.resident_chunk_textures and Terrain.rebuild_chunk_textures against scenes built from scratch."""
import ctypes as C

import numpy as np
import pytest

import rusterix_amd
from rusterix_amd import binding as B
from rusterix_amd import scenes
from rusterix_amd.abi import RXR_ERR_INVALID, RXR_ERR_UNSUPPORTED, RXR_OK, rxr_chunk as Chunk, rxr_frame as Frame, rxr_texture as Tex
from tests.test_gpu_bake import CHECKER
from tests.test_gpu_chunks import floor_quad, terrain_texture

pytestmark = pytest.mark.gpu
W, H = 208, 144


def constants():
    out = (C.c_uint32 * 3)()
    rusterix_amd.rxr_abi().rxr_debug_chunk_tex_constants(out)
    return dict(launch=out[0], segment=out[1], grid_x=out[2])


def texels(tag, w, h, opaque=True):
    """[h * w] RGBA8 as uint8 [h * w * 4]: random colours, alpha 255 or (opaque False) random"""
    rng = np.random.default_rng([0x43544558, tag])
    a = rng.integers(0, 256, size=(w * h, 4), dtype=np.uint8)
    if opaque:
        a[:, 3] = 255
    return a.reshape(-1)


def flag_of(data):
    return int((data.reshape(-1, 4)[:, 3] == 255).all())


class Pool:
    """a context of its own with a registration of `sizes`, one chunk naming slot 0; a numpy model of the pool next to it"""

    def __init__(self, handle=None):
        self.rxr = rusterix_amd.rxr_abi()
        self.own = handle is None
        self.ctx = C.c_void_p(handle) if handle else C.c_void_p()
        if self.own:
            assert self.rxr.rxr_create(C.byref(self.ctx), 0) == RXR_OK
        self.sizes, self.model = [], []

    def close(self):
        if self.own and self.ctx:
            self.rxr.rxr_destroy(self.ctx)
        self.ctx = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def error(self):
        return (self.rxr.rxr_last_error(self.ctx) or b"").decode()

    def register(self, sizes, data, expect=RXR_OK, n_chunks=1):
        """data[i]: uint8 bytes or None (a reserved slot)"""
        tex = (Tex * max(len(sizes), 1))()
        keep = [None if d is None else np.ascontiguousarray(d, np.uint8) for d in data]
        for t, (w, h), d in zip(tex, sizes, keep):
            t.rgba, t.width, t.height = (None if d is None else d.ctypes.data), w, h
        terrain = np.array([0 if sizes else -1] * n_chunks, np.int32)
        first = np.zeros(n_chunks + 1, np.uint32)
        rc = self.rxr.rxr_set_chunk_textures(self.ctx, C.cast(tex, C.c_void_p), len(sizes), terrain.ctypes.data, first.ctypes.data, None, n_chunks)
        assert rc == expect, (rc, self.error())
        if rc == RXR_OK:
            self.sizes = list(sizes)
            self.model = [np.zeros(w * h * 4, np.uint8) if d is None else d.copy() for (w, h), d in zip(sizes, keep)]
        return rc

    def read(self, slot):
        size, flag = (C.c_uint32 * 2)(), C.c_uint32(7)
        assert self.rxr.rxr_read_chunk_texture(self.ctx, slot, size, C.byref(flag), None) == RXR_OK, self.error()
        data = np.full(size[0] * size[1] * 4, 0xA5, np.uint8)
        assert self.rxr.rxr_read_chunk_texture(self.ctx, slot, None, None, data.ctypes.data) == RXR_OK, self.error()
        return (size[0], size[1]), flag.value, data

    def snapshot(self):
        return [self.read(s) for s in range(len(self.sizes))]

    def assert_matches_model(self, label=""):
        for s, (size, flag, data) in enumerate(self.snapshot()):
            assert size == tuple(self.sizes[s]), (label, s, size)
            bad = np.flatnonzero(data != self.model[s])
            assert bad.size == 0, f"{label}: slot {s} ({size}): {bad.size} bytes differ, first at byte {bad[:3].tolist()}"
            assert flag == flag_of(self.model[s]), f"{label}: slot {s} ({size}): flag {flag}, numpy says {flag_of(self.model[s])}"

    def update(self, slots, sources, form, expect=RXR_OK):
        slots = np.ascontiguousarray(slots, np.uint32)
        blob = np.concatenate([np.ascontiguousarray(s, np.uint8) for s in sources]) if len(sources) else np.zeros(4, np.uint8)
        if form == "host":
            rc = self.rxr.rxr_update_chunk_textures(self.ctx, slots.ctypes.data, len(slots), blob.ctypes.data)
        else:
            import torch

            s = torch.cuda.Stream()
            with torch.cuda.stream(s):     # written on that stream just before the call: the call must order itself behind it
                dev = torch.from_numpy(blob).to("cuda").clone()
            rc = self.rxr.rxr_update_chunk_textures_to(self.ctx, slots.ctypes.data, len(slots), dev.data_ptr(), s.cuda_stream)
            torch.cuda.synchronize()
        assert rc == expect, (rc, self.error())
        if rc == RXR_OK:
            for k, src in zip(slots, sources):
                self.model[int(k)] = np.ascontiguousarray(src, np.uint8).copy()
        return rc


SIZES = [(1, 1), (3, 5), (64, 64), (257, 129), (512, 512)]


@pytest.mark.parametrize("form", ["host", "device"])
def test_pool_round_trip_mixed_sizes_named_in_descending_order(form):
    K = constants()
    assert 512 * 512 > 2 * K["segment"], "the largest slot is meant to span several segments"
    with Pool() as p:
        poison = [texels(100 + i, w, h, opaque=False) for i, (w, h) in enumerate(SIZES)]
        p.register(SIZES, poison)
        p.assert_matches_model("registration")
        # [4, 1, 0]: 512 x 512 (16-byte body, several segments), then 3 x 5 at a 16-byte aligned source (three 16-byte groups and a tail
        # of three texels), then 1 x 1 at a source that is only 4-byte aligned (15 texels lie in front of it).  Slots 2 and 3 are not named.
        p.update([4, 1, 0], [texels(200, 512, 512), texels(201, 3, 5, opaque=False), texels(202, 1, 1)], form)
        p.assert_matches_model("update [4, 1, 0]")
        # [3, 2]: 257 x 129 = 33153 texels (eight full segments, then 96 16-byte groups and a tail of one), then 64 x 64 -- exactly one
        # segment -- at a source that is only 4-byte aligned
        p.update([3, 2], [texels(203, 257, 129), texels(204, 64, 64, opaque=False)], form)
        p.assert_matches_model("update [3, 2]")
        p.update([2], [texels(205, 64, 64)], form)     # translucent -> opaque: the flag follows
        p.assert_matches_model("update [2]")


@pytest.mark.parametrize("form", ["host", "device"])
def test_the_flag_sees_one_translucent_texel_wherever_it_lies(form):
    """one slot per position of the single texel with alpha 254; n = 2 segments + 7 texels, so the last segment is one 16-byte group
    and a tail of three.  The sources lie back to back with n odd, so their alignment cycles through 0, 12, 8, 4 bytes: the order is
    rotated four times and every position meets the 16-byte path and the dword path."""
    seg = constants()["segment"]
    n = 2 * seg + 7
    positions = [None, 0, n - 1, n - 2, n - 3, seg - 1, seg, 2 * seg - 1, 2 * seg, 2 * seg + 3, 2 * seg + 4]
    sizes = [(n, 1)] * len(positions)

    def source(k, salt):
        d = texels(300 + 16 * salt + k, n, 1).copy()
        if positions[k] is not None:
            d[4 * positions[k] + 3] = 254
        return d

    with Pool() as p:
        p.register(sizes, [source(k, 0) for k in range(len(positions))])
        p.assert_matches_model("registration")
        assert [p.read(k)[1] for k in range(len(positions))] == [1] + [0] * (len(positions) - 1)
        for rot in range(1, 5):
            order = list(np.roll(np.arange(len(positions)), rot))
            p.update(order, [source(k, rot) for k in order], form)
            p.assert_matches_model(f"rotation {rot}")
        p.update([3], [texels(399, n, 1)], form)      # ... and back to opaque
        p.assert_matches_model("opaque again")
        assert p.read(3)[1] == 1


def test_three_hundred_slots_cross_the_launch_cut_and_a_reserved_slot_is_zero():
    K = constants()
    n = 300
    assert K["launch"] < n < 2 * K["launch"]
    sizes = [(2, 2)] * n + [(5, 3)]
    data = [texels(400 + i, 2, 2, opaque=i % 3 != 0) for i in range(n)] + [None]
    with Pool() as p:
        p.register(sizes, data)
        assert p.rxr.rxr_debug_chunk_tex_launches(p.ctx) == 2
        p.assert_matches_model("registration")
        size, flag, zeros = p.read(n)
        assert size == (5, 3) and flag == 0 and not zeros.any(), "a slot without bytes reads back as zeros, not opaque"
        order = list(range(n))[::-1]
        p.update(order, [texels(800 + i, 2, 2, opaque=i % 5 != 0) for i in order], "device")
        assert p.rxr.rxr_debug_chunk_tex_launches(p.ctx) == 2
        p.assert_matches_model("update of 300")
        p.update([n], [texels(999, 5, 3)], "host")
        p.assert_matches_model("the reserved slot written")


def test_refusals_change_nothing():
    import torch

    with Pool() as p:
        sizes = [(8, 8), (3, 5), (64, 64)]
        p.register(sizes, [texels(500 + i, w, h, opaque=i != 1) for i, (w, h) in enumerate(sizes)])
        before = p.snapshot()
        slots = lambda *s: np.array(s, np.uint32)
        src = texels(510, 64, 64)
        dev = torch.from_numpy(np.concatenate([src, src])).to("cuda")

        def refused(call, words, status=RXR_ERR_INVALID):
            assert call() == status
            assert all(w in p.error() for w in words), p.error()
            after = p.snapshot()
            for (s0, f0, d0), (s1, f1, d1) in zip(before, after):
                assert s0 == s1 and f0 == f1 and d0.tobytes() == d1.tobytes(), "a refused call changed the pool"

        for name, call in (("rxr_update_chunk_textures", lambda s, n: p.rxr.rxr_update_chunk_textures(p.ctx, s.ctypes.data, n, src.ctypes.data)),
                           ("rxr_update_chunk_textures_to", lambda s, n: p.rxr.rxr_update_chunk_textures_to(p.ctx, s.ctypes.data, n, dev.data_ptr(), None))):
            refused(lambda: call(slots(2, 3), 2), [name, "slots[1] = 3", "no such slot"])
            refused(lambda: call(slots(2, 0, 2), 3), [name, "slots[2] = 2", "named twice"])
        two = slots(2)
        refused(lambda: p.rxr.rxr_update_chunk_textures_to(p.ctx, two.ctypes.data, 1, src.ctypes.data, None), ["not device memory"])
        refused(lambda: p.rxr.rxr_update_chunk_textures_to(p.ctx, two.ctypes.data, 1, dev.data_ptr() + 2, None), ["4-byte aligned"])
        refused(lambda: p.rxr.rxr_update_chunk_textures_to(p.ctx, two.ctypes.data, 1, None, None), ["4-byte aligned"])
        refused(lambda: p.rxr.rxr_update_chunk_textures(p.ctx, two.ctypes.data, 1, None), ["NULL rgba"])
        # a refused registration leaves the previous one as it was
        refused(lambda: p.register([(8, 0)], [None], expect=RXR_ERR_INVALID), ["rxr_set_chunk_textures", "side of 0"])
        p.sizes = sizes
        # no registration
        assert p.register([], [], n_chunks=0) == RXR_OK
        for call in (lambda: p.rxr.rxr_update_chunk_textures(p.ctx, two.ctypes.data, 1, src.ctypes.data),
                     lambda: p.rxr.rxr_update_chunk_textures_to(p.ctx, two.ctypes.data, 1, dev.data_ptr(), None)):
            assert call() == RXR_ERR_INVALID and "no registration" in p.error()
        assert p.rxr.rxr_read_chunk_texture(p.ctx, 0, None, None, None) == RXR_ERR_INVALID


def test_frames_must_match_the_registration():
    """a frame with another n_chunks, or one that carries its own chunk textures, is refused while a registration is held"""
    with Pool() as p:
        data = texels(600, 8, 8)
        tex = Tex(data.ctypes.data, 8, 8)
        chunks = (Chunk * 2)()
        for c in chunks:
            c.size = 8

        def upload(n_chunks):
            f = Frame()
            f.abi_version, f.width, f.height, f.tile_size, f.scaled2, f.flags = 5, 64, 64, 32, 1.0, 1 << 1
            f.chunks, f.n_chunks = chunks, n_chunks
            return p.rxr.rxr_upload_frame(p.ctx, C.byref(f))

        chunks[1].terrain_texture = C.pointer(tex)
        assert upload(2) == RXR_OK, p.error()                  # no registration: the frame carries its textures
        p.register([(8, 8)], [data], n_chunks=2)
        assert upload(2) == RXR_ERR_INVALID and "chunk 1 carries its own" in p.error()
        chunks[1].terrain_texture = None
        chunks[0].shader_textures, chunks[0].n_shader_textures = C.pointer(tex), 1
        assert upload(2) == RXR_ERR_INVALID and "chunk 0 carries its own" in p.error()
        chunks[0].shader_textures, chunks[0].n_shader_textures = None, 0
        assert upload(1) == RXR_ERR_INVALID and "1 chunks" in p.error() and "registered the textures of 2" in p.error()
        assert upload(2) == RXR_OK, p.error()
        chunks[0].size = 0
        assert upload(2) == RXR_ERR_INVALID and "size 0" in p.error()
        chunks[0].size = 8
        assert p.register([], [], n_chunks=0) == RXR_OK        # removed: frames carry their textures again
        chunks[1].terrain_texture = C.pointer(tex)
        assert upload(2) == RXR_OK, p.error()


# ---- frames through the mirror ---------------------------------------------------------------------------------------------------------
def two_chunk_scene(api, path, sample_mode, resident, terrain0=None, baked=None, holes1=False):
    """two chunks with a terrain batch each (3D: floor quads; 2D: rectangles), chunk 0 with one baked 64 x 64 shader texture on a box and one
    None entry (a program that runs), a static floor underneath"""
    scene = api.Scene.empty()
    scene.add_program(B.Program([[("Push", 0.0, 0.0, 1.0), "SetColor"]]))
    c0, c1 = scene.add_chunk(), scene.add_chunk()
    c0.terrain(terrain0 if terrain0 is not None else terrain_texture(31, 64, 64), origin=(0, 0), size=8)
    c1.terrain(terrain_texture(32, 48, 48, holes=holes1), origin=(8, 0), size=8)
    s0 = c0.add_shader(CHECKER, baked if baked is not None else terrain_texture(33, 64, 64))
    green = B.Program([["Color", ("Push", 0.2, 1.0, 0.2), "Mul", "SetColor"]])
    s1 = c0.add_shader(green, None)
    assets = api.Assets.default().textures([B.Tile.from_texture(scenes.noise_texture(8, 32, 32))])
    if path == "3d":
        scene.add_d3_static(floor_quad(api, -2.0, -2.0, 18.0, 10.0, y=-0.5).source(B.PixelSource.Pixel((40, 60, 200, 255))))
        c0.terrain_batch3d(floor_quad(api, 0.0, 0.0, 8.0, 8.0).source(B.PixelSource.Terrain()))
        c1.terrain_batch3d(floor_quad(api, 8.0, 0.0, 16.0, 8.0).source(B.PixelSource.Terrain()))
        for x, s in ((2.0, s0), (5.0, s1)):
            box = api.Batch3D.from_box(x, 0.0, 3.0, 1.5, 1.5, 1.5).cull_mode(B.CULL_OFF).with_computed_normals()
            c0.add_batch3d(box.source(B.PixelSource.StaticTileIndex(0)).repeat_mode(B.REPEAT_REPEAT_XY).shader(s))
        scene.lights([B.Light(B.LIGHT_POINT).with_position((8.0, 3.0, 4.0)).with_color((1.0, 0.9, 0.8)).with_intensity(2.0)
                      .with_start_distance(1.0).with_end_distance(14.0).compile()])
        cam = api.D3OrbitCamera.new()
        cam.set_parameter_f32("distance", 13.0)
        cam.center = (8.0, 0.0, 4.0)
        cam.azimuth = 1.3
        cam.elevation = 0.9

        def setup():
            v, p = cam.matrices(float(W), float(H))
            r = api.Rasterizer.setup(None, v, p).ambient((0.6, 0.6, 0.6, 1.0))
            r.sample_mode(sample_mode)
            return r
    else:
        c0.terrain_batch2d(api.Batch2D.from_rectangle(0.0, 0.0, 8.0, 8.0).source(B.PixelSource.Terrain()))
        c1.terrain_batch2d(api.Batch2D.from_rectangle(8.0, 0.0, 8.0, 8.0).source(B.PixelSource.Terrain()))
        m2d = B.Mat3.from_rows([[12.0, 0.0, 6.0], [0.0, 12.0, 10.0], [0.0, 0.0, 1.0]])

        def setup():
            r = api.Rasterizer.setup(m2d, B.Mat4.identity(), B.Mat4.identity())
            r.sample_mode(sample_mode)
            return r

    scene.resident_chunk_textures = resident
    return scenes._result(api, scene, assets, setup, W, H, 40, "chunk-textures", chunks=(c0, c1))


def last_kernel(product):
    return (rusterix_amd.rxr_abi().rxr_debug_last_raster_kernel(product.lib.rxh_context()) or b"").decode()


def render_named(product, cfg):
    px = scenes.render(cfg).copy()
    return px, last_kernel(product)


@pytest.mark.parametrize("sample_mode", [B.SAMPLE_NEAREST, B.SAMPLE_LINEAR])
@pytest.mark.parametrize("path", ["3d", "2d"])
def test_resident_frame_is_byte_identical_and_drawn_by_the_same_kernel(product, path, sample_mode):
    carried, kernel = render_named(product, two_chunk_scene(product, path, sample_mode, False))
    assert len(np.unique(carried.reshape(-1, 4), axis=0)) > 300, "the textures should be visible"
    n0 = product.chunk_texture_registrations()
    cfg = two_chunk_scene(product, path, sample_mode, True)
    resident, kernel_r = render_named(product, cfg)
    assert product.chunk_texture_registrations() == n0 + 1
    assert kernel and kernel_r == kernel, (kernel, kernel_r)
    assert resident.tobytes() == carried.tobytes(), f"{(resident != carried).any(axis=2).sum()} pixels differ"
    again, _ = render_named(product, cfg)
    assert product.chunk_texture_registrations() == n0 + 1, "an unchanged scene registers nothing"
    assert again.tobytes() == carried.tobytes()
    # the option off: the registration is removed, nothing is registered, the frame is the same
    cfg.scene.resident_chunk_textures = False
    off, _ = render_named(product, cfg)
    assert product.chunk_texture_registrations() == n0 + 1 and off.tobytes() == carried.tobytes()


def bake_terrain():
    """a terrain of chunk size 8 whose chunks (0, 0) and (1, 0) have sources, a blended cell and a cell without a texture"""
    def build(product):
        t = product.Terrain((1.0, 1.0), 8)
        a, b = terrain_texture(41, 16, 16), terrain_texture(42, 24, 24, holes=True)
        for x in range(16):
            for y in range(8):
                t.set_source(x, y, a if (x + y) % 3 else b)
        t.set_source(5, 5, None)
        t.set_blend_mode(2, 2, B.TERRAIN_BLEND_RADIUS, 2)
        return t
    return build


def test_update_from_the_device_bakes_gives_the_carried_frame(product):
    """rxr_bake_terrain_to -> rxr_update_chunk_textures_to for the terrain slot, rxr_bake_shaders_to -> the same for the 64 x 64 shader
    slot, then a host update to a translucent texture and back: each time the re-uploaded frame is the frame that carries those bytes"""
    import torch

    rxr = rusterix_amd.rxr_abi()
    terrain = bake_terrain()(product)
    baked_terrain = B.Texture(terrain.bake_chunks([(0, 0)], 8)[0].reshape(-1).copy(), 64, 64)     # (also makes the terrain resident)
    probe = product.Scene.empty()
    pc = probe.add_chunk()
    assets = product.Assets.default().textures([B.Tile.from_texture(scenes.noise_texture(8, 32, 32))])
    pc.add_shader(CHECKER, bake=True, assets=assets)
    baked_shader = pc.shader_texture(0)
    holes = terrain_texture(51, 64, 64, holes=True)
    want_terrain = scenes.render(two_chunk_scene(product, "3d", B.SAMPLE_NEAREST, False, terrain0=baked_terrain)).copy()
    want_both = scenes.render(two_chunk_scene(product, "3d", B.SAMPLE_NEAREST, False, terrain0=baked_terrain, baked=baked_shader)).copy()
    want_holes = scenes.render(two_chunk_scene(product, "3d", B.SAMPLE_NEAREST, False, terrain0=holes, baked=baked_shader)).copy()
    assert (want_terrain != want_both).any() and (want_both != want_holes).any()

    cfg = two_chunk_scene(product, "3d", B.SAMPLE_NEAREST, True)
    first = scenes.render(cfg).copy()                       # registers: slot 0 chunk 0's terrain, 1 its shader texture, 2 chunk 1's terrain
    assert (first != want_terrain).any()
    n0 = product.chunk_texture_registrations()
    ctx = product.lib.rxh_context()
    stream = torch.cuda.Stream()
    dev = torch.zeros(64 * 64 * 4, dtype=torch.uint8, device="cuda")
    coords, slot = np.array([0, 0], np.int32), np.zeros(1, np.uint32)
    assert rxr.rxr_bake_terrain_to(ctx, coords.ctypes.data, 1, 8, dev.data_ptr(), stream.cuda_stream) == RXR_OK, rxr.rxr_last_error(ctx)
    assert rxr.rxr_update_chunk_textures_to(ctx, slot.ctypes.data, 1, dev.data_ptr(), stream.cuda_stream) == RXR_OK, rxr.rxr_last_error(ctx)
    got = scenes.render(cfg).copy()
    assert got.tobytes() == want_terrain.tobytes(), f"{(got != want_terrain).any(axis=2).sum()} pixels differ"
    # the shader slot: CHECKER is program 1 of the resident set (scene.shaders[0], then chunk 0's shaders)
    program, slot[0] = np.array([1], np.uint32), 1
    assert rxr.rxr_bake_shaders_to(ctx, program.ctypes.data, 1, 64, 64, None, dev.data_ptr(), stream.cuda_stream) == RXR_OK, rxr.rxr_last_error(ctx)
    assert rxr.rxr_update_chunk_textures_to(ctx, slot.ctypes.data, 1, dev.data_ptr(), stream.cuda_stream) == RXR_OK, rxr.rxr_last_error(ctx)
    got = scenes.render(cfg).copy()
    assert got.tobytes() == want_both.tobytes(), f"{(got != want_both).any(axis=2).sum()} pixels differ"
    # opaque -> translucent -> opaque: a stale flag would keep the cut-out test off (or on)
    slot[0] = 0
    data = np.ascontiguousarray(holes.data, np.uint8)
    assert rxr.rxr_update_chunk_textures(ctx, slot.ctypes.data, 1, data.ctypes.data) == RXR_OK, rxr.rxr_last_error(ctx)
    got = scenes.render(cfg).copy()
    assert got.tobytes() == want_holes.tobytes(), f"{(got != want_holes).any(axis=2).sum()} pixels differ"
    data = np.ascontiguousarray(baked_terrain.data, np.uint8)
    assert rxr.rxr_update_chunk_textures(ctx, slot.ctypes.data, 1, data.ctypes.data) == RXR_OK, rxr.rxr_last_error(ctx)
    got = scenes.render(cfg).copy()
    assert got.tobytes() == want_both.tobytes(), f"{(got != want_both).any(axis=2).sum()} pixels differ"
    assert product.chunk_texture_registrations() == n0, "the updates went to the slots: nothing was registered again"
    torch.cuda.synchronize()


def test_a_group_takes_the_host_form_and_refuses_the_device_form(product):
    """the process-wide context as a group (two members on device 0): the registration replicates, the frame is byte-identical, the
    host update runs on every member, the _to form is RXR_ERR_UNSUPPORTED"""
    import torch

    rxr = rusterix_amd.rxr_abi()
    holes = terrain_texture(52, 64, 64, holes=True)
    try:
        ids = (C.c_int * 2)(0, 0)
        product.lib.rxh_set_devices(ids, 2)
        carried = scenes.render(two_chunk_scene(product, "3d", B.SAMPLE_NEAREST, False)).copy()
        want_holes = scenes.render(two_chunk_scene(product, "3d", B.SAMPLE_NEAREST, False, terrain0=holes)).copy()
        cfg = two_chunk_scene(product, "3d", B.SAMPLE_NEAREST, True)
        resident = scenes.render(cfg).copy()
        assert resident.tobytes() == carried.tobytes(), f"{(resident != carried).any(axis=2).sum()} pixels differ"
        ctx = product.lib.rxh_context()
        assert rxr.rxr_member_count(ctx) == 2
        slot, data = np.zeros(1, np.uint32), np.ascontiguousarray(holes.data, np.uint8)
        dev = torch.from_numpy(data).to("cuda")
        assert rxr.rxr_update_chunk_textures_to(ctx, slot.ctypes.data, 1, dev.data_ptr(), None) == RXR_ERR_UNSUPPORTED
        assert "multi-device" in (rxr.rxr_last_error(ctx) or b"").decode()
        assert rxr.rxr_update_chunk_textures(ctx, slot.ctypes.data, 1, data.ctypes.data) == RXR_OK, rxr.rxr_last_error(ctx)
        got = scenes.render(cfg).copy()
        assert got.tobytes() == want_holes.tobytes(), f"{(got != want_holes).any(axis=2).sum()} pixels differ"
        flag = C.c_uint32(7)
        assert rxr.rxr_read_chunk_texture(ctx, 0, None, C.byref(flag), None) == RXR_OK and flag.value == 0
    finally:
        product.lib.rxh_set_device(0)


# ---- the mirror's texture stroke --------------------------------------------------------------------------------------------------------
def terrain_scene(product, terrain, ppt, resident):
    scene = product.Scene.empty()
    scene.add_d3_static(floor_quad(product, -2.0, -2.0, 18.0, 10.0, y=-0.5).source(B.PixelSource.Pixel((40, 60, 200, 255))))
    chunks = []
    for k in range(2):
        c = scene.add_chunk()
        c.terrain(None, origin=(8 * k, 0), size=8)
        terrain.build_chunk_at((k, 0), ppt[k], c)
        c.terrain_batch3d(floor_quad(product, 8.0 * k, 0.0, 8.0 * k + 8.0, 8.0).source(B.PixelSource.Terrain()))
        chunks.append(c)
    cam = product.D3OrbitCamera.new()
    cam.set_parameter_f32("distance", 13.0)
    cam.center = (8.0, 0.0, 4.0)
    cam.azimuth = 1.3
    cam.elevation = 0.9

    def setup():
        v, p = cam.matrices(float(W), float(H))
        return product.Rasterizer.setup(None, v, p).ambient((0.8, 0.8, 0.8, 1.0))

    scene.resident_chunk_textures = resident
    return scenes._result(product, scene, product.Assets.default(), setup, W, H, 40, "chunk-textures-terrain", chunks=chunks)


def test_the_mirror_strokes_textures_on_the_device(product):
    terrain = bake_terrain()(product)
    reg = product.chunk_texture_registrations
    cfg = terrain_scene(product, terrain, (8, 8), True)
    n0 = reg()
    before = scenes.render(cfg).copy()
    assert reg() == n0 + 1
    scenes.render(cfg)
    assert reg() == n0 + 1, "a second upload without changes registers nothing"
    # the stroke: both chunks' cells change
    stroke = terrain_texture(43, 16, 16)
    for x in (3, 4, 11):
        terrain.set_source(x, 3, stroke)
    assert terrain.rebuild_chunk_textures(cfg.scene, [(0, 0), (1, 0)], [0, 1], 8) == 0
    assert all(c.terrain_texture_stale() for c in cfg.chunks)
    got_stroke = scenes.render(cfg).copy()
    assert reg() == n0 + 1, "the fast path keeps the registration current"
    assert (got_stroke != before).any()
    # the stale host copy is read back from the slot
    want_bytes = terrain.bake_chunks([(0, 0), (1, 0)], 8)
    for k, c in enumerate(cfg.chunks):
        tex = c.terrain_texture()
        assert (tex.width, tex.height) == (64, 64) and tex.data.tobytes() == want_bytes[k].tobytes()
        assert not c.terrain_texture_stale()
    # a second stroke on chunk 1 alone stays on the device; then chunk 0 changes its side: the fallback, and the registration that follows
    # must bring chunk 1's bytes back from its slot, not from the stale host copy
    terrain.set_source(12, 5, stroke)
    assert terrain.rebuild_chunk_textures(cfg.scene, [(1, 0)], [1], 8) == 0 and cfg.chunks[1].terrain_texture_stale()
    assert terrain.rebuild_chunk_textures(cfg.scene, [(0, 0)], [0], 4) == 1
    got_ppt = scenes.render(cfg).copy()
    assert reg() == n0 + 2
    # named twice: the library refuses, the mirror falls back
    assert terrain.rebuild_chunk_textures(cfg.scene, [(0, 0), (0, 0)], [0, 0], 4) == 1
    # the references: scenes built from scratch with build_chunk_at, their textures carried by the frames
    n1 = reg()
    want_ppt = scenes.render(terrain_scene(product, terrain, (4, 8), False)).copy()
    assert got_ppt.tobytes() == want_ppt.tobytes(), f"{(got_ppt != want_ppt).any(axis=2).sum()} pixels differ"
    for x in (12,):
        terrain.set_source(x, 5, terrain_texture(41, 16, 16) if (x + 5) % 3 else terrain_texture(42, 24, 24, holes=True))   # the second stroke undone
    want_stroke = scenes.render(terrain_scene(product, terrain, (8, 8), False)).copy()
    assert got_stroke.tobytes() == want_stroke.tobytes(), f"{(got_stroke != want_stroke).any(axis=2).sum()} pixels differ"
    assert reg() == n1, "with the option off nothing is registered"
    # ... and without the option the stroke takes the fallback
    off = terrain_scene(product, terrain, (8, 8), False)
    assert terrain.rebuild_chunk_textures(off.scene, [(0, 0)], [0], 8) == 1
