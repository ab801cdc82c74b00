"""The path tracer on the device (rxr_set_trace_scene / rxr_trace / rxr_accum_to_rgba, include/rxr.h) against the numpy restatement of
Tracer::trace (tests/trace_ref.py), which takes the device's own sRGB table:

  * paths without a diffuse bounce run no libm function on the device: EVERY FLOAT of the accumulation buffer equals the restatement's
    -- one bounce over the frame sizes at which the closest-hit kernels change (8x8 / 9x8 straddle the thread-per-triangle limit of 64
    rays, 16x16 / 17x16 one workgroup of rays, 37x21 is odd), the three cameras, eight mirror bounces over three frames in one call and
    in three, every texel source, material role and modifier, sample mode and repeat mode, and meshes in the opacity and overlay lists
    the tracer must not see;
  * spot / area / daylight / ambient lights: the bytes of to_u8 within one 8-bit step per channel of the restatement's, the bound
    tests/test_gpu_special_lights.py holds the rasterizer's exact light loop to (acos is the device's);
  * diffuse paths (cos and sin are the device's): per pixel within a tolerance taken from the restatement alone (S.diffuse_tolerance),
    at most 1 pixel in 50 outside; the mean of 64 device frames within three standard errors of 64 restated frames of another seed;
  * a trace between upload and render leaves the frame as it was; every refusal returns its code and leaves the buffer untouched."""
import ctypes as C

import numpy as np
import pytest

import rusterix_amd
from rusterix_amd import binding as B
from rusterix_amd import scenes
from rusterix_amd import trace as T
from rusterix_amd.abi import RXR_ERR_INVALID, RXR_ERR_UNSUPPORTED, RXR_OK
from tests import intersect_ref as R
from tests import trace_ref as TR
from tests import trace_scenes as S

pytestmark = pytest.mark.gpu
F = np.float32
GLOSSY_1 = (T.GLOSSY, T.MOD_NONE, 1.0)


@pytest.fixture(scope="module")
def tracer():
    with T.Tracer() as tr:
        yield tr


@pytest.fixture(scope="module")
def orc():
    from tests.oracle_api import load_oracle
    return load_oracle()


def same(a, b):
    return R.same(np.asarray(a, F).ravel(), np.asarray(b, F).ravel())


def assert_same(got, ref, label):
    if not same(got, ref):
        bad = np.argwhere(got.view(np.uint32) != ref.view(np.uint32))
        y, x, c = bad[0]
        raise AssertionError(f"{label}: {len(bad)} floats differ; first at pixel ({x}, {y}) channel {c}: got {got[y, x, c]!r}, expected {ref[y, x, c]!r}")


def run(tracer, orc, scene, camera, width, height, n_frames=1, seed=3, bounces=1, first_frame=0):
    """(device, restatement) after n_frames from `first_frame` into a buffer holding noise"""
    S.load(tracer, scene)
    acc = T.AccumBuffer(width, height)
    acc.pixels[:] = np.random.default_rng(width * 1000 + height).random((height, width, 4), dtype=F)   # (in/out: frame 0 must wipe it)
    acc.frame = first_frame
    start = acc.pixels.copy()
    tracer.trace(camera, acc, n_frames=n_frames, seed=seed, bounces=bounces)
    ref = TR.trace(orc, scene, camera, width, height, first_frame, n_frames, seed, bounces, start, tracer.srgb_table())
    return acc.pixels, ref


@pytest.mark.parametrize("size", [(1, 1), (8, 8), (9, 8), (16, 16), (17, 16), (37, 21)])
def test_one_bounce_is_exact(tracer, orc, size):
    w, h = size
    got, ref = run(tracer, orc, S.room(), S.cameras(w, h)["firstp"], w, h)
    assert_same(got, ref, f"{w}x{h}")
    if w * h >= 64:
        assert (ref[..., :3] > 0).any() and len(np.unique(ref[..., 0])) > 4


@pytest.mark.parametrize("camera", ["firstp", "orbit", "iso"])
def test_each_camera_is_exact(tracer, orc, camera):
    got, ref = run(tracer, orc, S.room(), S.cameras(21, 13)[camera], 21, 13, first_frame=2)
    assert_same(got, ref, camera)
    assert (ref[..., :3] > 0).any()


def test_eight_mirror_bounces_are_exact_in_one_call_and_in_three(tracer, orc):
    scene = S.room(material=GLOSSY_1, panel_material=GLOSSY_1)
    w, h = 16, 12
    cam = S.cameras(w, h)["firstp"]
    S.load(tracer, scene)
    one, three = T.AccumBuffer(w, h), T.AccumBuffer(w, h)
    tracer.trace(cam, one, n_frames=3, seed=9, bounces=8)
    for _ in range(3):
        tracer.trace(cam, three, n_frames=1, seed=9, bounces=8)
    ref, sigs = TR.trace(orc, scene, cam, w, h, 0, 3, 9, 8, np.zeros((h, w, 4), F), tracer.srgb_table(), signatures=True)
    assert_same(one.pixels, ref, "three frames in one call")
    assert_same(three.pixels, one.pixels, "three calls against one")
    assert one.frame == three.frame == 3
    depth = [len(s) for frame in sigs for s in frame]
    assert max(depth) == 8 and all(step[-1] == "S" for frame in sigs for s in frame for step in s if step != ("miss",))   # mirrors all the way


SOURCES = dict(pixel=S.PIXEL(90, 140, 250), static_two_frames=(T.SOURCE_STATIC_TILE, 0, (0, 0, 0, 0)), static_other_tile=(T.SOURCE_STATIC_TILE, 1, (0, 0, 0, 0)),
               dynamic=(T.SOURCE_DYNAMIC_TILE, 0, (0, 0, 0, 0)), other=(T.SOURCE_OTHER, 0, (9, 9, 9, 9)), terrain_without_chunk=(T.SOURCE_TERRAIN, 0, (0, 0, 0, 0)))


@pytest.mark.parametrize("source", sorted(SOURCES))
@pytest.mark.parametrize("sample_mode", [0, 1])
def test_sources_are_exact(tracer, orc, source, sample_mode):
    for animation_frame, repeat in ((1, 0), (2, 1), (5, 2), (4, 3)):
        scene = S.room(box_source=SOURCES[source], sample_mode=sample_mode, box_repeat=repeat, animation_frame=animation_frame)
        got, ref = run(tracer, orc, scene, S.cameras(16, 16)["firstp"], 16, 16)
        assert_same(got, ref, f"{source}, sample mode {sample_mode}, repeat mode {repeat}, animation frame {animation_frame}")
        if source in ("pixel", "dynamic") or sample_mode:
            break   # (a constant texel has no repeat mode; the dynamic tile has one frame; the repeat modes run with nearest sampling)


def test_terrain_from_a_resident_chunk_texture_is_exact(tracer, orc):
    """the floor and the box as terrain-sourced meshes of two chunks: one with a 24 x 24 texture over 8 tiles (3 pixels a tile) whose
    origin leaves part of the floor outside it (clamped), one without a texture (zero)"""
    for origin, tex in (((0, 0), S.texture(21, 24, 24)), ((2, -3), S.texture(22, 16, 24))):
        scene = S.room(box_source=(T.SOURCE_TERRAIN, 0, (0, 0, 0, 0)))
        scene["chunks"] = [dict(terrain_texture=tex, origin=origin, size=8), dict(terrain_texture=None, origin=(0, 0), size=8)]
        floor, inner = scene["meshes"][1], scene["meshes"][-2]
        floor.update(source=(T.SOURCE_TERRAIN, 0, (0, 0, 0, 0)), list=T.LIST_CHUNK_TERRAIN, chunk=0)
        inner.update(list=T.LIST_CHUNK, chunk=1)
        got, ref = run(tracer, orc, scene, S.cameras(16, 16)["firstp"], 16, 16)
        assert_same(got, ref, f"terrain, origin {origin}")
        plain, _ = run(tracer, orc, S.room(), S.cameras(16, 16)["firstp"], 16, 16)
        assert not same(got, plain)


def test_uvs_outside_the_unit_square_meet_every_repeat_mode(tracer, orc):
    for repeat in range(4):
        for sample_mode in (0, 1):
            scene = S.room(box_source=SOURCES["static_two_frames"], sample_mode=sample_mode, box_repeat=repeat)
            inner = scene["meshes"][-2]
            inner["uvs"] = (inner["uvs"] * F(2.75) - F(0.8)).astype(F)
            got, ref = run(tracer, orc, scene, S.cameras(16, 16)["firstp"], 16, 16)
            assert_same(got, ref, f"repeat mode {repeat}, sample mode {sample_mode}")


@pytest.mark.parametrize("role", [T.MATTE, T.GLOSSY, T.METALLIC, T.TRANSPARENT, T.EMISSIVE])
def test_material_roles_and_modifiers_are_exact(tracer, orc, role):
    """one bounce: every float.  Two bounces, where the material decides the second ray: every float of the pixels whose first bounce
    was not diffuse (a diffuse direction goes through the device's cos and sin)"""
    cam = S.cameras(16, 16)["firstp"]
    for modifier in range(5):
        scene = S.room(material=(role, modifier, 0.6), panel_material=(T.EMISSIVE, modifier, 0.8), box_source=SOURCES["static_two_frames"])
        got, ref = run(tracer, orc, scene, cam, 16, 16, bounces=1)
        assert_same(got, ref, f"role {role}, modifier {modifier}, one bounce")
        acc = T.AccumBuffer(16, 16)
        tracer.trace(cam, acc, n_frames=1, seed=3, bounces=2)
        ref2, sigs = TR.trace(orc, scene, cam, 16, 16, 0, 1, 3, 2, np.zeros((16, 16, 4), F), tracer.srgb_table(), signatures=True)
        exact = np.array([not (len(s) and s[0][-1] == "D") for s in sigs[0]]).reshape(16, 16)   # ("Dr": the roulette ended it there)
        assert exact.any()
        bits = acc.pixels.view(np.uint32) == ref2.view(np.uint32)
        assert bits[exact].all(), f"role {role}, modifier {modifier}, two bounces: {int((~bits[exact]).sum())} floats differ"


def test_opacity_and_overlay_meshes_are_not_seen(tracer, orc):
    front = [S.box(3.0, 1.0, 1.5, 2.5, 2.5, 0.1, source=S.PIXEL(255, 0, 255), list=T.LIST_CHUNK_OPACITY, chunk=0),
             S.box(3.5, 1.5, 1.2, 2.5, 2.5, 0.1, source=S.PIXEL(0, 255, 255), list=T.LIST_OVERLAY)]
    plain = S.room()
    scene = dict(plain, meshes=[front[0]] + plain["meshes"] + [front[1]])
    got, ref = run(tracer, orc, scene, S.cameras(16, 16)["firstp"], 16, 16)
    assert_same(got, ref, "with an opacity and an overlay mesh in front")
    got_plain, _ = run(tracer, orc, plain, S.cameras(16, 16)["firstp"], 16, 16)
    assert_same(got, got_plain, "against the room without them")


@pytest.mark.parametrize("kind", [B.LIGHT_SPOT, B.LIGHT_AREA, B.LIGHT_DAYLIGHT, B.LIGHT_AMBIENT])
def test_other_light_types_within_one_byte_step(tracer, orc, kind):
    lights = [S.point_light((3.5, 3.8, 3.0), kind=kind, intensity=0.4, start=1.5, end=7.0, flicker=0.3)]
    got, ref = run(tracer, orc, S.room(lights=lights), S.cameras(16, 16)["firstp"], 16, 16)
    acc = T.AccumBuffer(16, 16)
    acc.pixels[:] = got
    d = np.abs(tracer.to_u8(acc).astype(np.int16) - TR.to_u8(ref).astype(np.int16))
    assert d.max() <= 1, f"light type {kind}: {int((d > 1).sum())} bytes off by more than one step (max {int(d.max())})"
    lit = TR.trace(orc, S.room(lights=[]), S.cameras(16, 16)["firstp"], 16, 16, 0, 1, 3, 1, np.zeros((16, 16, 4), F), tracer.srgb_table())
    assert np.abs(ref[..., :3] - lit[..., :3]).max() > 0.01   # (the light reaches the room)


def test_diffuse_paths_within_the_reference_tolerance(tracer, orc):
    """The tolerance is the restatement's own: S.diffuse_tolerance runs it with cos and sin correctly rounded and again with both moved by
    4 float32 ulps (the bound tests/test_gpu_libm_ulp.py asserts for the device's), and takes 4 times the largest difference over the
    pixels whose path signatures agree.  Pixels outside it left through a triangle edge or a roulette threshold: at most 1 in 50."""
    scene, cam, w, h, seed = S.diffuse_case()
    S.load(tracer, scene)
    acc = T.AccumBuffer(w, h)
    tracer.trace(cam, acc, n_frames=4, seed=seed, bounces=8)
    ref, tolerance, disagree = S.diffuse_tolerance(orc, tracer.srgb_table())
    d = np.abs(acc.pixels - ref).max(axis=2)
    outside = int((d > tolerance).sum())
    print(f"diffuse room {w}x{h}: tolerance {tolerance:.3e} ({disagree} pixels of the two reference runs disagree), largest difference {d.max():.3e}, "
          f"median {np.median(d):.3e}, {outside} of {w * h} pixels beyond the tolerance")
    assert outside * 50 <= w * h, f"{outside} of {w * h} pixels beyond the tolerance {tolerance:.3e} (largest difference {d.max():.3e})"


def test_unbiased_against_another_seed(tracer, orc):
    w, h, frames = 16, 12, 64
    scene = S.diffuse_room()
    cam = S.cameras(w, h)["firstp"]
    S.load(tracer, scene)
    acc = T.AccumBuffer(w, h)
    tracer.trace(cam, acc, n_frames=frames, seed=100, bounces=8)
    table = tracer.srgb_table()
    per_frame = np.array([TR.trace(orc, scene, cam, w, h, 0, 1, 5000 + k, 8, np.zeros((h, w, 4), F), table)[..., :3].mean(axis=(0, 1), dtype=np.float64)
                          for k in range(frames)])   # (frame 0 of 64 seeds: independent samples, each the whole image's mean)
    mean, sem = per_frame.mean(axis=0), per_frame.std(axis=0, ddof=1) / np.sqrt(frames)
    got = acc.pixels[..., :3].mean(axis=(0, 1), dtype=np.float64)
    z = np.abs(got - mean) / sem     # three standard errors of the reference's mean, from its own per-frame variance
    print(f"image means: device {got}, restatement {mean}, standard error {sem}, z {z}")
    assert np.all(z <= 3.0), f"device mean {got} against {mean} +- {sem}: z = {z}"


def test_accum_to_rgba_follows_the_byte_rule(tracer):
    """AccumBuffer::to_u8_vec on the device over negatives, NaN, infinities, values above 1, the linear segment's threshold and alpha away
    from 1: a byte may differ from the float64 evaluation by one only where srgb * 255 + 0.5 lies within the pow bound of an integer
    (the rule of tests/test_bake_cpu.py); the stream form gives the same bytes"""
    import torch

    acc = T.AccumBuffer(64, 8)
    acc.pixels[:] = S.byte_rule_values(64, 8)
    got = tracer.to_u8(acc)
    S.assert_byte_rule(got, acc.pixels)
    assert got[0, 0].tolist() == [0, 10, 255, 255] and got[0, 1].tolist() == [0, 255, 0, 0]
    assert np.array_equal(got[..., 3], TR.to_u8(acc.pixels)[..., 3])          # alpha: no pow, the bytes are the transcription's
    dev, out = torch.from_numpy(acc.pixels).cuda(), torch.zeros((8, 64, 4), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    assert tracer.rxr.rxr_accum_to_rgba_to(tracer.ctx, dev.data_ptr(), 64, 8, out.data_ptr(), stream.cuda_stream) == RXR_OK, tracer.error()
    stream.synchronize()
    assert np.array_equal(out.cpu().numpy(), got)


def test_scene_trace_through_the_mirror(product, orc):
    """Scene.trace of the binding (the host mirror's Tracer): the device path registers tiles, batches, materials, lights and chunks
    itself and equals the transcription to the bit; the mirror's CPU path gives the same floats"""
    product.lib.rxh_set_device(0)
    for scene, bounces in ((S.room(material=GLOSSY_1, panel_material=GLOSSY_1, sample_mode=1), 8), (S.room(), 1)):
        scene = S.ordered(scene)
        sc, assets = S.mirror_scene(product, scene)
        cam = product.D3FirstPCamera.new()
        cam.position, cam.center, cam.fov = (4.0, 2.2, 0.6), (4.1, 1.9, 6.0), 70.0
        dev, cpu = product.AccumBuffer(17, 12), product.AccumBuffer(17, 12)
        sc.trace(cam, dev, assets, n_frames=2, seed=5, bounces=bounces, sample_mode=scene["sample_mode"])
        sc.trace(cam, cpu, assets, n_frames=2, seed=5, bounces=bounces, sample_mode=scene["sample_mode"], cpu=True)
        table = np.zeros(256, F)
        assert rusterix_amd.rxr_abi().rxr_trace_srgb_table(None, table.ctypes.data) == RXR_OK
        ref = TR.trace(orc, scene, S.cameras(17, 12)["firstp"], 17, 12, 0, 2, 5, bounces, np.zeros((12, 17, 4), F), table)
        assert dev.frame == cpu.frame == 2
        assert_same(dev.pixels.copy(), ref, "Scene.trace on the device")
        assert_same(cpu.pixels.copy(), ref, "Scene.trace on the CPU")
    with pytest.raises(B.RasterizeError):
        sc.trace(cam, dev, assets, bounces=9)


def test_two_batches_of_rays_at_1080p(tracer):
    """1920 x 1080 rays x five segments are more keys than one batch holds (2^23): the second batch starts at a ray offset.  An opacity
    and an overlay mesh interleaved with the room's make the five segments; the frame must equal the plain room's, which runs in one
    batch (and whose kernels the small frames above hold to the transcription)"""
    w, h = 1920, 1080
    cam = S.cameras(w, h)["firstp"]
    plain = S.room()
    hidden = [S.box(3.0, 1.0, 1.5, 2.5, 2.5, 0.1, source=S.PIXEL(255, 0, 255), list=T.LIST_CHUNK_OPACITY, chunk=0),
              S.box(3.5, 1.5, 1.2, 2.5, 2.5, 0.1, source=S.PIXEL(0, 255, 255), list=T.LIST_OVERLAY)]
    m = plain["meshes"]
    split = dict(plain, meshes=m[:2] + [hidden[0]] + m[2:5] + [hidden[1]] + m[5:])     # traced, ignored, traced, ignored, traced
    images = []
    for scene in (plain, split):
        S.load(tracer, scene)
        acc = T.AccumBuffer(w, h)
        tracer.trace(cam, acc, n_frames=1, seed=2, bounces=2)
        images.append(acc.pixels)
    assert_same(images[1], images[0], "five segments in two batches against one segment in one")
    assert (images[0][..., :3] > 0).mean() > 0.5


def test_a_trace_leaves_the_uploaded_frame_alone(product):
    product.lib.rxh_set_device(0)
    product.lib.rxh_set_device_projection(1)
    try:
        with R.recording(product) as meshes_of:
            cfg = scenes.cube_scene(product, 160, 120, 40)
        n_meshes = len(meshes_of(cfg.scene))
        before = scenes.render(cfg).copy()
        host, rxr = product.lib, rusterix_amd.rxr_abi()
        host.rxh_rasterizer_upload.restype = C.c_int
        r = cfg.setup()
        assert host.rxh_rasterizer_upload(r._h, cfg.scene._h, cfg.width, cfg.height, cfg.tile_size, cfg.assets._h) == 0
        ctx = host.rxh_context()
        err = lambda: (rxr.rxr_last_error(ctx) or b"").decode()
        assert rxr.rxr_set_trace_scene(ctx, None, None, n_meshes, None, 0, 0, 1, None, 0) == RXR_OK, err()
        kind, consts = T.camera_firstp((0.5, 0.5, -4.0), (0.5, 0.5, 0.5), 60.0, 32, 24)
        acc = np.zeros((24, 32, 4), F)
        assert rxr.rxr_trace(ctx, kind, consts.ctypes.data, 32, 24, 0, 2, 1, 4, acc.ctypes.data) == RXR_OK, err()
        assert np.all(acc[..., 3] == 1.0)
        px = np.zeros(cfg.width * cfg.height * 4, np.uint8)
        assert rxr.rxr_render_download(ctx, px.ctypes.data) == RXR_OK, err()
        assert np.array_equal(px.reshape(before.shape), before)
    finally:
        product.lib.rxh_set_device_projection(0)


def test_refusals_leave_the_buffer_untouched(tracer):
    rxr, ctx = tracer.rxr, tracer.ctx
    S.load(tracer, S.room())
    kind, consts = S.cameras(8, 8)["firstp"]
    acc = np.full((8, 8, 4), -7.0, F)
    cp, ap = consts.ctypes.data, acc.ctypes.data
    cases = [((kind, None, 8, 8, 0, 1, 1, 1, ap), RXR_ERR_INVALID), ((kind, cp, 8, 8, 0, 1, 1, 1, None), RXR_ERR_INVALID),
             ((kind, cp, 0, 8, 0, 1, 1, 1, ap), RXR_ERR_INVALID), ((kind, cp, 8, 0, 0, 1, 1, 1, ap), RXR_ERR_INVALID),
             ((kind, cp, 8, 8, 0, 0, 1, 1, ap), RXR_ERR_INVALID), ((3, cp, 8, 8, 0, 1, 1, 1, ap), RXR_ERR_INVALID),
             ((kind, cp, 8, 8, 0, 1, 1, T.MAX_BOUNCES + 1, ap), RXR_ERR_UNSUPPORTED)]
    for args, code in cases:
        assert rxr.rxr_trace(ctx, *args) == code, args
        assert tracer.error()
    n = len(S.room()["meshes"])
    assert rxr.rxr_set_trace_scene(ctx, None, None, n + 1, None, 0, 0, 1, None, 0) == RXR_ERR_INVALID      # a mismatched n_meshes ...
    assert rxr.rxr_trace(ctx, kind, cp, 8, 8, 0, 1, 1, 1, ap) == RXR_OK                           # ... leaves the scene that was set
    assert np.all(acc[..., 3] == 1.0)
    acc[:] = -7.0
    assert rxr.rxr_trace_to(ctx, kind, cp, 8, 8, 0, 1, 1, 1, ap, None) == RXR_ERR_INVALID            # host memory where device memory belongs
    # a terrain-sourced chunk mesh without a registered chunk texture, and tiles that do not exist
    for source, code in (((T.SOURCE_TERRAIN, 0, (0, 0, 0, 0)), RXR_ERR_UNSUPPORTED), ((T.SOURCE_STATIC_TILE, 9, (0, 0, 0, 0)), RXR_ERR_INVALID),
                         ((T.SOURCE_DYNAMIC_TILE, 1, (0, 0, 0, 0)), RXR_ERR_INVALID)):
        tracer.set_meshes([S.box(0, 0, 0, 1, 1, 1, source=source, list=T.LIST_CHUNK_TERRAIN, chunk=0)])
        assert rxr.rxr_set_trace_scene(ctx, None, None, 1, None, 0, 0, 1, None, 0) == code, source
        assert rxr.rxr_trace(ctx, kind, cp, 8, 8, 0, 1, 1, 1, ap) == RXR_ERR_INVALID            # (no trace scene for these meshes)
    # the asynchronous forms on a multi-device handle
    multi = C.c_void_p()
    assert rxr.rxr_create_multi(C.byref(multi), (C.c_int * 2)(0, 0), 2) == RXR_OK
    try:
        assert rxr.rxr_trace_to(multi, kind, cp, 8, 8, 0, 1, 1, 1, ap, None) == RXR_ERR_UNSUPPORTED
        assert rxr.rxr_accum_to_rgba_to(multi, ap, 8, 8, ap, None) == RXR_ERR_UNSUPPORTED
    finally:
        rxr.rxr_destroy(multi)
    assert np.all(acc == -7.0)


def test_trace_to_on_a_stream_equals_the_blocking_form(tracer):
    import torch

    scene = S.room(material=GLOSSY_1)
    w, h = 17, 16
    cam = S.cameras(w, h)["firstp"]
    S.load(tracer, scene)
    host = T.AccumBuffer(w, h)
    tracer.trace(cam, host, n_frames=2, seed=4, bounces=4)
    dev = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    rgba = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    kind, consts = cam
    assert tracer.rxr.rxr_trace_to(tracer.ctx, kind, consts.ctypes.data, w, h, 0, 2, 4, 4, dev.data_ptr(), stream.cuda_stream) == RXR_OK, tracer.error()
    assert tracer.rxr.rxr_accum_to_rgba_to(tracer.ctx, dev.data_ptr(), w, h, rgba.data_ptr(), stream.cuda_stream) == RXR_OK, tracer.error()
    stream.synchronize()
    assert_same(dev.cpu().numpy(), host.pixels, "rxr_trace_to")
    assert np.array_equal(rgba.cpu().numpy(), tracer.to_u8(host))
