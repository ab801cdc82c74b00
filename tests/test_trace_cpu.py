"""The path tracer's host side without a GPU: the ABI additions (header, generated Rust mirror, exports), every refusal of
rxr_check_trace_scene, the counter-based generator (the library's against tests/trace_ref.py's, and its statistics), the sRGB table, the
cameras' host constants, the host mirror's CPU trace (Scene.trace(cpu=True): bit-equal to tests/trace_ref.py on the scenes without a
diffuse bounce, inside the GPU test's tolerance on the diffuse one, its running average and its to_u8_vec bytes), and the diffuse
criterion's reference experiment: the runs of tests/trace_ref.py that set the tolerance must disagree on fewer than 1 pixel in 100."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import rusterix_amd
from rusterix_amd import binding as B
from rusterix_amd import trace as T
from rusterix_amd.abi import RXR_ERR_INVALID, RXR_ERR_UNSUPPORTED, RXR_OK
from tests import trace_ref as TR
from tests import trace_scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NAMES = ["rxr_check_trace_scene", "rxr_set_trace_scene", "rxr_trace_srgb_table", "rxr_trace_rand", "rxr_trace", "rxr_trace_to", "rxr_accum_to_rgba", "rxr_accum_to_rgba_to"]


@pytest.fixture(scope="module")
def rxr():
    lib = rusterix_amd.rxr_abi()
    return lib


@pytest.fixture(scope="module")
def orc():
    from tests.oracle_api import load_oracle
    return load_oracle()


def test_header_mirror_and_exports_agree(rxr):
    header = open(os.path.join(ROOT, "include", "rxr.h")).read()
    rs = open(os.path.join(ROOT, "shim", "rusterix-hip-shim", "src", "ffi.rs")).read()
    for name in NAMES:
        assert f" {name}(" in header and f"pub fn {name}(" in rs and hasattr(rxr, name), name
    assert "#define RXR_ABI_VERSION 5u" in header and "pub const RXR_ABI_VERSION: u32 = 5;" in rs     # functions and #defines only
    for define, value in (("RXR_TRACE_CAMERA_FIRSTP", 0), ("RXR_TRACE_CAMERA_ORBIT", 1), ("RXR_TRACE_CAMERA_ISO", 2), ("RXR_TRACE_CAMERA_FLOATS", 14),
                          ("RXR_TRACE_NO_MATERIAL", 4294967295), ("RXR_TRACE_MAX_BOUNCES", 8)):
        assert f"pub const {define}: u32 = {value};" in rs, define
    assert (T.CAMERA_FIRSTP, T.CAMERA_ORBIT, T.CAMERA_ISO, T.NO_MATERIAL, T.MAX_BOUNCES) == (0, 1, 2, 4294967295, 8)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_ffi.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout


def test_every_refusal_of_check_trace_scene(rxr):
    msg = C.create_string_buffer(256)
    light = B.Light(B.LIGHT_POINT).compile()
    lights = (B.RxrLight * 2)(light, light)
    kinds = np.array([[T.MATTE, T.MOD_NONE], [T.NO_MATERIAL, 0], [T.EMISSIVE, T.MOD_INV_SATURATION]], np.uint32)
    values = np.array([0.5, 0.0, 1.0], F)
    lp, kp, vp = C.cast(lights, C.c_void_p), kinds.ctypes.data, values.ctypes.data

    def check(*args):
        msg.value = b""
        return rxr.rxr_check_trace_scene(*args, msg, 256), msg.value.decode()

    assert check(kp, vp, 3, lp, 2, 0) == (RXR_OK, "")
    assert check(None, None, 3, None, 0, 1) == (RXR_OK, "")
    assert check(None, None, 0, None, 0, 0) == (RXR_OK, "")
    for args, code, word in (((kp, vp, 3, None, 2, 0), RXR_ERR_INVALID, "lights is NULL"), ((kp, vp, 3, lp, 2, 2), RXR_ERR_INVALID, "sample mode"),
                             ((kp, None, 3, lp, 2, 0), RXR_ERR_INVALID, "come together"), ((None, vp, 3, lp, 2, 0), RXR_ERR_INVALID, "come together"),
                             ((kp, vp, 3, lp, 4097, 0), RXR_ERR_UNSUPPORTED, "RXR_TRACE_MAX_LIGHTS")):
        rc, text = check(*args)
        assert rc == code and word in text, (args, rc, text)
    bad = kinds.copy()
    bad[2, 0] = 5
    rc, text = check(bad.ctypes.data, vp, 3, lp, 2, 0)
    assert rc == RXR_ERR_INVALID and "mesh 2" in text and "role" in text
    bad = kinds.copy()
    bad[0, 1] = 5
    rc, text = check(bad.ctypes.data, vp, 3, lp, 2, 0)
    assert rc == RXR_ERR_INVALID and "mesh 0" in text and "modifier" in text
    lights[1].light_type = 6
    rc, text = check(kp, vp, 3, lp, 2, 0)
    assert rc == RXR_ERR_INVALID and "light 1" in text
    assert rxr.rxr_check_trace_scene(kp, vp, 3, lp, 2, 0, None, 0) == RXR_ERR_INVALID     # (no room for a message: the code alone)
    assert rxr.rxr_trace_srgb_table(None, None) == RXR_ERR_INVALID


def test_the_generator_is_the_librarys_and_uniform(rxr):
    rng = np.random.default_rng(1)
    for seed, frame, pixel, slot in rng.integers(0, 2 ** 32, size=(200, 4), dtype=np.uint64).tolist() + [[0, 0, 0, 0], [2 ** 32 - 1, 1, 0, 33], [7, 3, 2 ** 28, 2]]:
        want = TR.rand_f32(seed, frame, np.array([pixel], np.uint64), slot)[0]
        got = F(rxr.rxr_trace_rand(seed, frame, pixel, slot))
        assert got == want and 0.0 <= got < 1.0, (seed, frame, pixel, slot, got, want)
    # 2^20 draws: pixels x slots of one frame.  U[0, 1): mean 1/2 +- 4.4 sigma (sigma = 1 / sqrt(12 n)), variance 1/12 +- 5 sigma
    # (sigma = sqrt(1/180 / n))
    n = 1 << 20
    x = TR.rand_f32(5, 2, np.repeat(np.arange(1 << 15, dtype=np.uint64), 32), np.tile(np.arange(32, dtype=np.uint64), 1 << 15)).astype(np.float64)
    assert x.min() >= 0.0 and x.max() < 1.0
    assert abs(x.mean() - 0.5) < 4.4 / np.sqrt(12.0 * n)
    assert abs(x.var() - 1.0 / 12.0) < 5.0 * np.sqrt(1.0 / 180.0 / n)
    # neighbours across pixel, frame and slot differ (24-bit outputs: a chance collision among 3 x 2^16 pairs is expected about 0.01 times)
    base = np.arange(1 << 16, dtype=np.uint64)
    u = lambda frame, pixel, slot: TR.rand_u32(9, frame, pixel, slot)
    assert np.all(u(0, base, 2) != u(0, base + np.uint64(1), 2))
    assert np.all(u(0, base, 2) != u(0, base, 3))
    assert all(np.all(u(f, base, 2) != u(f + 1, base, 2)) for f in range(4))
    # successive draws of one pixel are uncorrelated (|r| < 5 / sqrt(n))
    a, b = TR.rand_f32(9, 0, base, 4).astype(np.float64), TR.rand_f32(9, 0, base, 5).astype(np.float64)
    assert abs(np.corrcoef(a, b)[0, 1]) < 5.0 / np.sqrt(len(base))


def test_the_srgb_table_is_within_one_ulp_of_the_tests_pow(rxr):
    table = np.zeros(256, F)
    assert rxr.rxr_trace_srgb_table(None, table.ctypes.data) == RXR_OK
    ref = TR.srgb_table()
    assert table[0] == 0.0 and table[255] == 1.0 and np.all(np.diff(table) > 0)
    assert np.all(np.abs(table.view(np.int32) - ref.view(np.int32)) <= 1)
    exact = np.arange(256) * (1.0 / 255.0)
    exact = np.where(exact <= 0.04045, exact / 12.92, ((exact + 0.055) / 1.055) ** 2.4)
    assert np.allclose(table, exact, rtol=1e-5)


def test_camera_constants_of_known_poses():
    kind, c = T.camera_firstp((0, 0, 0), (0, 0, -5), 90.0, 200, 100)
    assert kind == T.CAMERA_FIRSTP and c.dtype == F and c.shape == (14,)
    assert np.array_equal(c[3:6], [0, 0, -1]) and np.array_equal(c[6:9], [1, 0, 0]) and np.array_equal(c[9:12], [0, 1, 0])
    assert abs(c[13] - 1.0) < 1e-6 and c[12] == c[13] * F(2.0)
    kind, c = T.camera_orbit((1, 2, 3), 10.0, 0.0, 0.0, 90.0, 100, 100)
    assert kind == T.CAMERA_ORBIT and np.allclose(c[0:3], [11, 2, 3]) and np.allclose(c[3:6], [-1, 0, 0]) and np.allclose(c[9:12], [0, 1, 0])
    assert np.allclose(c[6:9], [0, 0, -1])                       # forward x up
    kind, c = T.camera_iso((0, 0, 0), 0.0, 0.0, 5.0, 4.0, 300, 100)
    assert kind == T.CAMERA_ISO and np.allclose(c[0:3], [5, 0, 0]) and np.allclose(c[3:6], [-1, 0, 0]) and c[13] == 4.0 and c[12] == F(12.0)
    # the restated rays of the first camera: the centre of the image looks along forward, the corners span the field of view
    o, d = TR.camera_rays(*T.camera_firstp((0, 0, 0), (0, 0, -5), 90.0, 2, 2), 2, 2, np.zeros(4, F), np.zeros(4, F))
    assert np.array_equal(o, np.zeros((4, 3), F))
    assert np.allclose(d[0] * np.sqrt(3.0), [-1, 1, -1], atol=1e-6) and np.allclose(d[3], [0, 0, -1], atol=1e-6)   # pixel (0,0): uv (0, 1), the top left


@pytest.fixture(scope="module")
def product():
    return rusterix_amd.load()


def bits_equal(got, ref, label):
    got, ref = np.ascontiguousarray(got, F), np.ascontiguousarray(ref, F)
    bad = np.argwhere(got.view(np.uint32) != ref.view(np.uint32))
    assert len(bad) == 0, f"{label}: {len(bad)} floats differ; first at {bad[0].tolist()}: got {got[tuple(bad[0])]!r}, expected {ref[tuple(bad[0])]!r}"


def mirror_cpu(product, rxr, orc, scene, camera, w, h, n_frames=1, seed=3, bounces=1, first_frame=0, threads=0, calls=1):
    """(the mirror's CPU trace, tests/trace_ref.py) from the same noise, through Scene.trace(cpu=True)"""
    scene = S.ordered(scene)
    sc, assets = S.mirror_scene(product, scene)
    acc = product.AccumBuffer(w, h)
    acc.pixels[:] = np.random.default_rng(w * 1000 + h).random((h, w, 4), dtype=F)
    acc.frame = first_frame
    start = acc.pixels.copy()
    for _ in range(calls):
        sc.trace(camera, acc, assets, n_frames=n_frames // calls, seed=seed, bounces=bounces, sample_mode=scene["sample_mode"], cpu=True, threads=threads)
    assert acc.frame == first_frame + n_frames
    table = np.zeros(256, F)
    assert rxr.rxr_trace_srgb_table(None, table.ctypes.data) == RXR_OK
    ref = TR.trace(orc, scene, camera, w, h, first_frame, n_frames, seed, bounces, start, table)
    return acc.pixels.copy(), ref


@pytest.mark.parametrize("size", [(1, 1), (9, 8), (17, 16), (37, 21)])
def test_mirror_cpu_one_bounce_is_bit_equal(product, rxr, orc, size):
    w, h = size
    got, ref = mirror_cpu(product, rxr, orc, S.room(), S.cameras(w, h)["firstp"], w, h, threads=3)
    bits_equal(got, ref, f"{w}x{h}")
    if w * h >= 64:
        assert (ref[..., :3] > 0).any() and len(np.unique(ref[..., 0])) > 4


@pytest.mark.parametrize("camera", ["firstp", "orbit", "iso"])
def test_mirror_cpu_cameras_are_bit_equal(product, rxr, orc, camera):
    got, ref = mirror_cpu(product, rxr, orc, S.room(), S.cameras(21, 13)[camera], 21, 13, first_frame=2)
    bits_equal(got, ref, camera)


def test_mirror_cpu_binding_cameras_feed_the_same_constants(product):
    cam = product.D3FirstPCamera.new()
    cam.position, cam.center, cam.fov = (4.0, 2.2, 0.6), (4.1, 1.9, 6.0), 70.0
    kind, consts = cam.trace_constants(21, 13)
    want = S.cameras(21, 13)["firstp"]
    assert kind == want[0] and np.array_equal(consts, want[1])
    orb = product.D3OrbitCamera.new()
    orb.center, orb.distance, orb.azimuth, orb.elevation, orb.fov = (4.0, 1.5, 4.5), 3.6, -1.5, 0.35, 75.0
    kind, consts = orb.trace_constants(21, 13)
    want = S.cameras(21, 13)["orbit"]
    assert kind == want[0] and np.array_equal(consts, want[1])
    # an oblique pose against a float64 evaluation of d3firstp.rs:116-121
    p, c = np.array([4.0, 2.2, 0.6]), np.array([4.1, 1.9, 6.0])
    f = (c - p) / np.linalg.norm(c - p)
    r = np.cross(f, [0, 1, 0]) / np.linalg.norm(np.cross(f, [0, 1, 0]))
    hh = np.tan(np.radians(70.0) * 0.5)
    k, got = cam.trace_constants(21, 13)
    assert np.allclose(got, np.concatenate([p, f, r, np.cross(r, f), [hh * 21 / 13, hh]]), rtol=2e-6, atol=2e-7)


def test_mirror_cpu_eight_mirror_bounces_and_the_running_average(product, rxr, orc):
    """every mesh Glossy at 1: eight reflections, no libm.  Four frames from frame 1 into noise, in one call and in four: the running
    average old * (1 - t) + new * t, t = 1 / (frame + 1), is the transcription's to the bit, and so is every bounce behind it"""
    glossy = (T.GLOSSY, T.MOD_NONE, 1.0)
    scene = S.room(material=glossy, panel_material=glossy)
    cam = S.cameras(16, 12)["firstp"]
    one, ref = mirror_cpu(product, rxr, orc, scene, cam, 16, 12, n_frames=4, seed=9, bounces=8, first_frame=1)
    four, _ = mirror_cpu(product, rxr, orc, scene, cam, 16, 12, n_frames=4, seed=9, bounces=8, first_frame=1, calls=4, threads=1)
    bits_equal(one, ref, "four frames in one call")
    bits_equal(four, ref, "four calls")


@pytest.mark.parametrize("sample_mode", [0, 1])
def test_mirror_cpu_sources_materials_and_terrain_are_bit_equal(product, rxr, orc, sample_mode):
    cam = S.cameras(16, 16)["firstp"]
    static = (T.SOURCE_STATIC_TILE, 0, (0, 0, 0, 0))
    for repeat, frame, source in ((0, 1, static), (1, 2, static), (2, 5, (T.SOURCE_STATIC_TILE, 1, (0, 0, 0, 0))), (3, 4, (T.SOURCE_DYNAMIC_TILE, 0, (0, 0, 0, 0))),
                                  (0, 1, (T.SOURCE_OTHER, 0, (9, 9, 9, 9))), (0, 1, S.PIXEL(90, 140, 250))):
        scene = S.room(box_source=source, sample_mode=sample_mode, box_repeat=repeat, animation_frame=frame, material=(T.METALLIC, repeat + 1, 0.6))
        scene["meshes"][-2]["uvs"] = (scene["meshes"][-2]["uvs"] * F(2.75) - F(0.8)).astype(F)
        got, ref = mirror_cpu(product, rxr, orc, scene, cam, 16, 16)
        bits_equal(got, ref, f"source {source[0]}, repeat {repeat}, sample mode {sample_mode}")
    got, ref = mirror_cpu(product, rxr, orc, S.terrain_room(), cam, 16, 16)
    bits_equal(got, ref, "terrain")
    lights = [S.point_light((3.5, 3.8, 3.0), kind=k, intensity=0.4, start=1.5, end=7.0, flicker=0.3) for k in (B.LIGHT_AREA, B.LIGHT_DAYLIGHT, B.LIGHT_AMBIENT)]
    got, ref = mirror_cpu(product, rxr, orc, S.room(lights=lights), cam, 16, 16)
    bits_equal(got, ref, "area, daylight and ambient lights")


def test_mirror_cpu_diffuse_paths_within_the_reference_tolerance(product, rxr, orc):
    """the GPU test's criterion for the host's cosf and sinf: S.diffuse_tolerance, at most 1 pixel in 50 outside"""
    scene, cam, w, h, seed = S.diffuse_case()
    sc, assets = S.mirror_scene(product, S.ordered(scene))
    acc = product.AccumBuffer(w, h)
    sc.trace(cam, acc, assets, n_frames=4, seed=seed, bounces=8, cpu=True)
    table = np.zeros(256, F)
    assert rxr.rxr_trace_srgb_table(None, table.ctypes.data) == RXR_OK
    ref, tolerance, disagree = S.diffuse_tolerance(orc, table)
    d = np.abs(acc.pixels - ref).max(axis=2)
    outside = int((d > tolerance).sum())
    print(f"mirror CPU, diffuse room {w}x{h}: tolerance {tolerance:.3e}, largest difference {d.max():.3e}, {outside} of {w * h} pixels outside")
    assert outside * 50 <= w * h


def test_mirror_to_u8_vec_bytes(product):
    """AccumBuffer::to_u8_vec of the mirror: a byte may differ from the float64 evaluation by one only where srgb * 255 + 0.5 lies
    within the pow bound of an integer (the rule of tests/test_bake_cpu.py)"""
    acc = product.AccumBuffer(64, 8)
    acc.pixels[:] = S.byte_rule_values(64, 8)
    got = acc.to_u8_vec()
    S.assert_byte_rule(got, acc.pixels)
    assert got[0, 0].tolist() == [0, 10, 255, 255] and np.array_equal(TR.to_u8(acc.pixels)[..., 3], got[..., 3])


def test_diffuse_reference_runs_agree(orc):
    """the experiment behind the GPU test's tolerance: the restated runs (cos and sin correctly rounded / moved by +-4 ulp) take the same
    paths in all but fewer than 1 pixel in 100 (half the share the device is allowed), and the tolerance they give is small"""
    scene, cam, w, h, seed = S.diffuse_case()
    ref, tolerance, disagree = S.diffuse_tolerance(orc, TR.srgb_table())
    print(f"diffuse room {w}x{h}: tolerance {tolerance:.3e}, {disagree} of {w * h} pixels disagree, image mean {ref[..., :3].mean():.4f}")
    assert disagree * 100 < w * h
    assert 0.0 < tolerance < 1e-3 * float(ref[..., :3].mean())
    assert (ref[..., :3] > 0).mean() > 0.9
