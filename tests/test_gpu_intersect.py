"""Ray picking on the device (rxr_intersect / rxr_intersect_to / rxr_screen_rays_to, Scene::intersect, Rasterizer::screen_ray)
against the numpy restatement of Scene::intersect (tests/intersect_ref.py), bit for bit: t, mesh, triangle, hitpoint and, in full
mode, uv and normal -- on the product scenes, chunk scenes whose profile ids decide the winner, overlays, a transformed mesh, the
1 M-triangle grid and adversarial rays.  Every scene runs twice: all rays in one call (a thread per ray once there are more than 64)
and in calls of 16 (a thread per triangle).  The kernels' thresholds -- ray counts, ray batches, segment ends, meshes without triangles,
two streams -- and seeded scenes are in tests/test_gpu_intersect_fuzz.py."""
import ctypes as C

import numpy as np
import pytest

import rusterix_amd
from rusterix_amd import binding as B
from rusterix_amd import scenes
from rusterix_amd.abi import RXR_ERR_INVALID, RXR_ERR_UNSUPPORTED, RXR_OK
from tests import intersect_ref as R

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture()
def plain_context(product):
    yield
    product.lib.rxh_set_device(0)
    product.lib.rxh_set_device_projection(0)


same = R.same   # bitwise equality; any NaN equals any NaN


def assert_same(got, ref, label=""):
    for k in ref:
        if not same(got[k], ref[k]):
            bad = np.nonzero(~np.all((got[k] == ref[k]).reshape(len(ref["t"]), -1), axis=1))[0]
            r = bad[0] if len(bad) else 0
            raise AssertionError(f"{label} {k}: {len(bad)} rays differ; ray {r}: got {got[k][r]!r} ({got['mesh'][r]}, {got['triangle'][r]}), "
                                 f"expected {ref[k][r]!r} ({ref['mesh'][r]}, {ref['triangle'][r]})")


def check(scene, meshes, origins, dirs, label=""):
    recs = [R.tri_records(m) for m in meshes]
    for full in (False, True):
        ref = R.intersect(meshes, origins, dirs, full=full, records=recs)
        assert_same(scene.intersect(origins, dirs, full=full), ref, f"{label} full={full} (one call)")
        parts = [scene.intersect(origins[i:i + 16], dirs[i:i + 16], full=full) for i in range(0, len(origins), 16)]
        assert_same({k: np.concatenate([p[k] for p in parts]) for k in ref}, ref, f"{label} full={full} (calls of 16)")
    return ref


def aimed_rays(meshes, eye, rng, n_targets=48, n_random=16):
    """rays from `eye` at triangle centroids, edge midpoints and vertices of random triangles, plus random directions"""
    tris = [(mi, k) for mi, m in enumerate(meshes) for k in range(len(m["indices"]))]
    pick = rng.choice(len(tris), size=min(n_targets, len(tris)), replace=False)
    targets = []
    for j, p in enumerate(pick):
        mi, k = tris[p]
        v = meshes[mi]["vertices"][meshes[mi]["indices"][k].astype(np.int64), :3].astype(F)
        kind = j % 3
        targets.append((v[0] + v[1] + v[2]) / F(3.0) if kind == 0 else ((v[0] + v[1]) * F(0.5) if kind == 1 else v[0]))
    eye = np.asarray(eye, F)
    o = np.repeat(eye[None, :], len(targets) + n_random, axis=0)
    d = np.concatenate([np.array(targets, F) - eye[None, :], rng.standard_normal((n_random, 3)).astype(F)])
    return o, d.astype(F)


def adversarial_rays(rng):
    """against the unit quad at z = 0 (triangles (0,1,2), (0,2,3)): grazing, t near 1e-4, degenerate directions, huge coordinates,
    exact edge / vertex hits and misses"""
    o, d = [], []
    target = np.array([0.6, 0.3, 0.0], F)
    for dz in (F(1e-6) * F(s) for s in (0.5, 0.999, 1.0, 1.001, 1.5, 3.0)):
        for sign in (1, -1):
            dd = np.array([1.0, 0.2, sign * dz], F)
            o.append(target - dd)
            d.append(dd)
    dd = np.array([0.0, 0.0, 1.0], F)
    for t0 in (9.9e-5, 1e-4, 1.0001e-4, 2e-4):
        base = F(t0)
        for ulp in (-2, -1, 0, 1, 2):
            t = np.float32(base + np.float32(ulp) * np.spacing(base))
            o.append(np.array([0.25, 0.75, -t], F))
            d.append(dd)
    for bad in ((0, 0, 0), (np.nan, 0, 1), (0, 0, np.inf), (np.inf, np.inf, np.inf), (0, 0, -0.0), (1e-40, 0, 1e-40)):
        o.append(np.array([0.3, 0.3, -1.0], F))
        d.append(np.array(bad, F))
    for big in (1e19, 1e30, 3e38):
        o.append(np.array([0.5, 0.25, -big], F))
        d.append(np.array([0.0, 0.0, 1.0], F))
        o.append(np.array([big, big, -big], F))
        d.append(np.array([0.5 - big, 0.25 - big, big], F))
    for p in ((0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0.5, 0.5, 0), (0.5, 0, 0), (1, 0.5, 0), (0.5, 1, 0), (0, 0.5, 0)):
        o.append(np.array(p, F) + np.array([0.0, 0.0, -2.0], F))
        d.append(np.array([0.0, 0.0, 1.0], F))
        o.append(np.array(p, F) + np.array([0.3, -0.2, -2.0], F))
        d.append(np.array([-0.3, 0.2, 2.0], F))
    for _ in range(8):  # misses
        o.append(np.array([5.0, 5.0, -1.0], F) + rng.standard_normal(3).astype(F))
        d.append(np.array([0.0, 0.0, 1.0], F))
    o.append(np.array([0.5, 0.5, -1.0], F))
    d.append(np.array([0.0, 0.0, -1.0], F))
    return np.array(o, F), np.array(d, F)


def unit_quad(api, z=0.0, normal=(0.0, 0.0, -1.0)):
    v = np.array([(0, 0, z, 1), (1, 0, z, 1), (1, 1, z, 1), (0, 1, z, 1)], F)
    b = api.Batch3D.new(v, np.array([(0, 1, 2), (0, 2, 3)], np.uint32), v[:, :2].copy())
    return b.normals(np.array([normal] * 4, F))


def build(product, builder):
    with R.recording(product) as meshes_of:
        cfg = builder(product)
    return cfg, meshes_of(cfg.scene)


def bbox_eye(meshes, k=1.5):
    v = np.concatenate([m["vertices"][:, :3] for m in meshes if len(m["vertices"])])
    lo, hi = v.min(axis=0), v.max(axis=0)
    return ((lo + hi) / 2 + (hi - lo) * np.array([0.3, k, 0.9], F) + F(1.0)).astype(F)


@pytest.mark.parametrize("name", ["cube", "teapot", "map"])
def test_product_scenes(product, plain_context, name):
    builder = dict(cube=lambda api: scenes.cube_scene(api, 160, 120, 40),
                   teapot=lambda api: scenes.teapot_scene(api, 160, 120, 40, logo_size=64),
                   map=lambda api: scenes.map_scene(api, 160, 96, 40, logo_size=64))[name]
    cfg, meshes = build(product, builder)
    rng = np.random.default_rng(11)
    o, d = aimed_rays(meshes, bbox_eye(meshes), rng)
    ref = check(cfg.scene, meshes, o, d, name)
    assert (ref["mesh"] != R.MISS).sum() >= (len(o) - 16) // 2   # (most aimed rays hit; the 16 random ones may not)


def test_adversarial_rays(product, plain_context):
    with R.recording(product) as meshes_of:
        scene = product.Scene.empty()
        scene.add_d3_static(unit_quad(product))
        scene.add_d3_static(product.Batch3D.from_box(3, 3, 3, 1, 1, 1).with_computed_normals())
        meshes = meshes_of(scene)
    o, d = adversarial_rays(np.random.default_rng(5))
    ref = check(scene, meshes, o, d, "adversarial")
    assert (ref["mesh"] == R.MISS).any() and (ref["mesh"] == 0).any()
    miss = ref["mesh"] == R.MISS
    assert np.all(ref["t"][miss] == R.FLT_MAX) and np.all(ref["triangle"][miss] == 0)


def panes_scene(api, second_chunk, pid_near):
    """a far opacity pane (profile id 5) and, nearer the viewer, a chunk batch with profile id `pid_near`: with 5 the reference keeps
    the farther pane (scene.rs:238-240); in the pane's chunk or a second one"""
    scene = api.Scene.empty()
    c0 = scene.add_chunk()
    c0.add_batch3d_opacity(api.Batch3D.from_box(-0.6, -0.6, -1.0, 1.2, 1.2, 0.02).with_computed_normals().profile_id(5))
    c1 = scene.add_chunk() if second_chunk else c0
    near = api.Batch3D.from_box(-1.5, -1.0, 1.0, 3.0, 2.0, 0.05).with_computed_normals()
    if pid_near is not None:
        near.profile_id(pid_near)
    c1.add_batch3d(near)
    scene.add_d3_static(api.Batch3D.from_box(-3.0, -3.0, -3.0, 6.0, 6.0, 0.1).with_computed_normals())
    return scene


def front_rays(n=9):
    xs = np.linspace(-1.2, 1.2, n, dtype=F)
    o = np.array([(x, y, 4.5) for x in xs for y in xs], F)
    d = np.repeat(np.array([[0.0, 0.0, -1.0]], F), len(o), axis=0)
    d[::3] += np.array([0.01, -0.02, 0.0], F)
    return o, d


@pytest.mark.parametrize("second_chunk", [False, True])
@pytest.mark.parametrize("pid_near", [5, 6, None])
def test_chunk_profile_ids(product, plain_context, second_chunk, pid_near):
    with R.recording(product) as meshes_of:
        scene = panes_scene(product, second_chunk, pid_near)
        meshes = meshes_of(scene)
    o, d = front_rays()
    ref = check(scene, meshes, o, d, "panes")
    centre = len(o) // 2
    assert ref["mesh"][centre] == (0 if pid_near == 5 else 1), "the profile-id rule is meant to decide this ray"


@pytest.mark.parametrize("k", [1, 2, 3])
def test_nested_windows_and_two_windows(product, plain_context, k):
    from tests.test_gpu_chunks import nested_windows_scene, two_window_scene

    for builder in (lambda api: nested_windows_scene(api, k), lambda api: two_window_scene(api, k == 2)):
        cfg, meshes = build(product, builder)
        o, d = front_rays()
        check(cfg.scene, meshes, o, d, "windows")


def test_overlay_meshes(product, plain_context):
    with R.recording(product) as meshes_of:
        scene = product.Scene.empty()
        scene.add_d3_static(unit_quad(product, 0.0))
        scene.add_d3_overlay(unit_quad(product, 5.0))
        scene.add_d3_static(unit_quad(product, 2.0))
        scene.add_d3_overlay(unit_quad(product, 3.0))
        scene.add_d3_dynamic(unit_quad(product, -0.5))
        meshes = meshes_of(scene)
    o, d = adversarial_rays(np.random.default_rng(9))
    ref = check(scene, meshes, o, d, "overlay")
    assert meshes[-1]["list"] == R.LIST_OVERLAY
    straight = (d[:, 2] > 0) & (d[:, 0] == 0) & (d[:, 1] == 0) & (o[:, 0] > 0) & (o[:, 0] < 1) & (o[:, 1] > 0) & (o[:, 1] < 1) & (o[:, 2] < -1)
    assert np.all(ref["mesh"][straight] == len(meshes) - 1)   # the last overlay hit wins, however far


def test_transform_is_ignored(product, plain_context):
    with R.recording(product) as meshes_of:
        scene = product.Scene.empty()
        b = unit_quad(product)
        b.transform(B.Mat4.translation_3d((10.0, 0.0, 0.0)))
        scene.add_d3_static(b)
        meshes = meshes_of(scene)
    o = np.array([[0.25, 0.75, -1.0], [10.25, 0.75, -1.0]], F)
    d = np.array([[0.0, 0.0, 1.0], [0.0, 0.0, 1.0]], F)
    ref = check(scene, meshes, o, d, "transform")
    assert ref["mesh"].tolist() == [0, R.MISS]


@pytest.fixture(scope="module")
def grid(product):
    return build(product, lambda api: scenes.box_grid_scene(api, width=320, height=200))


def test_box_grid(product, plain_context, grid):
    cfg, meshes = grid
    assert sum(len(m["indices"]) for m in meshes) > 1_000_000
    rng = np.random.default_rng(3)
    o, d = aimed_rays(meshes, bbox_eye(meshes, 0.4), rng, n_targets=72, n_random=8)
    ref = check(cfg.scene, meshes, o[:80], d[:80], "grid")
    assert (ref["mesh"] != R.MISS).sum() >= 40


def test_screen_rays_and_pick_buffer(product, plain_context):
    import torch

    cfg, meshes = build(product, lambda api: scenes.map_scene(api, 320, 200, 40, logo_size=64))
    r = cfg.setup()
    r.rasterize(cfg.scene, np.zeros(320 * 200 * 4, np.uint8), 320, 200, 40, cfg.assets)
    iv, ip, _ = r.derived()
    ctx = product.lib.rxh_context()
    rxr = rusterix_amd.rxr_abi()
    W, H = 320, 200
    o = torch.empty((W * H, 3), dtype=torch.float32, device="cuda")
    d = torch.empty_like(o)
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    x0, y0, w, h = 17, 23, 40, 30
    assert rxr.rxr_screen_rays_to(ctx, iv.ctypes.data, ip.ctypes.data, float(W), float(H), x0, y0, w, h, o.data_ptr(), d.data_ptr(), sp) == RXR_OK
    stream.synchronize()
    got_o, got_d = o[:w * h].cpu().numpy(), d[:w * h].cpu().numpy()
    for j in range(h):
        for i in range(w):
            ro, rd = r.screen_ray(x0 + i, y0 + j)
            assert same(got_o[j * w + i], ro) and same(got_d[j * w + i], rd), (i, j)
    # the whole 320 x 200 pick buffer: screen rays, then rxr_intersect_to on the same stream, against the host-array call
    assert rxr.rxr_screen_rays_to(ctx, iv.ctypes.data, ip.ctypes.data, float(W), float(H), 0, 0, W, H, o.data_ptr(), d.data_ptr(), sp) == RXR_OK
    n = W * H
    t = torch.empty(n, dtype=torch.float32, device="cuda")
    mesh = torch.empty(n, dtype=torch.int32, device="cuda")
    tri = torch.empty_like(mesh)
    hp = torch.empty((n, 3), dtype=torch.float32, device="cuda")
    uv = torch.empty((n, 2), dtype=torch.float32, device="cuda")
    nrm = torch.empty((n, 3), dtype=torch.float32, device="cuda")
    host = cfg.scene.intersect(np.zeros((1, 3), F), np.ones((1, 3), F))  # (registers this scene's meshes)
    assert host["t"].shape == (1,)
    assert rxr.rxr_intersect_to(ctx, o.data_ptr(), d.data_ptr(), n, 1, t.data_ptr(), mesh.data_ptr(), tri.data_ptr(), hp.data_ptr(),
                                uv.data_ptr(), nrm.data_ptr(), sp) == RXR_OK
    stream.synchronize()
    ho, hd = o.cpu().numpy(), d.cpu().numpy()
    ref = cfg.scene.intersect(ho, hd, full=True)
    got = dict(t=t.cpu().numpy(), mesh=mesh.cpu().numpy().view(np.uint32), triangle=tri.cpu().numpy().view(np.uint32),
               hitpoint=hp.cpu().numpy(), uv=uv.cpu().numpy(), normal=nrm.cpu().numpy())
    assert_same(got, ref, "pick buffer")
    assert (ref["mesh"] != R.MISS).mean() > 0.5
    sub = np.arange(0, n, 997)
    assert_same({k: v[sub] for k, v in ref.items()}, R.intersect(meshes, ho[sub], hd[sub], full=True), "pick buffer vs numpy")
    # ... and every ray of the buffer against the vectorised reference
    assert_same(got, R.intersect_many(meshes, ho, hd, full=True), "the whole pick buffer vs numpy")


def test_new_meshes_are_hit_no_stale_records(product, plain_context):
    o = np.array([[0.25, 0.75, -1.0]], F)
    d = np.array([[0.0, 0.0, 1.0]], F)
    a = product.Scene.empty().add_d3_static(unit_quad(product, 0.0))
    b = product.Scene.empty().add_d3_static(unit_quad(product, 2.0))
    assert a.intersect(o, d)["t"][0] == 1.0
    assert b.intersect(o, d)["t"][0] == 3.0
    assert a.intersect(o, d)["t"][0] == 1.0
    # ... and through the ABI: rxr_set_meshes with other geometry on the same context
    ctx = product.lib.rxh_context()
    rxr = rusterix_amd.rxr_abi()
    assert rxr.rxr_intersect(ctx, None, d.ctypes.data, 1, 0, None, None, None, None, None, None) == RXR_ERR_INVALID
    out = np.zeros(4, F)
    assert rxr.rxr_intersect(ctx, o.ctypes.data, d.ctypes.data, 0, 0, out.ctypes.data, out.ctypes.data, out.ctypes.data, None, None, None) == RXR_OK
    assert rxr.rxr_intersect(ctx, o.ctypes.data, d.ctypes.data, 1, 2, out.ctypes.data, out.ctypes.data, out.ctypes.data, None, None, None) == RXR_ERR_INVALID


def test_a_fresh_context_misses_everything(product):
    rxr = rusterix_amd.rxr_abi()
    ctx = C.c_void_p()
    assert rxr.rxr_create(C.byref(ctx), 0) == RXR_OK
    try:
        o, d = adversarial_rays(np.random.default_rng(1))
        n = len(o)
        t, m, tri, hp = np.zeros(n, F), np.zeros(n, np.uint32), np.ones(n, np.uint32), np.ones((n, 3), F)
        assert rxr.rxr_intersect(ctx, o.ctypes.data, d.ctypes.data, n, 1, t.ctypes.data, m.ctypes.data, tri.ctypes.data, hp.ctypes.data, None, None) == RXR_OK
        assert np.all(t == R.FLT_MAX) and np.all(m == R.MISS) and np.all(tri == 0) and np.all(hp == 0)
        assert rxr.rxr_screen_rays_to(ctx, None, o.ctypes.data, 1.0, 1.0, 0, 0, 1, 1, o.ctypes.data, d.ctypes.data, None) == RXR_ERR_INVALID
        assert rxr.rxr_intersect_to(ctx, o.ctypes.data, None, 1, 0, t.ctypes.data, m.ctypes.data, tri.ctypes.data, None, None, None, None) == RXR_ERR_INVALID
    finally:
        rxr.rxr_destroy(ctx)


@pytest.mark.parametrize("device_projection", [0, 1])
def test_frames_around_intersect_calls_are_identical(product, plain_context, device_projection):
    product.lib.rxh_set_device_projection(device_projection)
    cfg, meshes = build(product, lambda api: scenes.map_scene(api, 320, 192, 40, logo_size=64))
    before = scenes.render(cfg).copy()
    o, d = aimed_rays(meshes, bbox_eye(meshes), np.random.default_rng(2))
    cfg.scene.intersect(o, d, full=True)
    after = scenes.render(cfg).copy()
    other = product.Scene.empty().add_d3_static(unit_quad(product))   # other geometry: registered again, then the frame's again
    other.intersect(o, d)
    again = scenes.render(cfg).copy()
    assert np.array_equal(before, after) and np.array_equal(before, again)
    # upload, intersect, render: the intersect of the same geometry leaves the uploaded frame alone
    host = product.lib
    host.rxh_rasterizer_upload.restype = C.c_int
    r = cfg.setup()
    assert host.rxh_rasterizer_upload(r._h, cfg.scene._h, cfg.width, cfg.height, cfg.tile_size, cfg.assets._h) == 0
    if device_projection:
        cfg.scene.intersect(o, d)
    ctx = host.rxh_context()
    rxr = rusterix_amd.rxr_abi()
    px = np.zeros(cfg.width * cfg.height * 4, np.uint8)
    assert rxr.rxr_render_download(ctx, px.ctypes.data) == RXR_OK
    assert np.array_equal(px.reshape(before.shape), before)
    words = (C.c_uint32 * 4)()
    assert rxr.rxr_debug_scratch(ctx, words) == 0
    assert list(words) == [0, 0, 0, 0]


def test_group_context(product, plain_context):
    cfg, meshes = build(product, lambda api: scenes.cube_scene(api, 160, 120, 40))
    o, d = aimed_rays(meshes, bbox_eye(meshes), np.random.default_rng(4))
    single = cfg.scene.intersect(o, d, full=True)
    ids = (C.c_int * 2)(0, 0)
    product.lib.rxh_set_devices(ids, 2)
    ctx = product.lib.rxh_context()
    rxr = rusterix_amd.rxr_abi()
    assert rxr.rxr_member_count(ctx) == 2
    assert_same(cfg.scene.intersect(o, d, full=True), single, "group")
    assert_same(single, R.intersect(meshes, o, d, full=True), "group vs numpy")
    buf = np.zeros(16, F)
    p = buf.ctypes.data
    assert rxr.rxr_intersect_to(ctx, p, p, 1, 0, p, p, p, None, None, None, None) == RXR_ERR_UNSUPPORTED
    assert rxr.rxr_screen_rays_to(ctx, p, p, 1.0, 1.0, 0, 0, 1, 1, p, p, None) == RXR_ERR_UNSUPPORTED
