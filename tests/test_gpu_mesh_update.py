"""rxr_update_meshes / rxr_update_meshes_to / rxr_mesh_bounds on the GPU (include/rxr.h; kernels k_mesh_check, k_mesh_commit in
rxr_project.hip).

The main assertion is EQUIVALENCE: context A gets rxr_set_meshes(new geometry); context B gets rxr_set_meshes(old geometry) and an
update to the new geometry.  Then the same device-projected 160 x 96 frame is byte-equal, rxr_read_projected_mesh is word-equal for
every mesh (the untouched neighbours included), rxr_mesh_bounds is equal under == and rxr_intersect is bit-equal on seeded rays.
A refused call leaves B rendering (WITHOUT a new upload: the resident frame is kept), picking and bounded exactly as before it.
The end-to-end half drives the host mirror: Scene.rebuild_terrain_meshes against the old route (Terrain.build_meshes, the batch
replaced, the scene registered again)."""
import ctypes as C

import numpy as np
import pytest

import rusterix_amd
from rusterix_amd import binding as B
from rusterix_amd.abi import RXR_ERR_INVALID, RXR_ERR_UNSUPPORTED, RXR_OK, rxr_frame as Frame
from tests import mesh_update_ref as M
from tests.pick_fuzz import IDENTITY, Mesh3D, PickContext

pytestmark = pytest.mark.gpu
F = np.float32
W, H = 160, 96


def camera(product, position=(0.0, 0.0, 0.0), center=(0.0, 0.0, -6.0)):
    cam = product.D3FirstPCamera.new()
    cam.position, cam.center = position, center
    v, p = cam.matrices(float(W), float(H))
    iv, ip, cp = product.Rasterizer.setup(None, v, p).derived()
    return dict(view=v, projection=p, inverse_view=iv, inverse_projection=ip, camera_pos=cp)


LIGHT = B.Light(B.LIGHT_POINT).with_position((1.5, 2.0, -2.0)).with_color((1.0, 0.9, 0.7)).with_intensity(2.0).with_start_distance(1.0).with_end_distance(30.0).compile()


class Ctx(PickContext):
    """a context of its own: meshes with a colour each, one device-projected lit frame, the debugging read-backs, both update forms"""

    def __init__(self):
        super().__init__()
        self.meshes = []

    def set_meshes(self, meshes, expect=RXR_OK):
        arr = (Mesh3D * max(len(meshes), 1))()
        keep = []
        for k, (a, m) in enumerate(zip(arr, meshes)):
            v, i, uv, nr = (np.ascontiguousarray(m[key], t) for key, t in (("vertices", F), ("indices", np.uint32), ("uvs", F), ("normals", F)))
            keep += [v, i, uv, nr]
            a.vertices, a.indices, a.uvs, a.normals = v.ctypes.data, i.ctypes.data, uv.ctypes.data, nr.ctypes.data
            a.n_vertices, a.n_triangles = len(v.reshape(-1, 4)), len(i.reshape(-1, 3))
            a.transform_3d = IDENTITY
            a.source.kind = B.SOURCE_PIXEL
            a.source.pixel = (C.c_uint8 * 4)(60 + 37 * k % 190, 250 - 53 * k % 190, 90 + 91 * k % 160, 255)
            a.shader, a.list, a.chunk = -1, m["list"], m.get("chunk", -1)
        rc = self.rxr.rxr_set_meshes(self.ctx, C.cast(arr, C.c_void_p), len(meshes))
        assert rc == expect, f"rxr_set_meshes: {rc}: {self.error()}"
        self.meshes = list(meshes)

    def upload(self, cam):
        f = Frame()
        f.abi_version, f.width, f.height, f.tile_size = 5, W, H, 32
        for k in ("view", "projection", "inverse_view", "inverse_projection"):
            setattr(f, k, (C.c_float * 16)(*cam[k]))
        f.camera_pos = (C.c_float * 3)(*cam["camera_pos"])
        f.scaled2, f.flags = 1.0, (1 << 1) | (1 << 4) | (1 << 5)     # 3D on, a background colour, ambient
        f.background_color = (C.c_uint8 * 4)(10, 20, 30, 255)
        f.ambient = (C.c_float * 4)(0.4, 0.4, 0.4, 1.0)
        light = (B.RxrLight * 1)(LIGHT)
        f.lights, f.n_lights = light, 1
        f.use_meshes = 1
        rc = self.rxr.rxr_upload_frame(self.ctx, C.byref(f))
        assert rc == RXR_OK, f"rxr_upload_frame: {rc}: {self.error()}"

    def render(self):
        """the resident frame (RXR_ERR_INVALID when there is none)"""
        px = np.zeros((H, W, 4), np.uint8)
        rc = self.rxr.rxr_render_download(self.ctx, px.ctypes.data)
        return rc, px

    def frame(self, cam):
        self.upload(cam)
        rc, px = self.render()
        assert rc == RXR_OK, self.error()
        return px

    def projected(self, index):
        m = self.meshes[index]
        nv, nt = len(m["vertices"]), len(m["indices"])
        cv, ct = nv + 4 * nt + 1, 3 * nt + 1
        counts = (C.c_uint32 * 2)()
        out = dict(pv=np.zeros((cv, 4), F), uv=np.zeros((cv, 2), F), nrm=np.zeros((cv, 3), F), idx=np.zeros((ct, 3), np.uint32),
                   edges=np.zeros((ct, 10), np.uint32), bbox=np.zeros(5, F))
        rc = self.rxr.rxr_read_projected_mesh(self.ctx, index, C.cast(counts, C.c_void_p), *(out[k].ctypes.data for k in ("pv", "uv", "nrm", "idx", "edges", "bbox")), cv, ct)
        assert rc == RXR_OK, self.error()
        words = [np.array(counts[:], np.uint32)]
        for k, n in (("pv", counts[0]), ("uv", counts[0]), ("nrm", counts[0]), ("idx", counts[1]), ("edges", counts[1]), ("bbox", 5)):
            words.append(out[k][:n].view(np.uint32).ravel())
        return np.concatenate(words)

    def bounds(self, index):
        lo, hi = (C.c_float * 3)(), (C.c_float * 3)()
        assert self.rxr.rxr_mesh_bounds(self.ctx, index, lo, hi) == RXR_OK, self.error()
        return np.array(lo[:], F), np.array(hi[:], F)

    def update(self, named, new_meshes, form="host", stream=None, **pack):
        """the update of meshes `named` to `new_meshes` (same order); the status"""
        counts, v, i, nr = M.pack(new_meshes, **pack)
        return self.update_arrays(named, counts, v, i, nr, form, stream)

    def update_arrays(self, named, counts, v, i, nr, form="host", stream=None):
        named = np.ascontiguousarray(named, np.uint32)
        if form == "host":
            return self.rxr.rxr_update_meshes(self.ctx, named.ctypes.data, len(named), counts.ctypes.data, v.ctypes.data, i.ctypes.data, nr.ctypes.data,
                                              v.shape[1], i.shape[1])
        import torch

        s = stream or torch.cuda.Stream()
        with torch.cuda.stream(s):     # written on that stream just before the call: the call must order itself behind them
            dev = [torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to("cuda", non_blocking=False).clone() for a in (counts, v, i, nr)]
        rc = self.rxr.rxr_update_meshes_to(self.ctx, named.ctypes.data, len(named), *(max(d.data_ptr(), 0) or None for d in dev), v.shape[1], i.shape[1], s.cuda_stream)
        torch.cuda.synchronize()
        return rc


def rays(seed, n=48):
    rng = np.random.default_rng(seed)
    o = (rng.random((n, 3), dtype=F) - F(0.5)) * F(0.5)
    target = (rng.random((n, 3), dtype=F) * 2 - 1) * F(2.2) + np.array([0, 0, -6], F)
    return o, (target - o).astype(F)


def snapshot(ctx, cam, seed=3):
    """everything the equivalence compares, as a dict of arrays"""
    snap = dict(frame=ctx.frame(cam))
    for k in range(len(ctx.meshes)):
        snap[f"mesh{k}"] = ctx.projected(k)
        snap[f"lo{k}"], snap[f"hi{k}"] = ctx.bounds(k)
    o, d = rays(seed)
    for k, a in ctx.intersect(o, d, full=True).items():
        snap["ray_" + k] = a
    return snap


def assert_same(a, b, label=""):
    assert a.keys() == b.keys()
    for k in a:
        if k[:2] in ("lo", "hi"):
            assert (a[k] == b[k]).all(), (label, k, a[k], b[k])     # under ==: the sign of a zero bound is not specified
        else:
            x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
            assert x.shape == y.shape and x.tobytes() == y.tobytes(), (label, k, int((x.view(np.uint8) != y.view(np.uint8)).sum()))


@pytest.fixture(scope="module")
def pair(product):
    a, b = Ctx(), Ctx()
    yield a, b, camera(product)
    a.close()
    b.close()


def equivalent(pair, old, new, named, form, cam=None, order=None, **pack):
    """A: set_meshes(new).  B: set_meshes(old), one frame (so a resident frame and pick records exist), update of `named` to new."""
    a, b, default_cam = pair
    cam = cam or default_cam
    a.set_meshes(new)
    want = snapshot(a, cam)
    b.set_meshes(old)
    before = snapshot(b, cam)
    order = list(named) if order is None else order
    rc = b.update(order, [new[k] for k in order], form, **pack)
    assert rc == RXR_OK, b.error()
    assert b.render()[0] == RXR_ERR_INVALID, "the resident frame must be dropped by an accepted update"
    b.meshes = list(new)
    got = snapshot(b, cam)
    assert_same(got, want, f"{form} {named}")
    return before, got


FORMS = ["host", "to"]


def three(seed=0, nv=(30, 50, 40), nt=(20, 40, 30)):
    centres = ((-2.0, 0.5, -6.0), (0.0, -0.5, -7.0), (2.0, 0.5, -6.0))
    return [M.grid_mesh(nv[k], nt[k], seed + k, centre=centres[k], extent=1.0) for k in range(3)]


# ---- equivalence ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("named", [[0], [1], [2], [2, 0, 1]], ids=["first", "middle", "last", "all-shuffled"])
def test_one_of_three_meshes_and_all_three(pair, named, form):
    old = three()
    new = [M.moved(m, 100 + k) if k in named else m for k, m in enumerate(old)]
    before, got = equivalent(pair, old, new, named, form)
    assert before["frame"].tobytes() != got["frame"].tobytes(), "the update should show in the frame"
    assert len(np.unique(got["frame"].reshape(-1, 4), axis=0)) > 20 and (got["ray_mesh"] != 0xFFFFFFFF).any()


def with_extreme(mesh, at):
    """vertex `at` becomes the box's extreme in x (max), y (min) and z (min)"""
    m = dict(mesh)
    v = np.array(m["vertices"], F)
    v[at, :3] = (F(3.25), F(-3.5), F(-9.75))
    m["vertices"] = v
    return m


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("nv", [1, 63, 64, 65, 255, 256, 257, 1025, 4225])
def test_vertex_counts_with_the_extreme_vertex_first_last_and_in_the_last_partial_wave(pair, nv, form):
    """three meshes of nv vertices, all updated in one call: the extreme vertex first, last, and first of the last (partial) wave --
    alone in it when nv % 64 == 1"""
    places = [0, nv - 1, (nv - 1) // 64 * 64]
    old = [M.grid_mesh(nv, 4, 10 + k, extent=1.5) for k in range(3)]
    new = [with_extreme(M.moved(m, 200 + k, extent=1.5), places[k]) for k, m in enumerate(old)]
    _, got = equivalent(pair, old, new, [0, 1, 2], form)
    for k in range(3):
        lo, hi = M.box_fast(new[k]["vertices"])
        assert (got[f"lo{k}"] == lo).all() and (got[f"hi{k}"] == hi).all()
        assert hi[0] == F(3.25) and lo[1] == F(-3.5) and lo[2] == F(-9.75)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("nt", [1, 85, 86, 8192])
def test_triangle_counts_around_256_index_words(pair, nt, form):
    old = [M.grid_mesh(40, nt, 20, extent=1.2), M.grid_mesh(7, 3, 21, centre=(2.5, 0, -6), extent=0.5)]
    new = [M.moved(old[0], 300, extent=1.2), old[1]]
    new[0]["indices"][-1] = (39, 0, 39)      # (the largest legal index in the last word)
    equivalent(pair, old, new, [0], form)


@pytest.mark.parametrize("form", FORMS)
def test_a_mesh_without_vertices_updated_with_counts_zero(pair, form):
    old = three()
    old[1] = M.grid_mesh(0, 0, 0)
    new = [M.moved(old[0], 400), M.grid_mesh(0, 0, 1), old[2]]
    _, got = equivalent(pair, old, new, [0, 1], form)
    assert (got["lo1"] == np.inf).all() and (got["hi1"] == -np.inf).all()


@pytest.mark.parametrize("form", FORMS)
def test_300_one_triangle_meshes_cross_the_launch_cut(pair, form):
    rng = np.random.default_rng(7)
    old = [M.grid_mesh(3, 1, 500 + k, centre=(rng.uniform(-3, 3), rng.uniform(-2, 2), -6.0), extent=0.3) for k in range(300)]
    for m in old:
        m["indices"][:] = (0, 1, 2)
    new = [M.moved(m, 900 + k, extent=0.3) for k, m in enumerate(old)]
    for m in new:
        m["indices"][:] = (2, 1, 0)
    order = list(rng.permutation(300))
    equivalent(pair, old, new, list(range(300)), form, order=order)


@pytest.mark.parametrize("form", FORMS)
def test_strides_beyond_the_counts_with_poisoned_slack(pair, form):
    old = three()
    new = [M.moved(m, 600 + k) for k, m in enumerate(old)]
    equivalent(pair, old, new, [0, 1, 2], form, vstride=131, tstride=77, slack=True)


# ---- the box ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_nan_vertices_are_ignored_and_an_all_nan_mesh_keeps_infinities(pair, form):
    old = three()
    new = [M.moved(m, 700 + k) for k, m in enumerate(old)]
    new[0]["vertices"][5, 0] = np.nan       # one coordinate: the vertex's y and z still count
    new[0]["vertices"][9, :3] = np.nan
    new[1]["vertices"][:, :3] = np.nan      # nothing but NaN
    _, got = equivalent(pair, old, new, [0, 1, 2], form)
    lo, hi = M.box(new[0]["vertices"])
    assert np.isfinite(lo).all() and (got["lo0"] == lo).all() and (got["hi0"] == hi).all()
    assert (got["lo1"] == np.inf).all() and (got["hi1"] == -np.inf).all()


@pytest.mark.parametrize("form", FORMS)
def test_zero_bounds_of_either_sign_compare_equal(pair, form):
    old = three()
    new = list(old)
    new[1] = M.moved(old[1], 710)
    v = new[1]["vertices"]
    v[:, 0] = np.where(np.arange(len(v)) % 2 == 0, F(-0.0), F(0.0))      # x: lo == hi == 0, of whichever sign
    v[:, 1] = np.minimum(v[:, 1], F(0.0))
    v[::3, 1] = F(-0.0)                                                   # y: hi is a zero
    _, got = equivalent(pair, old, new, [1], form)
    assert got["lo1"][0] == 0 and got["hi1"][0] == 0 and got["hi1"][1] == 0


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("direction", ["leaves", "enters"])
def test_the_frustum_cull_reads_the_new_box(pair, product, direction, form):
    """the new geometry wholly outside the frustum while the old was inside, and the reverse: the cull reads aabb_lo / hi"""
    inside, outside = three(), three()
    outside[1] = M.moved(inside[1], 720, centre=(0.0, 0.0, 40.0), extent=1.0)      # behind the camera
    old, new = (inside, outside) if direction == "leaves" else (outside, inside)
    before, got = equivalent(pair, old, new, [1], form)
    assert before["frame"].tobytes() != got["frame"].tobytes()
    rejected = (got if direction == "leaves" else before)["mesh1"]
    assert rejected[0] == 0 and rejected[1] == 0, "the mesh behind the camera should have been culled"


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def refused(b, cam, call, why):
    """`call()` is RXR_ERR_INVALID with `why` in the message, and B renders the RESIDENT frame, picks and is bounded as before"""
    before = snapshot(b, cam)
    rc = call()
    assert rc == RXR_ERR_INVALID, (rc, b.error())
    assert why in b.error(), b.error()
    rc, px = b.render()                      # (no upload in between: the frame must still be resident)
    assert rc == RXR_OK and px.tobytes() == before["frame"].tobytes()
    assert_same(snapshot(b, cam), before, why)


@pytest.mark.parametrize("form", FORMS)
def test_refusals_found_by_the_check_kernel_change_nothing(pair, form):
    _, b, cam = pair
    old = three()
    b.set_meshes(old)
    new = [M.moved(m, 800 + k) for k, m in enumerate(old)]
    bad = [dict(m) for m in new]
    bad[2] = dict(new[2], indices=new[2]["indices"].copy())
    bad[2]["indices"][-1, 2] = len(new[2]["vertices"])          # == n_vertices, the last word of the last named mesh
    refused(b, cam, lambda: b.update([0, 1, 2], bad, form), "mesh_indices[2] = 2: triangle 29 has a vertex index")
    for which, k, msg in (("vertices", 0, "vertex count"), ("indices", 1, "triangle count")):
        for delta in (-1, 1):
            counts, v, i, nr = M.pack(new, vstride=60, tstride=50, slack=True)
            col = 0 if which == "vertices" else 1
            counts[k, col] = int(counts[k, col]) + delta
            refused(b, cam, lambda: b.update_arrays([0, 1, 2], counts, v, i, nr, form), f"mesh_indices[{k}] = {k}: its {msg} differs")
    # ... and the same arrays, untouched, are accepted afterwards
    assert b.update([0, 1, 2], new, form) == RXR_OK, b.error()


@pytest.mark.parametrize("form", FORMS)
def test_refusals_found_on_the_host_change_nothing(pair, form):
    _, b, cam = pair
    old = three()
    b.set_meshes(old)
    new = [M.moved(m, 810 + k) for k, m in enumerate(old)]
    refused(b, cam, lambda: b.update([0, 1, 0], [new[0], new[1], new[0]], form), "named twice")
    refused(b, cam, lambda: b.update([0, 3], [new[0], new[1]], form), "no such mesh")
    refused(b, cam, lambda: b.update([0, 1, 2], new, form, vstride=49), "vertex_stride 49 is below its 50 vertices")
    refused(b, cam, lambda: b.update([0, 1, 2], new, form, tstride=39), "triangle_stride 39 is below its 40 triangles")
    counts, v, i, nr = M.pack(new)
    named = np.arange(3, dtype=np.uint32)
    args = (named.ctypes.data, 1 << 31, counts.ctypes.data, v.ctypes.data, i.ctypes.data, nr.ctypes.data, 0xFFFFFFFF, 0xFFFFFFFF)
    if form == "host":
        refused(b, cam, lambda: b.rxr.rxr_update_meshes(b.ctx, *args), "sizes overflow")
        refused(b, cam, lambda: b.rxr.rxr_update_meshes(b.ctx, named.ctypes.data, 3, counts.ctypes.data, None, i.ctypes.data, nr.ctypes.data, 50, 40), "NULL")
    else:
        import torch

        refused(b, cam, lambda: b.rxr.rxr_update_meshes_to(b.ctx, *args, None), "sizes overflow")
        dev = [torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda() for a in (counts, v, i, nr)]
        torch.cuda.synchronize()
        p = [d.data_ptr() for d in dev]
        # a host pointer, an odd address, a NULL pointer
        refused(b, cam, lambda: b.rxr.rxr_update_meshes_to(b.ctx, named.ctypes.data, 3, p[0], v.ctypes.data, p[2], p[3], 50, 40, None), "dev_vertices is not device memory")
        refused(b, cam, lambda: b.rxr.rxr_update_meshes_to(b.ctx, named.ctypes.data, 3, p[0], p[1], p[2] + 1, p[3], 50, 40, None), "dev_indices must be 4-byte aligned")
        refused(b, cam, lambda: b.rxr.rxr_update_meshes_to(b.ctx, named.ctypes.data, 3, p[0], p[1], p[2], None, 50, 40, None), "dev_normals must be 4-byte aligned")
    assert b.update([0, 1, 2], new, form) == RXR_OK, b.error()


def test_no_valid_registration_and_the_empty_call():
    with Ctx() as c:
        one = M.grid_mesh(3, 1, 1)
        assert c.update([], [], "host") == RXR_OK                       # n == 0 does nothing, registration or not
        assert c.update([0], [one], "host") == RXR_ERR_INVALID and "no such mesh" in c.error()
        broken = dict(one, indices=np.array([[0, 1, 3]], np.uint32))
        c.set_meshes([one, broken], expect=RXR_ERR_INVALID)             # (leaves the context without a valid registration)
        assert c.update([0], [one], "host") == RXR_ERR_INVALID and "no valid registration" in c.error()
        assert c.update([0], [one], "to") == RXR_ERR_INVALID and "no valid registration" in c.error()
        c.set_meshes([one])
        assert c.update([0], [M.moved(one, 2)], "host") == RXR_OK, c.error()


# ---- multi-device handles --------------------------------------------------------------------------------------------------------------
def test_a_group_of_one_device_takes_the_host_form_only(pair, product):
    a, _, cam = pair
    old = three()
    new = [M.moved(m, 820 + k) for k, m in enumerate(old)]
    g = Ctx()
    g.close()                                                            # (a handle of rxr_create_multi in the plain one's place)
    devs = (C.c_int * 1)(0)
    assert g.rxr.rxr_create_multi(C.byref(g.ctx), devs, 1) == RXR_OK
    try:
        g.set_meshes(old)
        assert g.update([2, 0], [new[2], new[0]], "to") == RXR_ERR_UNSUPPORTED and "multi-device" in g.error()
        assert g.update([2, 0], [new[2], new[0]], "host") == RXR_OK, g.error()
        a.set_meshes([new[0], old[1], new[2]])
        for k in range(3):
            assert all((x == y).all() for x, y in zip(g.bounds(k), a.bounds(k)))
        g.meshes = [new[0], old[1], new[2]]
        assert g.frame(cam).tobytes() == a.frame(cam).tobytes()
        assert g.update([1, 1], [new[1], new[1]], "host") == RXR_ERR_INVALID and "named twice" in g.error()
    finally:
        g.close()


# ---- end to end: the host mirror ---------------------------------------------------------------------------------------------------------
CS, CELLS = 16, 32
COORDS = [(0, 0), (1, 0), (0, 1), (1, 1)]


def height(x, y):
    return float(F(0.8 * np.sin(x / 3.0) * np.cos(y / 4.0)))


def terrain_scene(api, heights):
    """a 32 x 32-cell terrain in four chunks of 16, one terrain_batch3d each, and a static box; returns (terrain, scene, render)"""
    t = api.Terrain((1.0, 1.0), CS)
    for (x, y), h in heights.items():
        t.set_height(x, y, h)
    scene = api.Scene.empty()
    for k, mesh in enumerate(t.build_meshes(COORDS)):
        scene.add_chunk().terrain_batch3d(mesh.source(B.PixelSource.Pixel((40 + 50 * k, 200 - 40 * k, 90, 255))))
    scene.add_d3_static(api.Batch3D.from_box(14.0, 1.0, 14.0, 3.0, 3.0, 3.0).with_computed_normals().source(B.PixelSource.Pixel((250, 240, 60, 255))))
    scene.lights([B.Light(B.LIGHT_POINT).with_position((16.0, 9.0, 16.0)).with_color((1.0, 0.95, 0.8)).with_intensity(3.0).with_start_distance(2.0)
                  .with_end_distance(60.0).compile()])
    cam = api.D3OrbitCamera.new()
    cam.set_parameter_f32("distance", 30.0)
    cam.center = (16.0, 0.0, 16.0)
    cam.azimuth, cam.elevation = 0.9, 0.8
    assets = api.Assets.default()

    def render():
        v, p = cam.matrices(float(W), float(H))
        out = np.zeros(W * H * 4, np.uint8)
        api.Rasterizer.setup(None, v, p).ambient((0.5, 0.5, 0.5, 1.0)).rasterize(scene, out, W, H, 32, assets)
        return out.reshape(H, W, 4)

    return t, scene, render


@pytest.fixture()
def devproj(product):
    product.lib.rxh_set_device_projection(1)
    yield product
    product.lib.rxh_set_device_projection(0)


def test_a_height_stroke_through_the_mirror_takes_the_fast_path(devproj):
    api = devproj
    base = {(x, y): height(x, y) for y in range(CELLS) for x in range(CELLS) if (x, y) != (20, 5)}      # (one cell of chunk (1, 0) is absent)
    stroke = {(x, y): base[(x, y)] + 2.5 for y in range(3, 9) for x in range(18, 26) if (x, y) in base}   # chunk (1, 0) only
    added = dict(stroke)
    added[(20, 5)] = 3.0                                                                                    # ... and a cell that did not exist

    def old_route(edits):
        t, scene, render = terrain_scene(api, base)
        first = render()
        for (x, y), h in edits.items():
            t.set_height(x, y, h)
        # Terrain.build_meshes, the batch replaced, rasterize (the scene is registered again)
        t2, scene2, render2 = terrain_scene(api, {**base, **edits})
        return first, render2()

    for edits, want_rc in ((stroke, 0), (added, 1)):
        first, want = old_route(edits)
        t, scene, render = terrain_scene(api, base)
        assert render().tobytes() == first.tobytes()
        for (x, y), h in edits.items():
            t.set_height(x, y, h)
        rxr = rusterix_amd.rxr_abi()
        lo0, hi0 = (C.c_float * 3)(), (C.c_float * 3)()
        assert rxr.rxr_mesh_bounds(api.lib.rxh_context(), 1, lo0, hi0) == RXR_OK
        assert scene.rebuild_terrain_meshes(t, [(1, 0)], [1]) == want_rc
        got = render()
        assert got.tobytes() == want.tobytes(), (want_rc, int((got != want).any(axis=2).sum()))
        assert got.tobytes() != first.tobytes(), "the stroke should show"
        lo, hi = (C.c_float * 3)(), (C.c_float * 3)()
        assert rxr.rxr_mesh_bounds(api.lib.rxh_context(), 1, lo, hi) == RXR_OK and hi[1] > hi0[1] + 0.5
        if want_rc == 0:
            # a pick straight down onto the raised cells hits the new surface, in chunk 1's terrain batch (mesh 1)
            hit = scene.intersect([[21.5, 50.0, 6.5]], [[0.0, -1.0, 0.0]])
            assert hit["mesh"][0] == 1
            y = hit["hitpoint"][0][1]
            assert abs(y - (height(21, 6) + 2.5)) < 1.5 and y > height(21, 6) + 1.0, y


def test_the_mirror_refuses_without_device_projection_and_falls_back_without_a_registration(product):
    base = {(x, y): height(x, y) for y in range(CELLS) for x in range(CELLS)}
    t, scene, render = terrain_scene(product, base)
    with pytest.raises(B.RasterizeError) as e:
        scene.rebuild_terrain_meshes(t, [(1, 0)], [1])
    assert e.value.code == RXR_ERR_UNSUPPORTED
    product.lib.rxh_set_device_projection(1)
    try:
        # no frame of this scene has been uploaded: the context holds other geometry, the next upload registers from the host arrays
        t.set_height(20, 5, 4.0)
        assert scene.rebuild_terrain_meshes(t, [(1, 0)], [1]) == 1
        _, _, want = terrain_scene(product, {**base, (20, 5): 4.0})
        assert render().tobytes() == want().tobytes()
        with pytest.raises(B.RasterizeError):
            scene.rebuild_terrain_meshes(t, [(1, 0)], [7])
    finally:
        product.lib.rxh_set_device_projection(0)
