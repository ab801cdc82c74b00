"""Vertex normals on the device (rxr_vertex_normals / rxr_vertex_normals_to, include/rxr.h; rusterix_amd/csrc/rxr_normals.hip) against
the oracle's Batch3D::compute_vertex_normals over exactly the arrays given (tests/vertex_normals_ref.py): every comparison is on the
uint32 view, no tolerance; a NaN of the reference is answered by a NaN.  The normals are filled with a sentinel before every call:
every slot past a mesh's vertex count must still hold it.

Both routes are pinned through RXR_VERTEX_NORMALS_SMALL_MAX (a huge value: one workgroup per mesh; 0: the sorted gather), and every
call asserts through rxr_debug_vertex_normals that the route it meant to test is the one that ran.  Shapes are the smallest at which
each mechanism can go wrong."""
import ctypes as C

import numpy as np
import pytest

from rusterix_amd import binding as B
from rusterix_amd.abi import RXR_ERR_INVALID, RXR_ERR_UNSUPPORTED, RXR_OK
from tests import vertex_normals_ref as R
from tests.test_gpu_mesh_update import Ctx, camera
from tests.vertex_normals_ref import F, SENTINEL

pytestmark = pytest.mark.gpu

SMALL, GENERAL = 1, 2                    # RXR_VERTEX_NORMALS_ROUTE_*
ROUTES = ["small", "general"]
ORDER_SEEDS = (11, 12, 13, 14)           # tests/test_vertex_normals_cpu.py checks the conditions for the same seeds


def pin(monkeypatch, route):
    """sends the following calls through `route`; returns the RXR_VERTEX_NORMALS_ROUTE_* the debug counter must then report"""
    if route == "default":
        monkeypatch.delenv("RXR_VERTEX_NORMALS_SMALL_MAX", raising=False)
        return None
    monkeypatch.setenv("RXR_VERTEX_NORMALS_SMALL_MAX", "4000000000" if route == "small" else "0")
    return SMALL if route == "small" else GENERAL


class NCtx(Ctx):
    def route(self):
        launches = C.c_uint32(0xDEAD)
        return self.rxr.rxr_debug_vertex_normals(self.ctx, C.byref(launches)), launches.value

    def host(self, counts, vertices, indices, normals):
        n, vs, ts = len(counts), vertices.shape[1], indices.shape[1]
        return self.rxr.rxr_vertex_normals(self.ctx, n, counts.ctypes.data, vertices.ctypes.data, indices.ctypes.data, normals.ctypes.data, vs, ts)

    def normals(self, meshes, want_route, vstride=None, tstride=None):
        """rxr_vertex_normals over `meshes`; the whole normals array [n][VS][3], after asserting the route"""
        counts, v, i, nr = R.pack(meshes, vstride, tstride)
        rc = self.host(counts, v, i, nr)
        assert rc == RXR_OK, self.error()
        if want_route is not None:
            assert self.route()[0] == want_route, self.route()
        return nr

    def to(self, counts, v, i, nr, stream=None, with_refused=True):
        """rxr_vertex_normals_to over torch tensors written on `stream` just before the call; (rc, the tensors)"""
        import torch

        s = stream or torch.cuda.Stream()
        with torch.cuda.stream(s):
            dev = [torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to("cuda").clone() for a in (counts, v, i, nr)]
            refused = torch.full((len(counts),), 0x5A5A5A5A, dtype=torch.int32, device="cuda") if with_refused else None
        rc = self.rxr.rxr_vertex_normals_to(self.ctx, len(counts), *(d.data_ptr() or None for d in dev), refused.data_ptr() if with_refused else None,
                                            v.shape[1], i.shape[1], s.cuda_stream)
        return rc, dev, refused, s


@pytest.fixture(scope="module")
def ctx():
    c = NCtx()
    yield c
    c.close()


def check(ctx, oracle, meshes, want_route, vstride=None, tstride=None, label=""):
    got = ctx.normals(meshes, want_route, vstride, tstride)
    want = R.expected(oracle, meshes, got.shape[1])
    assert R.same_bits(got, want), (label, R.differing_vertices(got.reshape(-1, 3), want.reshape(-1, 3)))
    return got


# ---- 1. the smallest meshes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ROUTES)
def test_one_triangle_two_triangles_and_a_box(ctx, oracle, monkeypatch, route):
    want = pin(monkeypatch, route)
    one = (np.array([[0, 0, 0, 1], [1, 0.5, 0, 1], [0.25, 1, 2, 1]], F), np.array([[0, 1, 2]], np.uint32))
    two = (np.array([[0, 0, 0, 1], [1, 0.5, 0, 1], [0.25, 1, 2, 1], [1.5, 1.25, -1, 1]], F), np.array([[0, 1, 2], [2, 1, 3]], np.uint32))
    bv, bi, _, _ = oracle.Batch3D.from_box(-1.0, 0.5, 2.0, 2.0, 1.0, 3.0).geometry()
    assert bv.shape == (24, 4) and bi.shape == (12, 3)
    for label, mesh in (("one", one), ("two", two), ("box", (bv, bi))):
        got = check(ctx, oracle, [mesh], want, label=label)
        assert np.isfinite(got).all() and np.allclose(np.linalg.norm(got[0], axis=1), 1.0, atol=1e-6)
        assert ctx.route()[1] == 1


# ---- 2. the order of the additions ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("seed", ORDER_SEEDS)
def test_sums_run_in_ascending_triangle_index(ctx, oracle, monkeypatch, route, seed):
    want = pin(monkeypatch, route)
    v, i = R.generated(seed, 40, 120)
    forward, backward = R.transcribed_normals(v, i), R.transcribed_normals(v, i, reverse=True)
    # conditions, not measurements: the reversed order must show in at least a quarter of the vertices, at most a quarter may be NaN
    assert R.differing_vertices(forward, backward) >= 10 and int(np.isnan(forward).any(axis=1).sum()) <= 10
    got = check(ctx, oracle, [(v, i)], want, label=seed)
    assert R.same_bits(got[0], forward) and not R.same_bits(got[0], backward)


# ---- 3. the sign of zero -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ROUTES)
def test_a_lone_negative_zero_becomes_positive(ctx, oracle, monkeypatch, route):
    want = pin(monkeypatch, route)
    v, i = R.negative_zero_triangle()
    assert np.signbit(R.face_normals(v, i)[0, 0])
    got = check(ctx, oracle, [(v, i)], want)
    assert (got[0].view(np.uint32) == np.array([0, 0x3F800000, 0], np.uint32)).all(), got[0].view(np.uint32)


# ---- 4. unused and repeated vertices, degenerate triangles, values that are not finite ---------------------------------------------------
@pytest.mark.parametrize("route", ROUTES)
def test_unused_repeated_degenerate_and_not_finite(ctx, oracle, monkeypatch, route):
    want = pin(monkeypatch, route)
    v, i = R.generated(41, 20, 30)
    i[i >= 17] = 3                                              # vertices 17, 18, 19 are used by no triangle
    i[5] = (4, 4, 9)                                            # (a, a, b): added twice to a, a NaN in a and b
    v[10, :3], v[11, :3], v[12, :3] = (1, 1, 1), (2, 2, 2), (3, 3, 3)
    i[6] = (10, 11, 12)                                         # three collinear points
    unused = check(ctx, oracle, [(v, i)], want, label="unused")
    assert (unused[0, 17:].view(np.uint32) == 0).all(), "unused vertices are exact +0.0 triples"
    ref = R.oracle_normals(oracle, v, i)
    poisoned = np.isnan(ref).any(axis=1)
    assert poisoned[[4, 9, 10, 11, 12]].all() and not poisoned.all()
    assert (np.isnan(unused[0]).any(axis=1) == poisoned).all(), "NaNs in exactly the vertices the oracle poisons"
    v2, i2 = R.generated(42, 20, 30)
    v2[3, 1], v2[8, 0] = np.nan, np.inf
    check(ctx, oracle, [(v2, i2)], want, label="nan and inf")


# ---- 5. valence at the machine's edges ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("valence", [63, 64, 65, 255, 256, 257, 1025])
def test_a_fan_apex(ctx, oracle, monkeypatch, route, valence):
    want = pin(monkeypatch, route)
    v, i = R.fan(valence)
    got = check(ctx, oracle, [(v, i)], want, label=valence)
    assert np.isfinite(got[0, 0]).all()


# ---- 6. the route bound --------------------------------------------------------------------------------------------------------------------
_BOUND_MESHES = {}


def bound_mesh(oracle, nt):
    if nt not in _BOUND_MESHES:
        v, i = R.generated(60, 300, nt)
        _BOUND_MESHES[nt] = ((v, i), R.oracle_normals(oracle, v, i))
    return _BOUND_MESHES[nt]


def constants(ctx):
    out = (C.c_uint32 * 3)()
    ctx.rxr.rxr_debug_vertex_normals_constants(out)
    return out[0], out[1], out[2]


@pytest.mark.parametrize("override", ["default", "general", "small"])
@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_meshes_around_the_small_routes_bound(ctx, oracle, monkeypatch, override, delta):
    bound, cap, _ = constants(ctx)
    assert 0 < bound < cap and cap * 24 + 16 <= 160 * 1024
    nt = bound + delta
    pin(monkeypatch, override)
    want_route = {"default": SMALL if nt <= bound else GENERAL, "general": GENERAL, "small": SMALL}[override]
    mesh, want = bound_mesh(oracle, nt)
    got = ctx.normals([mesh], want_route)
    assert R.same_bits(got[0], want), R.differing_vertices(got[0], want)


def test_an_override_is_cut_to_what_a_workgroup_holds(ctx, oracle, monkeypatch):
    _, cap, _ = constants(ctx)
    pin(monkeypatch, "small")
    mesh, want = bound_mesh(oracle, cap)
    assert R.same_bits(ctx.normals([mesh], SMALL)[0], want)
    mesh, want = bound_mesh(oracle, cap + 1)
    assert R.same_bits(ctx.normals([mesh], GENERAL)[0], want)


# ---- 7. several meshes in one call ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ROUTES)
def test_counts_of_zero_one_and_the_stride_across_a_launch_cut(ctx, oracle, monkeypatch, route):
    want = pin(monkeypatch, route)
    VS, TS = 23, 31
    empty = (np.zeros((0, 4), F), np.zeros((0, 3), np.uint32))
    meshes = [R.generated(70, VS, TS), empty, R.generated(71, 3, 1), R.generated(72, VS, 1), R.generated(73, 5, TS), empty,
              (R.generated(74, 1, 0)[0], np.zeros((0, 3), np.uint32)), R.generated(75, VS, TS), R.generated(76, 11, 7)]
    monkeypatch.setenv("RXR_VERTEX_NORMALS_LAUNCH_SLOTS", str(4 * TS))       # four meshes a launch: 9 meshes = 3 launches
    got = check(ctx, oracle, meshes, want, vstride=VS, tstride=TS)
    assert ctx.route()[1] == 3
    assert (got[1] == SENTINEL).all() and (got[2, 3:] == SENTINEL).all() and (got[6, 0].view(np.uint32) == 0).all()
    monkeypatch.delenv("RXR_VERTEX_NORMALS_LAUNCH_SLOTS")
    # strides larger than any count, in one launch
    got = check(ctx, oracle, meshes, want, vstride=VS + 9, tstride=TS + 5)
    assert ctx.route()[1] == 1 and (got[:, VS:] == SENTINEL).all()
    # nothing at all
    assert ctx.rxr.rxr_vertex_normals(ctx.ctx, 0, None, None, None, None, 5, 5) == RXR_OK


# ---- 8. against an independent kernel -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ROUTES)
def test_the_terrain_mesh_kernels_own_normals(ctx, monkeypatch, route):
    from tests.terrain_hit_ref import HeightSpec

    want = pin(monkeypatch, route)
    cs = 16
    spec = HeightSpec((1.0, 0.75), cs)
    rng = np.random.default_rng(8)
    for y in range(-2, cs + 2):
        for x in range(-2, cs + 2):
            if (x, y) not in ((3, 3), (4, 3), (9, 12), (0, 0), (15, 15), (7, 8)):       # holes
                spec.height(x, y, float(rng.random() * 3 - 1))
    keep, args = spec.arrays()
    assert ctx.rxr.rxr_set_terrain_heights(ctx.ctx, *args) == RXR_OK, ctx.error()
    vs, ts = (cs + 1) ** 2, 2 * cs * cs
    counts, v, i = np.zeros((1, 2), np.uint32), np.full((1, vs, 4), 1e30, F), np.zeros((1, ts, 3), np.uint32)
    theirs = np.full((1, vs, 3), SENTINEL, F)
    cc = np.zeros((1, 2), np.int32)
    assert ctx.rxr.rxr_terrain_meshes(ctx.ctx, cc.ctypes.data, 1, cs, counts.ctypes.data, v.ctypes.data, i.ctypes.data, theirs.ctypes.data) == RXR_OK, ctx.error()
    assert 200 < counts[0, 0] < vs and 400 < counts[0, 1] < ts
    mine = np.full((1, vs, 3), SENTINEL, F)
    assert ctx.host(counts, v, i, mine) == RXR_OK, ctx.error()
    assert ctx.route()[0] == want
    assert (mine.view(np.uint32) == theirs.view(np.uint32)).all(), R.differing_vertices(mine[0], theirs[0])


# ---- 9. the teapot ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ROUTES)
def test_the_teapot(ctx, oracle, monkeypatch, route):
    import os

    want = pin(monkeypatch, route)
    d = np.load(os.path.join(os.path.dirname(__file__), "golden", "teapot_mesh.npz"))
    v = np.ones((len(d["positions"]), 4), F)
    v[:, :3] = d["positions"]
    check(ctx, oracle, [(v, d["indices"].astype(np.uint32))], want)


# ---- 10. the device form, chained into rxr_update_meshes_to ---------------------------------------------------------------------------------
def lit_mesh(seed, oracle):
    v, i = R.generated(seed, 30, 40)
    v[:, :3] = v[:, :3] * F(0.3) + np.array([0, 0, -6], F)
    return dict(vertices=v, indices=i, uvs=np.zeros((30, 2), F), normals=R.oracle_normals(oracle, v, i), list=3)


@pytest.mark.parametrize("route", ROUTES)
def test_device_form_on_a_side_stream_feeds_update_meshes_to(ctx, oracle, product, monkeypatch, route):
    import torch

    want = pin(monkeypatch, route)
    cam = camera(product)
    new = [lit_mesh(90, oracle), lit_mesh(91, oracle)]
    other = NCtx()
    try:
        other.set_meshes(new)                                   # registered from the host with the oracle's normals
        reference = other.frame(cam)
    finally:
        other.close()
    old = [dict(m, vertices=m["vertices"] + F(0.125), normals=np.zeros_like(m["normals"])) for m in new]
    ctx.set_meshes(old)
    assert ctx.frame(cam).tobytes() != reference.tobytes()
    counts, v, i, nr = R.pack([(m["vertices"], m["indices"]) for m in new], vstride=37, tstride=45)
    rc, dev, refused, s = ctx.to(counts, v, i, nr)
    assert rc == RXR_OK, ctx.error()
    assert ctx.route()[0] == want
    named = np.arange(2, dtype=np.uint32)
    rc = ctx.rxr.rxr_update_meshes_to(ctx.ctx, named.ctypes.data, 2, *(d.data_ptr() for d in dev), 37, 45, s.cuda_stream)
    assert rc == RXR_OK, ctx.error()
    torch.cuda.synchronize()
    assert (refused.cpu().numpy() == 0).all()
    ctx.meshes = list(new)
    assert ctx.frame(cam).tobytes() == reference.tobytes()
    assert len(np.unique(reference.reshape(-1, 4), axis=0)) > 20, "the meshes should show, lit"
    got = dev[3].cpu().numpy()
    assert R.same_bits(got, R.expected(oracle, [(m["vertices"], m["indices"]) for m in new], 37))


# ---- 11. refusals ------------------------------------------------------------------------------------------------------------------------------
def refusal_inputs():
    """four meshes at strides 12 / 16: clean, one triangle with an index == its vertex count (below the stride), clean, clean"""
    meshes = [R.generated(100, 12, 16), R.generated(101, 9, 14), R.generated(102, 10, 16), R.generated(103, 7, 5)]
    counts, v, i, nr = R.pack(meshes, vstride=12, tstride=16)
    return meshes, counts, v, i, nr


@pytest.mark.parametrize("route", ROUTES)
def test_the_host_form_refuses_and_writes_nothing(ctx, monkeypatch, route):
    pin(monkeypatch, route)
    meshes, counts, v, i, nr = refusal_inputs()
    bad = i.copy()
    bad[1, 6, 2] = 9
    assert ctx.host(counts, v, bad, nr) == RXR_ERR_INVALID
    assert "mesh 1: triangle 6 has a vertex index 9 that is not below its 9 vertices" in ctx.error(), ctx.error()
    c = counts.copy()
    c[2, 0] = 13
    assert ctx.host(c, v, i, nr) == RXR_ERR_INVALID and "mesh 2: its 13 vertices exceed vertex_stride 12" in ctx.error(), ctx.error()
    c = counts.copy()
    c[3, 1] = 17
    assert ctx.host(c, v, i, nr) == RXR_ERR_INVALID and "mesh 3: its 17 triangles exceed triangle_stride 16" in ctx.error(), ctx.error()
    assert ctx.rxr.rxr_vertex_normals(ctx.ctx, 4, counts.ctypes.data, None, i.ctypes.data, nr.ctypes.data, 12, 16) == RXR_ERR_INVALID and "NULL" in ctx.error()
    assert ctx.rxr.rxr_vertex_normals(ctx.ctx, 1 << 31, counts.ctypes.data, v.ctypes.data, i.ctypes.data, nr.ctypes.data, 0xFFFFFFFF, 0xFFFFFFFF) == RXR_ERR_INVALID
    assert "overflow" in ctx.error()
    assert (nr == SENTINEL).all(), "nothing is written by a refused call"
    assert ctx.host(counts, v, i, nr) == RXR_OK, ctx.error()


@pytest.mark.parametrize("route", ROUTES)
def test_the_device_form_skips_what_it_cannot_refuse(ctx, oracle, monkeypatch, route):
    import torch

    want = pin(monkeypatch, route)
    meshes, counts, v, i, nr = refusal_inputs()
    i[1, 6, 2] = 9                                            # == mesh 1's vertex count; below the stride: memory the test owns
    i[1, 13] = (11, 0, 1)                                     # ... and a second one
    counts[2, 0] = 13                                         # above the stride: the whole mesh is skipped
    rc, dev, refused, s = ctx.to(counts, v, i, nr)
    assert rc == RXR_OK, ctx.error()
    assert ctx.route()[0] == want
    torch.cuda.synchronize()
    assert refused.cpu().numpy().view(np.uint32).tolist() == [0, 2, 0xFFFFFFFF, 0]
    got = dev[3].cpu().numpy()
    clean = [meshes[0], (meshes[1][0], np.delete(meshes[1][1], [6, 13], axis=0)), (np.zeros((0, 4), F), np.zeros((0, 3), np.uint32)), meshes[3]]
    assert R.same_bits(got, R.expected(oracle, clean, 12)), "refused triangles contribute nothing; the skipped mesh is not written"
    # without dev_refused, and a later call on the context still works
    rc, dev, _, _ = ctx.to(counts, v, i, nr, with_refused=False)
    assert rc == RXR_OK, ctx.error()
    torch.cuda.synchronize()
    assert R.same_bits(dev[3].cpu().numpy(), R.expected(oracle, clean, 12))
    check(ctx, oracle, meshes, want)


def test_the_device_forms_pointer_checks_and_multi_device_handles(ctx):
    import torch

    meshes, counts, v, i, nr = refusal_inputs()
    dev = [torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda() for a in (counts, v, i, nr)]
    torch.cuda.synchronize()
    p = [d.data_ptr() for d in dev]
    call = lambda *a: ctx.rxr.rxr_vertex_normals_to(ctx.ctx, 4, *a, 12, 16, None)
    assert call(p[0], v.ctypes.data, p[2], p[3], None) == RXR_ERR_INVALID and "dev_vertices is not device memory" in ctx.error()
    assert call(p[0], p[1], p[2] + 1, p[3], None) == RXR_ERR_INVALID and "dev_indices must be 4-byte aligned" in ctx.error()
    assert call(p[0], p[1], p[2], None, None) == RXR_ERR_INVALID and "dev_normals must be 4-byte aligned" in ctx.error()
    assert call(p[0], p[1], p[2], p[3], nr.ctypes.data) == RXR_ERR_INVALID and "dev_refused is not device memory" in ctx.error()
    assert ctx.rxr.rxr_vertex_normals_to(ctx.ctx, 0, None, None, None, None, None, 12, 16, None) == RXR_OK
    g = NCtx()
    g.close()                                                 # (a handle of rxr_create_multi in the plain one's place)
    devs = (C.c_int * 1)(0)
    assert g.rxr.rxr_create_multi(C.byref(g.ctx), devs, 1) == RXR_OK
    try:
        assert g.rxr.rxr_vertex_normals_to(g.ctx, 4, *p, None, 12, 16, None) == RXR_ERR_UNSUPPORTED and "multi-device" in g.error()
        assert g.host(counts, v, i, nr) == RXR_OK, g.error()
        assert g.route()[0] == SMALL
    finally:
        g.close()


# ---- 12. the mirror and the binding ----------------------------------------------------------------------------------------------------------
W, H = 160, 96


def box_scene(api, device):
    scene = api.Scene.empty()
    for k in range(4):
        b = api.Batch3D.from_box(-3.0 + 1.6 * k, -0.5, -6.0 - 0.3 * k, 1.0, 1.0 + 0.2 * k, 1.0).source(B.PixelSource.Pixel((60 + 40 * k, 220 - 30 * k, 120, 255)))
        scene.add_d3_dynamic(b)
    v, i = R.generated(120, 30, 40)
    v[:, :3] = v[:, :3] * F(0.25) + np.array([0, 1.5, -6], F)
    scene.add_d3_dynamic(api.Batch3D.new(v, i, np.zeros((30, 2), F)).source(B.PixelSource.Pixel((240, 200, 80, 255))))
    scene.compute_dynamic_normals(device=device)
    scene.lights([B.Light(B.LIGHT_POINT).with_position((1.0, 3.0, -3.0)).with_color((1.0, 0.95, 0.8)).with_intensity(3.0).with_start_distance(2.0)
                  .with_end_distance(40.0).compile()])
    cam = api.D3FirstPCamera.new()
    cam.position, cam.center = (0.0, 0.5, 0.0), (0.0, 0.0, -6.0)
    v_, p_ = cam.matrices(float(W), float(H))
    out = np.zeros(W * H * 4, np.uint8)
    api.Rasterizer.setup(None, v_, p_).ambient((0.3, 0.3, 0.3, 1.0)).rasterize(scene, out, W, H, 32, api.Assets.default())
    return [scene.batch3d_normals(B.LIST_DYNAMIC, k) for k in range(5)], out.reshape(H, W, 4)


def test_the_mirrors_device_normals_and_a_lit_frame(product, oracle):
    cpu_normals, cpu_frame = box_scene(product, False)
    dev_normals, dev_frame = box_scene(product, True)
    for k, (a, b) in enumerate(zip(cpu_normals, dev_normals)):
        assert len(a) == (24 if k < 4 else 30) and R.same_bits(b, a), k
    assert dev_frame.tobytes() == cpu_frame.tobytes()
    assert len(np.unique(cpu_frame.reshape(-1, 4), axis=0)) > 20, "the boxes should show, lit"
    # the raw pair of the binding, on the process-wide context
    v, i = R.generated(121, 12, 20)
    counts, vv, ii, nr = R.pack([(v, i)])
    got = product.vertex_normals(counts, vv, ii, nr)
    assert got is nr and R.same_bits(got[0], R.oracle_normals(oracle, v, i))
