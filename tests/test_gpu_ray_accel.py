"""The ray box tree on the device (rxr_set_ray_accel / rxr_ray_accel_info, rusterix_amd/csrc/rxr_ray_accel.hip): with the mode on,
every output word of the many-ray picking path and every float of the path tracer's accumulation buffer is what the brute-force
kernels write on the same context -- and, for the small scenes, what tests/intersect_ref.py computes.  Tree shapes at every size
where a level fills, leaves across meshes and segments, ties, wild triangles, rays that hit nothing by construction, seeded scenes,
rebuilds, and the count that proves triangles were skipped."""
import ctypes as C

import numpy as np
import pytest

from rusterix_amd import trace as T
from rusterix_amd.abi import RXR_ERR_INVALID, RXR_OK
from tests import intersect_ref as R
from tests import mesh_update_ref as M
from tests import pick_fuzz as P
from tests import ray_accel_ref as A
from tests import trace_scenes as S

pytestmark = pytest.mark.gpu
F = np.float32
OFF, ON, COUNT = T.RAY_ACCEL_OFF, T.RAY_ACCEL_ON, T.RAY_ACCEL_COUNT
L, W = A.LEAF, A.WIDTH
COUNTS = (1, L - 1, L, L + 1, L * W - 1, L * W, L * W + 1, L * W * W + 1)


@pytest.fixture(scope="module")
def pick():
    with P.PickContext() as ctx:
        yield ctx


@pytest.fixture(scope="module")
def tracer():
    with T.Tracer() as tr:
        yield tr


def set_mode(ctx, mode):
    return ctx.rxr.rxr_set_ray_accel(ctx.ctx, mode)


def info(ctx):
    out = (C.c_uint64 * len(T.RAY_ACCEL_INFO))()
    assert ctx.rxr.rxr_ray_accel_info(ctx.ctx, out) == RXR_OK, ctx.error()
    return dict(zip(T.RAY_ACCEL_INFO, (int(x) for x in out)))


def on_and_off(ctx, o, d, label, full=True, ref=None, mode=ON):
    """mode off, then on, on the same context: every output word equal (and equal to `ref`); returns the result"""
    assert set_mode(ctx, OFF) == RXR_OK
    off = ctx.intersect(o, d, full=full)
    assert set_mode(ctx, mode) == RXR_OK
    before = info(ctx)["batches"]
    on = ctx.intersect(o, d, full=full)
    after = info(ctx)
    assert set_mode(ctx, OFF) == RXR_OK
    bad = P.differences(on, off, f"{label}: tree against brute force,")
    assert bad is None, bad
    if ref is not None:
        bad = P.differences(off, ref if full else P.plain_of(ref), f"{label}: against the restatement,")
        assert bad is None, bad
    assert after["batches"] == before + (1 if len(o) > 64 and after["triangles"] else 0), (label, before, after)
    return on


def aimed(meshes, eye, rng, n):
    """n rays from `eye`: two thirds at vertices, edge points and inner points of random triangles, the rest anywhere"""
    live = [m for m in meshes if len(m["indices"])]
    o = np.tile(np.asarray(eye, F), (n, 1))
    d = rng.standard_normal((n, 3)).astype(F)
    for r in range(0, n, 3):
        for rr in (r, r + 1):
            if rr >= n:
                break
            m = live[int(rng.integers(len(live)))]
            v = m["vertices"][m["indices"][int(rng.integers(len(m["indices"])))].astype(np.int64), :3]
            kind = int(rng.integers(3))
            target = v[0] if kind == 0 else v[0] + (v[1] - v[0]) * F(rng.random()) if kind == 1 else (v[0] + v[1] + v[2]) / F(3.0)
            d[rr] = target - o[rr]
    return o, d


def grid(n, seed, **kw):
    rng = np.random.default_rng(seed)
    v3, idx = P._grid(rng, n)
    v = np.concatenate([v3, np.ones((len(v3), 1), F)], axis=1)
    return P.mesh(v, idx, rng.uniform(-2, 3, (len(v), 2)), rng.standard_normal((len(v), 3)), **kw)


@pytest.mark.parametrize("ntri", COUNTS)
def test_tree_sizes_where_a_level_fills(pick, ntri):
    meshes = [grid(ntri, 100 + ntri)]
    pick.set_meshes(meshes)
    rng = np.random.default_rng(ntri)
    o, d = aimed(meshes, (0.5, 7.0, 3.0), rng, 300)
    ref = R.intersect_many(meshes, o, d, full=True)
    on_and_off(pick, o, d, f"{ntri} triangles", ref=ref)
    assert set_mode(pick, ON) == RXR_OK
    pick.intersect(o, d)
    i = info(pick)
    cnt = A.levels(ntri)
    assert (i["valid"], i["triangles"], i["nodes"], i["levels"], i["wild"]) == (1, ntri, sum(cnt), len(cnt), 0), i
    assert (ref["mesh"] != R.MISS).sum() > 50
    set_mode(pick, OFF)


def test_a_leaf_across_two_meshes_and_two_segments(pick):
    """5 static triangles and 7 overlay ones: the first leaf holds both meshes, and both segments"""
    meshes = [grid(5, 1), grid(7, 2, list=R.LIST_OVERLAY), grid(L + 3, 3, list=R.LIST_OVERLAY), grid(2, 4, list=R.LIST_OVERLAY)]
    pick.set_meshes(meshes)
    o, d = aimed(meshes, (0.2, 6.0, 4.0), np.random.default_rng(5), 400)
    ref = R.intersect_many(meshes, o, d, full=True)
    on_and_off(pick, o, d, "a leaf across meshes", ref=ref)
    assert len(np.unique(ref["mesh"])) >= 4


def test_several_segments_in_one_scene(pick):
    """a plain run, chunk meshes with equal and with different profile ids, overlay meshes, a mesh without triangles between them"""
    meshes = [grid(30, 1, list=R.LIST_CHUNK_OPACITY, chunk=0), grid(70, 2, list=R.LIST_CHUNK, chunk=0), grid(9, 3, list=R.LIST_CHUNK, chunk=0, pid=4),
              grid(64, 4, list=R.LIST_CHUNK, chunk=0, pid=4), grid(65, 5, list=R.LIST_CHUNK, chunk=0, pid=5), grid(0, 6, list=R.LIST_CHUNK, chunk=0, pid=5),
              grid(33, 7, list=R.LIST_CHUNK_TERRAIN, chunk=0), grid(200, 8), grid(17, 9, list=R.LIST_DYNAMIC), grid(40, 10, list=R.LIST_OVERLAY),
              grid(3, 11, list=R.LIST_OVERLAY)]
    assert len(P.segments(meshes)) >= 6
    pick.set_meshes(meshes)
    o, d = aimed(meshes, (0.4, 8.0, 2.0), np.random.default_rng(6), 1500)
    ref = R.intersect_many(meshes, o, d, full=True)
    on_and_off(pick, o, d, "several segments", ref=ref)
    on_and_off(pick, o, d, "several segments, plain", full=False, ref=ref)
    assert len(np.unique(ref["mesh"])) >= 8


def test_64_rays_stay_on_the_few_ray_path_and_65_take_the_tree(pick):
    meshes = [grid(500, 12), grid(40, 13, list=R.LIST_OVERLAY)]
    pick.set_meshes(meshes)
    o, d = aimed(meshes, (0.1, 5.0, 5.0), np.random.default_rng(7), 65)
    ref = R.intersect_many(meshes, o, d, full=True)
    for n in (64, 65):
        on_and_off(pick, o[:n], d[:n], f"{n} rays", ref=P.prefix(ref, n))     # (asserts the batch count: + 0 and + 1)


def test_identical_triangles_the_earliest_wins(pick):
    """equal codes, equal t: 150 copies of one triangle in a mesh, and the same again in a second mesh and in an overlay"""
    v = np.array([(0, 0, 0, 1), (2, 0, 0, 1), (0, 2, 0, 1)], F)
    idx = np.tile(np.array([(0, 1, 2)], np.uint32), (150, 1))
    meshes = [P.mesh(v, idx), P.mesh(v, idx, list=R.LIST_DYNAMIC), P.mesh(v, idx[:9], list=R.LIST_OVERLAY)]
    rng = np.random.default_rng(8)
    o, d = aimed(meshes, (0.5, 0.5, -5.0), rng, 200)
    ref = R.intersect_many(meshes, o, d, full=True)
    pick.set_meshes(meshes[:2])
    got = on_and_off(pick, o, d, "identical triangles", ref=R.intersect_many(meshes[:2], o, d, full=True))
    hit = got["mesh"] != R.MISS
    assert hit.sum() > 100 and (got["mesh"][hit] == 0).all() and (got["triangle"][hit] == 0).all()
    pick.set_meshes(meshes)
    got = on_and_off(pick, o, d, "identical triangles under an overlay", ref=ref)
    assert (got["mesh"][hit] == 2).all() and (got["triangle"][hit] == 0).all()


def test_two_meshes_hit_at_equal_t(pick):
    a, b = grid(300, 21), grid(300, 21, list=R.LIST_DYNAMIC)     # the same geometry twice: every hit ties
    c = grid(300, 21, list=R.LIST_CHUNK, chunk=0, pid=1)
    meshes = [c, a, b]
    pick.set_meshes(meshes)
    o, d = aimed(meshes, (0.3, 6.0, 3.0), np.random.default_rng(9), 600)
    ref = R.intersect_many(meshes, o, d, full=True)
    got = on_and_off(pick, o, d, "equal t across meshes", ref=ref)
    hit = got["mesh"] != R.MISS
    assert hit.sum() > 200 and (got["mesh"][hit] == 0).all()


def test_slivers_and_axis_aligned_quads_from_far_origins(pick):
    """the CPU generator's rays: through vertices and edge points, grazing, from 1e-2 .. 1e5 away; plus every ray against every
    other triangle"""
    rng = np.random.default_rng(10)
    sl = A.triangles(rng, 400, "sliver")
    slivers = np.concatenate([np.stack(sl, axis=1).reshape(-1, 3), np.ones((1200, 1), F)], axis=1)
    n = 20
    xs, zs = np.meshgrid(np.arange(n + 1, dtype=F), np.arange(n + 1, dtype=F))
    qv = np.stack([xs.ravel(), np.zeros(xs.size, F), zs.ravel(), np.ones(xs.size, F)], axis=1)
    i0 = (np.arange(n)[:, None] * (n + 1) + np.arange(n)[None, :]).ravel()
    qi = np.stack([np.stack([i0, i0 + 1, i0 + n + 2], 1), np.stack([i0, i0 + n + 2, i0 + n + 1], 1)], 1).reshape(-1, 3)
    meshes = [P.mesh(slivers, np.arange(1200, dtype=np.uint32).reshape(-1, 3)), P.mesh(qv, qi, list=R.LIST_DYNAMIC)]
    pick.set_meshes(meshes)
    q = qv[qi.astype(np.int64), :3]
    o1, d1 = A.aimed_rays(rng, *sl)
    o2, d2 = A.aimed_rays(rng, q[:, 0], q[:, 1], q[:, 2])
    o, d = np.concatenate([o1, o2]), np.concatenate([d1, d2])
    ref = R.intersect_many(meshes, o, d, full=True)
    on_and_off(pick, o, d, "slivers and quads", ref=ref)
    assert (ref["mesh"] == 0).sum() > 50 and (ref["mesh"] == 1).sum() > 200
    assert set_mode(pick, ON) == RXR_OK
    pick.intersect(o, d)
    p0, e1, e2 = A.records(*sl)
    assert info(pick)["wild"] == int(A.wild(p0, e1, e2).sum())      # the device's wild rule is the restatement's
    set_mode(pick, OFF)


def test_a_triangle_with_a_nan_vertex_among_good_ones(pick):
    m = grid(700, 31)
    bad = int(m["indices"][333, 1])
    m["vertices"][bad, 1] = np.nan
    n_wild = int((m["indices"] == bad).any(axis=1).sum())
    m2 = grid(90, 32, list=R.LIST_OVERLAY)
    m2["vertices"][int(m2["indices"][5, 0]), 0] = np.inf
    meshes = [m, m2]
    pick.set_meshes(meshes)
    o, d = aimed(meshes, (0.2, 7.0, 2.5), np.random.default_rng(11), 900)
    ref = R.intersect_many(meshes, o, d, full=True)
    on_and_off(pick, o, d, "a NaN vertex", ref=ref)
    assert set_mode(pick, ON) == RXR_OK
    pick.intersect(o, d)
    assert info(pick)["wild"] == n_wild + int((m2["indices"] == m2["indices"][5, 0]).any(axis=1).sum())
    set_mode(pick, OFF)
    assert (ref["mesh"] != R.MISS).sum() > 300


def test_nan_inf_and_zero_direction_rays(pick):
    meshes = [grid(400, 41), grid(30, 42, list=R.LIST_OVERLAY)]
    pick.set_meshes(meshes)
    rng = np.random.default_rng(12)
    o, d = aimed(meshes, (0.0, 6.0, 1.0), rng, 400)
    k = 0
    for arr in (o, d):
        for s in P.SPECIALS:
            for c in range(3):
                arr[k, c] = F(s)
                k += 1
    d[k] = 0
    d[k + 1] = (1e-40, 0, 1e-40)
    d[k + 2] = (np.inf, np.inf, np.inf)
    o[k + 3] = (np.nan, np.nan, np.nan)
    ref = R.intersect_many(meshes, o, d, full=True)
    on_and_off(pick, o, d, "special rays", ref=ref)
    assert (ref["mesh"][k:k + 4] == R.MISS).all() and (ref["mesh"] != R.MISS).sum() > 100


@pytest.mark.parametrize("seed", P.SEEDS[:20])
def test_seeded_scenes(pick, seed):
    meshes = P.random_pick_scene(seed)
    o, d = P.random_rays(meshes, seed, 1000)
    pick.set_meshes(meshes)
    ref = R.intersect_many(meshes, o, d, full=True)
    on_and_off(pick, o, d, f"seed {seed}", ref=ref)
    on_and_off(pick, o[:257], d[:257], f"seed {seed}, 257 rays, plain", full=False, ref=P.prefix(ref, 257))


def test_rebuilds_and_modes(pick):
    a, b = M.grid_mesh(60, 100, 1), M.grid_mesh(50, 80, 2, lst=R.LIST_DYNAMIC)
    for m in (a, b):
        m.update(chunk=-1, has_pid=False, pid=0)
    pick.set_meshes([a, b])
    rng = np.random.default_rng(13)
    o, d = aimed([a, b], (0.0, 0.0, 1.0), rng, 300)
    i0 = info(pick)
    assert (i0["mode"], i0["valid"]) == (OFF, 0)
    on_and_off(pick, o, d, "first build", ref=R.intersect_many([a, b], o, d, full=True))
    i1 = info(pick)
    assert i1["builds"] == i0["builds"] + 1 and (i1["mode"], i1["valid"], i1["triangles"]) == (OFF, 1, 180)
    # mode on again over the same meshes: the tree still stands
    assert set_mode(pick, ON) == RXR_OK
    pick.intersect(o, d)
    assert info(pick)["builds"] == i1["builds"] and info(pick)["mode"] == ON
    # rxr_update_meshes, then a query: one more build, and the new geometry's results
    b2 = M.moved(b, 3)
    counts, v, idx, nr = M.pack([b2])
    named = np.array([1], np.uint32)
    rc = pick.rxr.rxr_update_meshes(pick.ctx, named.ctypes.data, 1, counts.ctypes.data, v.ctypes.data, idx.ctypes.data, nr.ctypes.data, v.shape[1], idx.shape[1])
    assert rc == RXR_OK, pick.error()
    assert info(pick)["valid"] == 0
    o2, d2 = aimed([a, b2], (0.0, 0.0, 1.0), rng, 300)
    ref2 = R.intersect_many([a, b2], o2, d2, full=True)
    got = pick.intersect(o2, d2, full=True)
    assert P.differences(got, ref2, "after rxr_update_meshes:") is None
    i2 = info(pick)
    assert i2["builds"] == i1["builds"] + 1 and i2["valid"] == 1 and i2["batches"] == i1["batches"] + 2
    on_and_off(pick, o2, d2, "after rxr_update_meshes", ref=ref2)
    # rxr_set_meshes again
    c = grid(77, 51)
    pick.set_meshes([c])
    assert info(pick)["valid"] == 0
    o3, d3 = aimed([c], (0.0, 6.0, 1.0), rng, 200)
    on_and_off(pick, o3, d3, "after rxr_set_meshes", ref=R.intersect_many([c], o3, d3, full=True))
    i3 = info(pick)
    assert i3["builds"] == i2["builds"] + 1 and (i3["mode"], i3["valid"], i3["triangles"]) == (OFF, 1, 77)
    # mode off: no build after another rxr_set_meshes, results equal, the info says so
    pick.set_meshes([c, a])
    got = pick.intersect(o3, d3, full=True)
    assert P.differences(got, R.intersect_many([c, a], o3, d3, full=True), "mode off:") is None
    i4 = info(pick)
    assert (i4["mode"], i4["valid"], i4["builds"], i4["batches"]) == (OFF, 0, i3["builds"], i3["batches"])
    # an invalid mode changes nothing
    assert set_mode(pick, 3) == RXR_ERR_INVALID and "rxr_set_ray_accel" in pick.error()
    assert set_mode(pick, 0xFFFFFFFF) == RXR_ERR_INVALID
    assert info(pick)["mode"] == OFF
    # no meshes at all: every ray misses, in both modes
    pick.set_meshes([])
    on_and_off(pick, o3, d3, "no meshes", ref=R.intersect_many([], o3, d3, full=True))


def test_the_tree_culls(pick):
    """a 64 x 64 grid of unit quads in the plane y = 0 (8 192 triangles), 1 024 rays straight down: brute force runs rays x triangles
    tests, the tree at most a quarter of that (any working tree: orders of magnitude fewer)"""
    n = 64
    xs, zs = np.meshgrid(np.arange(n + 1, dtype=F), np.arange(n + 1, dtype=F))
    v = np.stack([xs.ravel(), np.zeros(xs.size, F), zs.ravel(), np.ones(xs.size, F)], axis=1)
    i0 = (np.arange(n)[:, None] * (n + 1) + np.arange(n)[None, :]).ravel()
    idx = np.stack([np.stack([i0, i0 + 1, i0 + n + 2], 1), np.stack([i0, i0 + n + 2, i0 + n + 1], 1)], 1).reshape(-1, 3)
    meshes = [P.mesh(v, idx)]
    pick.set_meshes(meshes)
    rng = np.random.default_rng(14)
    o = np.stack([rng.uniform(0, n, 1024), np.full(1024, 9.0), rng.uniform(0, n, 1024)], axis=1).astype(F)
    d = np.tile(np.array([0, -1, 0], F), (1024, 1))
    before = info(pick)
    got = on_and_off(pick, o, d, "the grid", mode=COUNT)
    after = info(pick)
    assert (got["mesh"] == 0).all() and np.allclose(got["t"], 9.0, atol=1e-3)
    assert after["batches"] == before["batches"] + 1
    print(f"ray-triangle tests: {after['tests']} of {1024 * 8192} ({after['tests'] / 1024:.1f} a ray), nodes {after['nodes']}, levels {after['levels']}")
    assert 1024 <= after["tests"] <= 1024 * 8192 // 4
    # the count is the last counted call's: a second call does not add to it, a call under _ON leaves it
    assert set_mode(pick, COUNT) == RXR_OK
    pick.intersect(o[:512], d[:512])
    half = info(pick)["tests"]
    assert 512 <= half < after["tests"]
    assert set_mode(pick, ON) == RXR_OK
    pick.intersect(o, d)
    assert info(pick)["tests"] == half
    set_mode(pick, OFF)


# ---- the path tracer -------------------------------------------------------------------------------------------------------------
def trace_both(tracer, scene, label, w=24, h=16, bounces=8, seed=5):
    """frames 0 and 1 with the mode off and on: every float of the accumulation buffer equal"""
    S.load(tracer, scene)
    cam = S.cameras(w, h)["firstp"]
    out = {}
    for mode in (OFF, COUNT, ON):
        tracer.ray_accel = mode
        acc = T.AccumBuffer(w, h)
        before = tracer.ray_accel_info()
        tracer.trace(cam, acc, n_frames=2, seed=seed, bounces=bounces)
        after = tracer.ray_accel_info()
        assert acc.frame == 2
        out[mode] = acc.pixels.copy()
        assert after["batches"] - before["batches"] == (0 if mode == OFF else 2 * bounces), (label, mode, before, after)
        if mode == COUNT:
            ntri = sum(len(m["indices"]) for m in scene["meshes"])
            assert 0 < after["tests"] < 2 * bounces * w * h * ntri
    tracer.ray_accel = OFF
    for mode in (COUNT, ON):
        bits = out[mode].view(np.uint32) == out[OFF].view(np.uint32)
        assert bits.all(), f"{label}, mode {mode}: {int((~bits).sum())} floats differ from the brute-force trace"
    assert (out[OFF][..., :3] > 0).any() and len(np.unique(out[OFF][..., 0])) > 8
    return out[OFF]


def test_trace_the_room_with_eight_bounces(tracer):
    trace_both(tracer, S.diffuse_room(), "the diffuse room")
    trace_both(tracer, S.room(), "the room")


def test_trace_a_terrain_sourced_mesh(tracer):
    trace_both(tracer, S.terrain_room(), "the terrain room")


def test_trace_with_meshes_in_the_opacity_and_overlay_lists(tracer):
    front = [S.box(3.0, 1.0, 1.5, 2.5, 2.5, 0.1, source=S.PIXEL(255, 0, 255), list=T.LIST_CHUNK_OPACITY, chunk=0),
             S.box(3.5, 1.5, 1.2, 2.5, 2.5, 0.1, source=S.PIXEL(0, 255, 255), list=T.LIST_OVERLAY)]
    plain = S.diffuse_room()
    with_lists = trace_both(tracer, dict(plain, meshes=[front[0]] + plain["meshes"] + [front[1]]), "opacity and overlay meshes")
    assert R.same(with_lists, trace_both(tracer, plain, "the room without them"))


def test_scene_ray_accel_through_the_mirror(product):
    """Scene.ray_accel hands the mode to the context: the same picks, and the info shows a batch through the tree"""
    meshes = [grid(600, 61), grid(50, 62, list=R.LIST_OVERLAY)]
    scene = P.host_scene(product, meshes)
    o, d = aimed(meshes, (0.3, 6.0, 2.0), np.random.default_rng(15), 500)
    ref = R.intersect_many(meshes, o, d, full=True)
    try:
        assert scene.ray_accel == OFF
        off = scene.intersect(o, d, full=True)
        i0 = scene.ray_accel_info()
        assert i0["mode"] == OFF
        scene.ray_accel = COUNT
        on = scene.intersect(o, d, full=True)
        i1 = scene.ray_accel_info()
        assert (i1["mode"], i1["valid"], i1["triangles"]) == (COUNT, 1, 650) and i1["batches"] == i0["batches"] + 1
        assert 0 < i1["tests"] < 500 * 650
        for got in (off, on):
            assert P.differences(got, ref, "the mirror:") is None
    finally:
        scene.ray_accel = OFF
        scene.intersect(o[:1], d[:1])    # (hands the default back to the shared context)
