"""Ray picking on the device at every threshold of rxr_intersect.hip, against tests/intersect_ref.py::intersect_many: every ray and
every output (t, mesh, triangle, hitpoint, uv, normal) bit for bit, NaN equal to NaN, no tolerance.

  * test_random_pick_scene: seeded scenes and rays (tests/pick_fuzz.py) at 1, 8, 9, 64, 65, 256, 257 and 3 000 rays -- the switches
    ISECT_RAYS_PER_Y, ISECT_FEW_RAYS and ISECT_WG -- and k_isect_by_tri against k_isect_by_ray on the same 64 rays;
  * test_product_scenes_many_rays: cube, teapot and map through k_isect_by_ray;
  * test_ray_batches, test_more_segments_than_keys_per_workgroup_row: isect_run's split into batches of rays (r0 > 0);
  * test_segment_edges_in_the_by_ray_kernel: segment ends at a slice start, an LDS chunk start, the last triangle of a slice and
    several times inside one chunk;
  * test_one_wave_many_segments: one wave of k_isect_by_tri with hits in many segments;
  * test_empty_meshes: meshes without triangles, scenes without triangles, no meshes;
  * test_equal_t_across_meshes_and_segments: ties inside a plain run and across segments;
  * test_two_streams_and_growing_scratch: two caller streams, a growing key scratch, host-array calls and other geometry in between.

The 33 000-segment case is kept: registration, run and reference take about a second.  The module takes about 35 s on an MI355X
box, most of it numpy (test_ray_batches: 12 s of reference).

Scenes are registered through rxr_set_meshes on a context of the test's own (pick_fuzz.PickContext) unless the host mirror is the
point of the test."""
import ctypes as C

import numpy as np
import pytest

import rusterix_amd
from rusterix_amd import scenes
from rusterix_amd.abi import RXR_OK
from tests import intersect_ref as R
from tests import pick_fuzz as P
from tests.test_gpu_intersect import bbox_eye, build, plain_context  # noqa: F401  (plain_context: a fixture)

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def pick():
    with P.PickContext() as ctx:
        yield ctx


def assert_bits(got, ref, label):
    assert set(got) == set(ref), label
    bad = P.differences(got, ref, label)
    assert bad is None, bad


def check_counts(ctx, meshes, o, d, counts, label):
    """every count of `counts` (prefixes of the rays), plain and full, against intersect_many; the full reference"""
    ref = R.intersect_many(meshes, o, d, full=True)
    ctx.set_meshes(meshes)
    for n in counts:
        assert_bits(ctx.intersect(o[:n], d[:n], full=True), P.prefix(ref, n), f"{label}, {n} rays, full")
        assert_bits(ctx.intersect(o[:n], d[:n]), P.prefix(P.plain_of(ref), n), f"{label}, {n} rays, plain")
    return ref


# seeds a sweep (tools/intersect_fuzz_sweep.py) found failing would be added here by name, like seed 1043 in test_gpu_fuzz.py
@pytest.mark.parametrize("seed", P.SEEDS)
def test_random_pick_scene(product, pick, seed):
    bad = P.check_seed(seed, pick)
    assert bad is None, bad


@pytest.mark.parametrize("seed", P.SEEDS[:4])
def test_random_pick_scene_through_the_host_mirror(product, plain_context, seed):
    """the same scenes pushed batch by batch into the host mirror's Scene (without the meshes that have no vertices: the mirror
    cannot hold them), 3 000 rays: Scene.intersect registers them in the order the generator lists them"""
    meshes = [m for m in P.random_pick_scene(seed) if len(m["vertices"])]
    o, d = P.random_rays(meshes, seed, 3000)
    scene = P.host_scene(product, meshes)
    assert_bits(scene.intersect(o, d, full=True), R.intersect_many(meshes, o, d, full=True), f"seed {seed}")


def many_rays(meshes, eye, rng, n_aimed=700, n_random=300):
    """rays from around `eye` at centroids, edge midpoints, vertices and random points of random triangles (drawn with replacement:
    the cube has 12), and random directions; shuffled"""
    tris = [(mi, k) for mi, m in enumerate(meshes) for k in range(len(m["indices"]))]
    o = (np.asarray(eye, F)[None, :] + rng.standard_normal((n_aimed + n_random, 3)) * 0.2).astype(F)
    d = rng.standard_normal((n_aimed + n_random, 3)).astype(F)
    for j, p in enumerate(rng.integers(0, len(tris), n_aimed)):
        mi, k = tris[p]
        v = meshes[mi]["vertices"][meshes[mi]["indices"][k].astype(np.int64), :3].astype(F)
        w = rng.dirichlet(np.ones(3)).astype(F)
        target = [(v[0] + v[1] + v[2]) / F(3.0), (v[0] + v[1]) * F(0.5), v[0], w[0] * v[0] + w[1] * v[1] + w[2] * v[2]][j % 4]
        d[j] = (target - o[j]) * F(rng.uniform(0.01, 100.0))
    order = rng.permutation(len(o))
    return np.ascontiguousarray(o[order]), np.ascontiguousarray(d[order])


@pytest.mark.parametrize("name", ["cube", "teapot", "map"])
def test_product_scenes_many_rays(product, plain_context, name):
    builder = dict(cube=lambda api: scenes.cube_scene(api, 160, 120, 40),
                   teapot=lambda api: scenes.teapot_scene(api, 160, 120, 40, logo_size=64),
                   map=lambda api: scenes.map_scene(api, 160, 96, 40, logo_size=64))[name]
    cfg, meshes = build(product, builder)
    rng = np.random.default_rng(23)
    o, d = many_rays(meshes, bbox_eye(meshes), rng)
    ref = R.intersect_many(meshes, o, d, full=True)
    assert (ref["mesh"] != R.MISS).sum() >= 300
    for n in (1000, 65):    # (both through k_isect_by_ray)
        assert_bits(cfg.scene.intersect(o[:n], d[:n], full=True), P.prefix(ref, n), f"{name}, {n} rays, full")
        assert_bits(cfg.scene.intersect(o[:n], d[:n]), P.prefix(P.plain_of(ref), n), f"{name}, {n} rays, plain")


def quad_at(z, lst, pid=None, size=1.0):
    v = np.array([(0, 0, z, 1), (size, 0, z, 1), (size, size, z, 1), (0, size, z, 1)], F)
    uv = np.array([(0.1, 0.2), (0.9, 0.3), (0.8, 0.7), (0.2, 0.95)], F) + F(z)
    nr = np.array([(0.1, 0.2, -1.0), (-0.2, 0.1, -0.9), (0.3, -0.1, -1.1), (0.0, 0.3, -0.8)], F)
    return P.mesh(v, [(0, 1, 2), (0, 2, 3)], uv, nr, list=lst, chunk=0 if lst == R.LIST_CHUNK else -1, pid=pid)


def test_ray_batches(product, pick):
    """300 one-quad segments and 32 768 rays need more keys than ISECT_KEYS_MAX: isect_run splits the rays, the keys are indexed
    by the ray's place in its batch and the outputs by its place in the call"""
    import torch

    k = P.kernel_constants()
    # chunk quads with distinct profile ids come first, nearest last; overlays (registered after them) at their own depths
    chunk = [quad_at(300.0 - i, R.LIST_CHUNK, pid=i, size=1.0 + 0.01 * (i % 7)) for i in range(150)]
    overlay = [quad_at(400.0 + i, R.LIST_OVERLAY, pid=i % 3, size=1.0 - 0.005 * i) for i in range(150)]
    meshes = chunk + overlay
    segs = P.segments(meshes)
    assert len(segs) == 300 and sum(len(m["indices"]) for m in meshes) == 600
    n = 32768
    batches = P.expected_batches(n, len(segs), k)
    assert len(batches) > 1 and n * len(segs) > k["ISECT_KEYS_MAX"], batches
    # straight and slanted rays over [-0.2, 1.2]^2: misses outside, the last (smallest) overlay that still covers the ray
    # inside the unit square, the last chunk quad that does on the rim around it -- all of it on both sides of every split
    rng = np.random.default_rng(77)
    o = np.concatenate([rng.uniform(-0.2, 1.2, (n, 2)), np.full((n, 1), -5.0)], axis=1).astype(F)
    d = np.concatenate([rng.standard_normal((n, 2)) * 1e-4, rng.uniform(0.5, 2.0, (n, 1))], axis=1).astype(F)
    ref = R.intersect_many(meshes, o, d, full=True)
    r0 = 0
    for nb in batches:
        part = ref["mesh"][r0:r0 + nb]
        assert (part == R.MISS).any() and len(np.unique(part[part != R.MISS])) >= 20, "every batch is to hold misses and many winners"
        assert (part[part != R.MISS] < 150).any() and (part[part != R.MISS] >= 150).any()
        r0 += nb
    pick.set_meshes(meshes)
    assert_bits(pick.intersect(o, d, full=True), ref, "rxr_intersect, full")
    assert_bits(pick.intersect(o, d), P.plain_of(ref), "rxr_intersect, plain")
    stream = torch.cuda.Stream()
    dev = pick.intersect_to(o, d, full=True, stream=stream)
    stream.synchronize()
    assert_bits(P.to_host(dev), ref, "rxr_intersect_to on a caller stream")


def test_more_segments_than_keys_per_workgroup_row(product):
    """33 000 one-triangle overlay segments: ISECT_KEYS_MAX / nseg is below ISECT_WG, the batch is ISECT_WG rays (the floor of
    isect_run's formula) -- 600 rays in batches of 256, 256 and 88"""
    k = P.kernel_constants()
    nm, n = 33000, 600
    assert P.expected_batches(n, nm, k) == [k["ISECT_WG"], k["ISECT_WG"], n - 2 * k["ISECT_WG"]]
    rng = np.random.default_rng(5)
    c = rng.uniform(-1.0, 1.0, (nm, 1, 3)) * np.array([4.0, 4.0, 1.0])
    tri = (c + rng.standard_normal((nm, 3, 3)) * 0.35).astype(F)
    verts = np.concatenate([tri, np.ones((nm, 3, 1), F)], axis=2)
    one = np.array([[0, 1, 2]], np.uint32)
    uvs, nrm = rng.uniform(0, 1, (nm, 3, 2)).astype(F), rng.standard_normal((nm, 3, 3)).astype(F)
    meshes = [dict(vertices=verts[i], indices=one, uvs=uvs[i], normals=nrm[i], list=R.LIST_OVERLAY, chunk=-1, has_pid=False, pid=0)
              for i in range(nm)]
    o = np.concatenate([rng.uniform(-4.0, 4.0, (n, 2)), np.full((n, 1), -6.0)], axis=1).astype(F)
    d = np.concatenate([rng.standard_normal((n, 2)) * 0.05, np.ones((n, 1))], axis=1).astype(F)
    ref = R.intersect_many(meshes, o, d, full=True)
    assert (ref["mesh"] != R.MISS).mean() > 0.9 and len(np.unique(ref["mesh"])) > 200
    with P.PickContext(meshes) as ctx:
        assert_bits(ctx.intersect(o, d, full=True), ref, "33 000 segments")


def fan(n, z, lst, pid=None):
    """n triangles over the square [-1, 1]^2 at depth z: a fan around its centre, the rim cut into n pieces (the pieces cut the
    corners off: from 64 triangles on it covers [-0.9, 0.9]^2); fewer than 8: n copies of one large triangle"""
    rng = np.random.default_rng(n)
    if n < 8:
        v = np.tile(np.array([(-4, -3, z, 1), (4, -3, z, 1), (0, 6, z, 1)], F), (n, 1))
        return P.mesh(v, np.arange(3 * n).reshape(n, 3), rng.uniform(0, 1, (3 * n, 2)), rng.standard_normal((3 * n, 3)), list=lst,
                      chunk=0 if lst == R.LIST_CHUNK else -1, pid=pid)
    s = np.arange(n + 1, dtype=np.float64) * (8.0 / n)      # the rim by arc length, 0 .. 8
    side, u = np.minimum(s // 2, 3).astype(int), s % 2
    u[-1], side[-1] = 0.0, 0
    x = np.select([side == 0, side == 1, side == 2, side == 3], [u - 1, np.ones_like(u), 1 - u, -np.ones_like(u)])
    y = np.select([side == 0, side == 1, side == 2, side == 3], [-np.ones_like(u), u - 1, np.ones_like(u), 1 - u])
    v = np.concatenate([[[0.0, 0.0, z, 1.0]], np.stack([x, y, np.full(n + 1, z), np.ones(n + 1)], axis=1)]).astype(F)
    idx = np.stack([np.zeros(n, np.uint32), np.arange(1, n + 1, dtype=np.uint32), np.arange(2, n + 2, dtype=np.uint32)], axis=1)
    return P.mesh(v, idx, rng.uniform(0, 1, (n + 2, 2)), rng.standard_normal((n + 2, 3)), list=lst, chunk=0 if lst == R.LIST_CHUNK else -1, pid=pid)


def test_segment_edges_in_the_by_ray_kernel(product, pick):
    """4 096 triangles in 7 one-mesh segments of 1024, 1, 1023, 256, 255, 257 and 1280: with 65 to 256 rays k_isect_by_ray runs 4
    slices of 1 024, and a segment ends at a slice start (1024, 2048), one triangle later (1025), at LDS chunk starts (2304), one
    before (2559) and after them (2816), and twice within one chunk.  Every mesh covers the same square, every ray hits all."""
    sizes = [1024, 1, 1023, 256, 255, 257, 1280]
    # plain / profile id / overlay in turn; depths chosen so that no rule is idle:
    #   0 plain z=5 | 1 chunk id 1 z=4 (nearer: wins) | 2 overlay z=9 (wins) | 3 static z=7 (nearer: wins) | 4 chunk id 2 z=6 (wins)
    #   | 5 overlay z=8 (wins, id 2) | 6 chunk id 2 z=3: nearer, but the best has the same id -- the overlay stays
    spec = [(R.LIST_STATIC, None, 5.0), (R.LIST_CHUNK, 1, 4.0), (R.LIST_OVERLAY, None, 9.0), (R.LIST_STATIC, None, 7.0),
            (R.LIST_CHUNK, 2, 6.0), (R.LIST_OVERLAY, 2, 8.0), (R.LIST_CHUNK, 2, 3.0)]
    meshes = [fan(n, z, lst, pid) for n, (lst, pid, z) in zip(sizes, spec)]
    # (chunk meshes after an overlay: an order rxr_set_meshes takes, though the host mirror never produces it)
    assert [s[1] for s in P.segments(meshes)] == [1024, 1025, 2048, 2304, 2559, 2816, 4096]
    rng = np.random.default_rng(31)
    n = 3000
    o = np.concatenate([rng.uniform(-0.7, 0.7, (n, 2)), np.full((n, 1), -2.0)], axis=1).astype(F)
    d = np.zeros((n, 3), F)
    d[:, 2] = rng.uniform(0.5, 3.0, n).astype(F)
    slanted = np.arange(n) % 3 == 2
    d[slanted, :2] = (rng.standard_normal((int(slanted.sum()), 2)) * 0.02).astype(F)
    ref = check_counts(pick, meshes, o, d, (64, 65, 200, 256, 257, 3000), "fans")
    straight = ~slanted
    assert np.all(ref["mesh"][straight] == 5) and np.all(np.abs(ref["t"][straight] - F(10.0)) < 1e-3)   # (z = 8 from z = -2)
    # without the last mesh's profile id the nearest mesh wins: the rule above decided
    assert np.all(R.intersect_many(meshes[:6] + [dict(meshes[6], has_pid=False)], o[:16], d[:16])["mesh"][~slanted[:16]] == 6)
    # the same with each rule alone in front: the winner is read off the depths
    for keep, winner in (([0, 1], 1), ([0, 1, 2], 2), ([0, 3], 0), ([3, 4, 6], 4), ([3, 6], 6), ([4, 6], 4)):
        sub = [meshes[i] for i in keep]
        r = check_counts(pick, sub, o[:300], d[:300], (64, 65, 300), f"fans {keep}")
        assert np.all(r["mesh"][:300][straight[:300]] == keep.index(winner)), keep


def test_one_wave_many_segments(product, pick):
    """40 meshes of 1 to 3 triangles, each a segment of its own, 79 triangles: two waves of k_isect_by_tri whose hits lie in many
    segments (an atomic per hitting lane; `seg` of the first hitting lane is not the others'); then the same with 100 rays"""
    rng = np.random.default_rng(40)
    meshes = []
    for i in range(40):
        n = 1 + i % 3
        z = float(rng.uniform(1.0, 9.0))
        # n large triangles, each covering the unit square around the origin
        v = np.concatenate([np.array([(-4, -3, z, 1), (4, -3, z, 1), (0, 6, z, 1)], F) + np.array([0, 0, 0.01 * j, 0], F) for j in range(n)])
        v[:, :2] += rng.uniform(-0.3, 0.3, (3 * n, 2)).astype(F)
        lst, pid = (R.LIST_OVERLAY, None) if i % 4 == 3 else (R.LIST_CHUNK, i % 5)
        if lst == R.LIST_OVERLAY:
            v[:, :2] *= F(rng.uniform(0.15, 0.6))     # (an overlay covers part of the rays only: it wins wherever it is hit)
        meshes.append(P.mesh(v, np.arange(3 * n).reshape(n, 3), rng.uniform(0, 1, (3 * n, 2)), rng.standard_normal((3 * n, 3)),
                             list=lst, chunk=0 if lst == R.LIST_CHUNK else -1, pid=pid))
    assert len(P.segments(meshes)) == 40
    n = 100
    o = np.concatenate([rng.uniform(-1.5, 1.5, (n, 2)), np.full((n, 1), -1.0)], axis=1).astype(F)
    d = np.concatenate([rng.standard_normal((n, 2)) * 0.05, np.ones((n, 1))], axis=1).astype(F)
    o[::10, 0] = 30.0   # (some miss everything)
    alone = [R.intersect_many([m], o, d)["mesh"] != R.MISS for m in meshes]
    assert np.median(np.sum(alone, axis=0)) >= 30, "most rays are to hit most meshes"
    ref = check_counts(pick, meshes, o, d, (16, 100), "40 segments")
    assert len(np.unique(ref["mesh"])) >= 4 and (ref["mesh"] == R.MISS).any()


def test_empty_meshes(product, pick):
    rng = np.random.default_rng(6)
    none = lambda lst=R.LIST_STATIC, nv=0, pid=None: P.mesh(rng.standard_normal((nv, 4)), np.zeros((0, 3), np.uint32), list=lst, pid=pid,
                                                          chunk=0 if lst <= R.LIST_CHUNK_TERRAIN else -1)
    q = lambda z, lst, pid=None: quad_at(z, lst, pid)
    meshes = [none(R.LIST_CHUNK_OPACITY), none(R.LIST_CHUNK, 3, pid=1),              # first
              q(9.0, R.LIST_CHUNK, 1), none(R.LIST_CHUNK, 0, pid=1), none(R.LIST_CHUNK, 2), q(8.0, R.LIST_CHUNK, 1),   # between two id segments
              q(7.0, R.LIST_CHUNK, 2),
              q(6.0, R.LIST_STATIC), none(R.LIST_STATIC, 5), none(R.LIST_STATIC), q(5.0, R.LIST_STATIC), q(5.5, R.LIST_DYNAMIC),  # inside a run
              none(R.LIST_DYNAMIC), q(20.0, R.LIST_OVERLAY, 1), none(R.LIST_OVERLAY, 1), none(R.LIST_OVERLAY)]          # last
    assert [s[2:] for s in P.segments(meshes)] == [(2, 3, "pid"), (5, 6, "pid"), (6, 7, "pid"), (7, 12, "plain"), (13, 14, "overlay")]
    n = 300
    o = np.concatenate([rng.uniform(-0.3, 1.3, (n, 2)), np.full((n, 1), -1.0)], axis=1).astype(F)
    d = np.concatenate([rng.standard_normal((n, 2)) * 0.01, np.ones((n, 1))], axis=1).astype(F)
    d[::2, :2] = 0.0
    ref = check_counts(pick, meshes, o, d, (9, 64, 65, 300), "empty meshes")
    inside = (o[:, 0] > 0.05) & (o[:, 0] < 0.95) & (o[:, 1] > 0.05) & (o[:, 1] < 0.95) & (np.arange(n) % 2 == 0)   # (straight rays)
    assert np.all(ref["mesh"][inside] == 13) and (ref["mesh"] == R.MISS).any()     # the overlay, by its registered index
    # without the overlay the registered index of the winner shows: mesh 10 (z = 5) behind two empty meshes of its run
    ref = check_counts(pick, meshes[:13], o, d, (9, 64, 65, 300), "empty meshes, no overlay")
    assert np.all(ref["mesh"][inside] == 10)
    # ... and with the chunk meshes alone: 2 (z = 9) is hit first, 5 (same id, nearer) is kept out, 6 (another id, nearer) wins
    ref = check_counts(pick, meshes[:7], o, d, (9, 64, 65, 300), "empty meshes, chunk only")
    assert np.all(ref["mesh"][inside] == 6)
    ref = check_counts(pick, meshes[:6], o, d, (9, 65), "empty meshes, one profile id")
    assert np.all(ref["mesh"][inside] == 2)
    # scenes without a triangle, and no meshes at all: every ray misses
    for label, ms in (("only empty meshes", [none(), none(R.LIST_OVERLAY, 4), none(R.LIST_CHUNK, 2, pid=1)]), ("no meshes", [])):
        pick.set_meshes(ms)
        for cnt in (1, 64, 65, 300):
            for full in (False, True):
                got = pick.intersect(o[:cnt], d[:cnt], full=full)
                assert np.all(got["t"] == R.FLT_MAX) and np.all(got["mesh"] == R.MISS) and np.all(got["triangle"] == 0), label
                assert all(not got[key].any() for key in got if key in ("hitpoint", "uv", "normal")), label
                assert_bits(got, R.intersect_many(ms, o[:cnt], d[:cnt], full=full), label)


def test_equal_t_across_meshes_and_segments(product, pick):
    """the same quad registered many times: inside a plain run the key's triangle index keeps the earliest, across segments the
    fold's strict `<` does, an overlay copy takes it anyway, a chunk copy with the best's profile id never does"""
    q = lambda lst, pid=None: quad_at(2.0, lst, pid)
    cases = [([q(R.LIST_STATIC), q(R.LIST_STATIC), q(R.LIST_DYNAMIC)], 0),
             ([q(R.LIST_CHUNK, 1), q(R.LIST_CHUNK, 2), q(R.LIST_STATIC)], 0),
             ([q(R.LIST_STATIC), q(R.LIST_OVERLAY), q(R.LIST_OVERLAY)], 2),
             ([q(R.LIST_CHUNK_OPACITY), q(R.LIST_CHUNK, 1), q(R.LIST_CHUNK), q(R.LIST_CHUNK_TERRAIN)], 0)]
    rng = np.random.default_rng(8)
    n = 200
    o = np.concatenate([rng.uniform(0.3, 0.7, (n, 2)), np.full((n, 1), -1.0)], axis=1).astype(F)
    d = np.concatenate([rng.standard_normal((n, 2)) * 0.01, rng.uniform(0.5, 2.0, (n, 1))], axis=1).astype(F)
    for meshes, winner in cases:
        # the duplicated triangle inside one mesh as well: the earlier index
        meshes[0] = dict(meshes[0], indices=np.array([(0, 1, 2), (0, 2, 3), (0, 1, 2), (0, 2, 3)], np.uint32))
        ref = check_counts(pick, meshes, o, d, (16, 64, 65, 200), f"copies {[m['list'] for m in meshes]}")
        assert np.all(ref["mesh"] == winner) and np.all(ref["triangle"] < 2)


def test_two_streams_and_growing_scratch(product, plain_context):
    """one context, two caller streams taking turns with growing ray counts (each growth reallocates the key scratch while the
    other stream's call may still run), a host-array call and other geometry in between: every call's result is that of the
    geometry registered when it was queued"""
    import torch

    rxr = rusterix_amd.rxr_abi()
    mk = lambda seed: [m for m in P.random_pick_scene(seed) if len(m["vertices"])]
    meshes_a = next(m for m in (mk(s) for s in P.SEEDS) if len(P.segments(m)) >= 8 and sum(len(x["indices"]) for x in m) < 1500)
    meshes_b = [quad_at(2.0, R.LIST_STATIC), quad_at(1.0, R.LIST_OVERLAY, size=0.5)]
    scene_a, scene_b = P.host_scene(product, meshes_a), P.host_scene(product, meshes_b)
    ctx = product.lib.rxh_context()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    rays = {n: P.random_rays(meshes_a, 1000 + n, n) for n in (100, 1000, 10000, 100000)}
    small = P.random_rays(meshes_a, 7, 500)
    scene_a.intersect(small[0][:1], small[1][:1])      # (registers scene a)
    queued, host_results = [], []

    def queue(n, stream, full):
        o, d = rays[n]
        dev = dict(o=torch.from_numpy(o).cuda(), d=torch.from_numpy(d).cuda())
        shapes = dict(t=(n,), mesh=(n,), triangle=(n,), hitpoint=(n, 3), **(dict(uv=(n, 2), normal=(n, 3)) if full else {}))
        for key, shp in shapes.items():
            dev[key] = torch.full(shp, -7, dtype=torch.int32 if key in ("mesh", "triangle") else torch.float32, device="cuda")
        torch.cuda.current_stream().synchronize()       # (the inputs are written before the caller stream reads them)
        p = lambda key: dev[key].data_ptr() if key in dev else None
        rc = rxr.rxr_intersect_to(ctx, p("o"), p("d"), n, 1 if full else 0, p("t"), p("mesh"), p("triangle"), p("hitpoint"), p("uv"),
                                  p("normal"), stream.cuda_stream)
        assert rc == RXR_OK, rxr.rxr_last_error(ctx)
        queued.append((f"{n} rays, stream {streams.index(stream)}, full={full}", dev, o, d, full))

    queue(100, streams[0], True)
    queue(1000, streams[1], False)
    host_results.append(("host-array call, scene a", scene_a.intersect(*small, full=True), meshes_a))
    queue(10000, streams[0], True)
    queue(100000, streams[1], True)
    # other geometry and back: Scene.intersect registers its own meshes (rxr_set_meshes waits for what is queued)
    host_results.append(("host-array call, scene b", scene_b.intersect(*small, full=True), meshes_b))
    host_results.append(("host-array call, scene a again", scene_a.intersect(*small, full=True), meshes_a))
    queue(100000, streams[0], False)
    queue(1000, streams[1], True)
    queue(10000, streams[1], False)
    queue(100, streams[0], False)
    for s in streams:
        s.synchronize()
    for label, got, meshes in host_results:
        assert_bits(got, R.intersect_many(meshes, *small, full=True), label)
    refs = {}
    for label, dev, o, d, full in queued:
        if len(o) not in refs:
            refs[len(o)] = R.intersect_many(meshes_a, o, d, full=True)
        ref = refs[len(o)]
        assert_bits(P.to_host(dev), ref if full else P.plain_of(ref), label)
