"""A wave per ray through the ray box tree on the device (rxr_set_ray_wave / rxr_ray_wave_info; k_accel_by_wave,
rusterix_amd/csrc/rxr_ray_accel.hip).  Under RXR_RAY_WAVE_FORCE, so that small scenes reach the kernel, every
output word of rxr_intersect -- RXR_INTERSECT_FULL and plain -- is what the same context writes with both switches off and, for scenes
up to 4 097 triangles, what tests/intersect_ref.py computes; every float of the path tracer's accumulation buffer likewise.
rxr_ray_wave_info's BATCHES and RAYS move by exactly the batches and rays sent -- the proof that the kernel ran -- and
RXR_RAY_ACCEL_INFO_BATCHES, the thread walk's, does not move.  Every test calls rxr_set_ray_wave: none passes on a library without it."""
import ctypes as C
import functools

import numpy as np
import pytest

from rusterix_amd import trace as T
from rusterix_amd.abi import RXR_ERR_INVALID, RXR_OK
from tests import intersect_ref as R
from tests import mesh_update_ref as M
from tests import pick_fuzz as P
from tests import ray_accel_ref as A
from tests import ray_wave_ref as V
from tests import trace_scenes as S

pytestmark = pytest.mark.gpu
F = np.float32
OFF, ON, COUNT = T.RAY_ACCEL_OFF, T.RAY_ACCEL_ON, T.RAY_ACCEL_COUNT
W_OFF, W_ON, W_FORCE = T.RAY_WAVE_OFF, T.RAY_WAVE_ON, T.RAY_WAVE_FORCE
L = A.LEAF
NTRI = (1, 7, 8, 9, 63, 64, 65, 511, 512, 513, 4095, 4096, 4097, 32769)
RAYS = (1, 3, 4, 5, 64, 65, 300)
REF_MAX = 4097      # scenes up to this many triangles are also held to tests/intersect_ref.py


@pytest.fixture(scope="module")
def pick():
    with P.PickContext() as ctx:
        ctx.registered = None
        yield ctx


@pytest.fixture(scope="module")
def tracer():
    with T.Tracer() as tr:
        yield tr


def set_accel(ctx, mode):
    return ctx.rxr.rxr_set_ray_accel(ctx.ctx, mode)


def set_wave(ctx, mode):
    return ctx.rxr.rxr_set_ray_wave(ctx.ctx, mode)


def set_refresh(ctx, mode):
    return ctx.rxr.rxr_set_ray_refresh(ctx.ctx, mode)


def accel_info(ctx):
    out = (C.c_uint64 * len(T.RAY_ACCEL_INFO))()
    assert ctx.rxr.rxr_ray_accel_info(ctx.ctx, out) == RXR_OK, ctx.error()
    return dict(zip(T.RAY_ACCEL_INFO, (int(x) for x in out)))


def wave_info(ctx):
    out = (C.c_uint64 * len(T.RAY_WAVE_INFO))()
    assert ctx.rxr.rxr_ray_wave_info(ctx.ctx, out) == RXR_OK, ctx.error()
    return dict(zip(T.RAY_WAVE_INFO, (int(x) for x in out)))


def register(ctx, meshes, key=None):
    if key is None or ctx.registered != key:
        ctx.set_meshes(meshes)
    ctx.registered = key


def wave_and_off(ctx, meshes, o, d, label, ref=None, accel=ON):
    """both switches off, then the tree on and RXR_RAY_WAVE_FORCE, on the same context, full and plain: every output word equal (and
    equal to `ref`), the wave counters moved by what was sent, the thread walk's batch counter not at all; returns the full result"""
    nseg = len(P.segments(meshes))
    sent = len(P.expected_batches(len(o), nseg)) if nseg else 0      # (no triangle registered: nothing is launched)
    assert set_accel(ctx, OFF) == RXR_OK and set_wave(ctx, W_OFF) == RXR_OK
    off = {full: ctx.intersect(o, d, full=full) for full in (True, False)}
    assert set_accel(ctx, accel) == RXR_OK and set_wave(ctx, W_FORCE) == RXR_OK
    got = {}
    for full in (True, False):
        w0, a0 = wave_info(ctx), accel_info(ctx)
        got[full] = ctx.intersect(o, d, full=full)
        w1, a1 = wave_info(ctx), accel_info(ctx)
        assert (w1["mode"], w1["batches"] - w0["batches"], w1["rays"] - w0["rays"]) == (W_FORCE, sent, len(o) if sent else 0), (label, full, w0, w1)
        assert a1["batches"] == a0["batches"], (label, a0, a1)
    assert set_accel(ctx, OFF) == RXR_OK and set_wave(ctx, W_OFF) == RXR_OK
    for full in (True, False):
        bad = P.differences(got[full], off[full], f"{label}, full={full}: a wave per ray against both switches off,")
        assert bad is None, bad
        if ref is not None:
            bad = P.differences(off[full], ref if full else P.plain_of(ref), f"{label}, full={full}: against the restatement,")
            assert bad is None, bad
    return got[True]


# the generators of tests/test_gpu_ray_accel.py, restated
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


# ---- tree sizes x ray counts -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sized_scene(ntri):
    """(meshes, 300 aimed rays, the restatement's answer or None): computed once, shared by the ray counts, left unchanged"""
    meshes = [grid(ntri, 100 + ntri)]
    o, d = aimed(meshes, (0.5, 7.0, 3.0), np.random.default_rng(ntri), 300)
    ref = R.intersect_many(meshes, o, d, full=True) if ntri <= REF_MAX else None
    return meshes, o, d, ref


@pytest.mark.parametrize("n_rays", RAYS)
@pytest.mark.parametrize("ntri", NTRI)
def test_tree_sizes_and_ray_counts(pick, ntri, n_rays):
    """tops 0 to 5 of both parities with ragged last nodes; partial workgroups of four rays and both sides of ISECT_FEW_RAYS"""
    meshes, o, d, ref = sized_scene(ntri)
    register(pick, meshes, ("sized", ntri))
    got = wave_and_off(pick, meshes, o[:n_rays], d[:n_rays], f"{ntri} triangles, {n_rays} rays", ref=None if ref is None else P.prefix(ref, n_rays))
    if n_rays == 300:
        assert (got["mesh"] != R.MISS).sum() > 50       # (tests/test_gpu_ray_accel.py's condition: not passed on misses alone)
        i = accel_info(pick)
        cnt = A.levels(ntri)
        assert (i["valid"], i["triangles"], i["nodes"], i["levels"]) == (1, ntri, sum(cnt), len(cnt)), i


# ---- the scenes of the existing tree tests ---------------------------------------------------------------------------------------
def test_a_leaf_across_two_meshes_and_two_segments(pick):
    meshes = [grid(5, 1), grid(7, 2, list=R.LIST_OVERLAY), grid(L + 3, 3, list=R.LIST_OVERLAY), grid(2, 4, list=R.LIST_OVERLAY)]
    register(pick, meshes)
    o, d = aimed(meshes, (0.2, 6.0, 4.0), np.random.default_rng(5), 400)
    ref = R.intersect_many(meshes, o, d, full=True)
    wave_and_off(pick, meshes, o, d, "a leaf across meshes", ref=ref)
    assert len(np.unique(ref["mesh"])) >= 4


def test_64_positions_that_straddle_three_segments(pick):
    """one level-1 node over a plain segment of 20 triangles and two overlay segments of 13 and 40: no lane-uniform segment, every
    hit lane finds its own; then the next node lies in one segment again"""
    meshes = [grid(20, 71), grid(13, 72, list=R.LIST_OVERLAY), grid(40, 73, list=R.LIST_OVERLAY)]
    segs = P.segments(meshes)
    assert len(segs) == 3 and segs[0][1] < 64 and segs[1][1] < 64 < segs[2][1]
    register(pick, meshes)
    o, d = aimed(meshes, (0.3, 6.5, 3.5), np.random.default_rng(74), 300)
    ref = R.intersect_many(meshes, o, d, full=True)
    wave_and_off(pick, meshes, o, d, "three segments in 64 positions", ref=ref)
    assert set(np.unique(ref["mesh"])) >= {0, 1, 2}


def test_several_segments_in_one_scene(pick):
    """a plain run, chunk meshes with equal and with different profile ids, overlay meshes, a mesh without triangles between them"""
    meshes = [grid(30, 1, list=R.LIST_CHUNK_OPACITY, chunk=0), grid(70, 2, list=R.LIST_CHUNK, chunk=0), grid(9, 3, list=R.LIST_CHUNK, chunk=0, pid=4),
              grid(64, 4, list=R.LIST_CHUNK, chunk=0, pid=4), grid(65, 5, list=R.LIST_CHUNK, chunk=0, pid=5), grid(0, 6, list=R.LIST_CHUNK, chunk=0, pid=5),
              grid(33, 7, list=R.LIST_CHUNK_TERRAIN, chunk=0), grid(200, 8), grid(17, 9, list=R.LIST_DYNAMIC), grid(40, 10, list=R.LIST_OVERLAY),
              grid(3, 11, list=R.LIST_OVERLAY)]
    assert len(P.segments(meshes)) >= 6
    register(pick, meshes)
    o, d = aimed(meshes, (0.4, 8.0, 2.0), np.random.default_rng(6), 700)
    ref = R.intersect_many(meshes, o, d, full=True)
    wave_and_off(pick, meshes, o, d, "several segments", ref=ref)
    assert len(np.unique(ref["mesh"])) >= 8


def test_no_meshes_registered(pick):
    register(pick, [])
    o, d = aimed([grid(77, 51)], (0.0, 6.0, 1.0), np.random.default_rng(13), 100)
    got = wave_and_off(pick, [], o, d, "no meshes", ref=R.intersect_many([], o, d, full=True))
    assert (got["mesh"] == R.MISS).all()


def test_identical_triangles_the_earliest_wins(pick):
    """equal t: 150 copies of one triangle in a mesh, the same again in a second mesh and in an overlay"""
    v = np.array([(0, 0, 0, 1), (2, 0, 0, 1), (0, 2, 0, 1)], F)
    idx = np.tile(np.array([(0, 1, 2)], np.uint32), (150, 1))
    meshes = [P.mesh(v, idx), P.mesh(v, idx, list=R.LIST_DYNAMIC), P.mesh(v, idx[:9], list=R.LIST_OVERLAY)]
    o, d = aimed(meshes, (0.5, 0.5, -5.0), np.random.default_rng(8), 200)
    register(pick, meshes[:2])
    got = wave_and_off(pick, meshes[:2], o, d, "identical triangles", ref=R.intersect_many(meshes[:2], o, d, full=True))
    hit = got["mesh"] != R.MISS
    assert hit.sum() > 100 and (got["mesh"][hit] == 0).all() and (got["triangle"][hit] == 0).all()
    register(pick, meshes)
    got = wave_and_off(pick, meshes, o, d, "identical triangles under an overlay", ref=R.intersect_many(meshes, o, d, full=True))
    assert (got["mesh"][hit] == 2).all() and (got["triangle"][hit] == 0).all()


def test_wild_triangles_a_nan_vertex_and_slivers(pick):
    rng = np.random.default_rng(10)
    m = grid(700, 31)
    m["vertices"][int(m["indices"][333, 1]), 1] = np.nan
    sl = A.triangles(rng, 200, "sliver")
    with np.errstate(all="ignore"):
        p0, e1, e2 = A.records(*sl)
        assert (A.kappa(e1, e2) > A.KAPPA_CAP).sum() > 5          # slivers too thin for a box: always tested
    slivers = np.concatenate([np.stack(sl, axis=1).reshape(-1, 3), np.ones((600, 1), F)], axis=1)
    meshes = [m, P.mesh(slivers, np.arange(600, dtype=np.uint32).reshape(-1, 3), list=R.LIST_DYNAMIC)]
    register(pick, meshes)
    o1, d1 = aimed(meshes[:1], (0.2, 7.0, 2.5), rng, 300)
    o2, d2 = A.aimed_rays(rng, *sl)
    o, d = np.concatenate([o1, o2]), np.concatenate([d1, d2])
    ref = R.intersect_many(meshes, o, d, full=True)
    wave_and_off(pick, meshes, o, d, "wild triangles", ref=ref)
    assert (ref["mesh"] == 0).sum() > 50 and (ref["mesh"] == 1).sum() > 30
    assert accel_info(pick)["wild"] >= 6


def test_nan_inf_and_zero_direction_rays(pick):
    meshes = [grid(400, 41), grid(30, 42, list=R.LIST_OVERLAY)]
    register(pick, meshes)
    o, d = aimed(meshes, (0.0, 6.0, 1.0), np.random.default_rng(12), 400)
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
    wave_and_off(pick, meshes, o, d, "special rays", ref=ref)
    assert (ref["mesh"][k:k + 4] == R.MISS).all() and (ref["mesh"] != R.MISS).sum() > 100


def test_rays_that_hit_nothing_by_construction(pick):
    meshes = [grid(513, 81)]
    register(pick, meshes)
    v = meshes[0]["vertices"][:, :3]
    centre = v.mean(axis=0)
    rng = np.random.default_rng(82)
    o = (centre + np.array([0, 40.0, 0], F) + rng.standard_normal((130, 3)) * 0.1).astype(F)
    d = (o - centre).astype(F)                        # away from everything
    got = wave_and_off(pick, meshes, o, d, "rays that leave", ref=R.intersect_many(meshes, o, d, full=True))
    assert (got["mesh"] == R.MISS).all()


# ---- the count ---------------------------------------------------------------------------------------------------------------------
def device_nodes(ctx, ntri):
    n = C.c_uint64()
    assert ctx.rxr.rxr_debug_ray_accel_nodes(ctx.ctx, None, 0, C.byref(n)) == RXR_OK, ctx.error()
    flat = np.zeros((n.value, 8), F)
    assert ctx.rxr.rxr_debug_ray_accel_nodes(ctx.ctx, flat.ctypes.data_as(C.POINTER(C.c_float)), n.value, C.byref(n)) == RXR_OK, ctx.error()
    return V.split_nodes(flat, ntri)


@pytest.mark.parametrize("ntri", (65, 4097))
def test_the_count_is_the_restated_walks(pick, ntri):
    """RXR_RAY_ACCEL_INFO_TESTS covers this route: the sum over the rays of the positions tests/ray_wave_ref.py: wave_walk tests, its
    passes the restated box test over the device's own nodes -- the same float operations, so exactly; half the rays point away from
    everything, so the count is below rays x triangles"""
    meshes, o, d, _ = sized_scene(ntri)
    o, d = o[:120].copy(), d[:120].copy()
    centre = meshes[0]["vertices"][:, :3].mean(axis=0)
    d[::2] = o[::2] - centre
    register(pick, meshes, ("sized", ntri))
    wave_and_off(pick, meshes, o, d, f"counted, {ntri} triangles", accel=COUNT)
    assert set_accel(pick, COUNT) == RXR_OK and set_wave(pick, W_FORCE) == RXR_OK
    pick.intersect(o, d)
    tests = accel_info(pick)["tests"]
    nodes = device_nodes(pick, ntri)
    assert set_accel(pick, OFF) == RXR_OK and set_wave(pick, W_OFF) == RXR_OK
    with np.errstate(all="ignore"):
        dn = R.normalized(d)
    want = 0
    for r in range(len(o)):
        if not A.ray_dead(o[r], dn[r]):
            want += len(V.wave_walk(ntri, V.passes_of(nodes, o[r], dn[r]))[0])
    print(f"{ntri} triangles, {len(o)} rays: {tests} ray-triangle tests counted, {want} restated, {len(o) * ntri} brute force")
    assert tests == want
    if ntri > 64:
        assert tests < len(o) * ntri


# ---- after mesh updates --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("refresh", (T.RAY_REFRESH_FULL, T.RAY_REFRESH_RANGED))
def test_after_rxr_update_meshes(pick, refresh):
    a, b, c = M.grid_mesh(60, 100, 1), M.grid_mesh(50, 80, 2, lst=R.LIST_DYNAMIC), M.grid_mesh(40, 30, 3, lst=R.LIST_OVERLAY)
    for m in (a, b, c):
        m.update(chunk=-1, has_pid=False, pid=0)
    meshes = [a, b, c]
    assert set_refresh(pick, refresh) == RXR_OK
    try:
        register(pick, meshes)
        rng = np.random.default_rng(21)
        o, d = aimed(meshes, (0.0, 0.0, 1.0), rng, 300)
        wave_and_off(pick, meshes, o, d, "before the update", ref=R.intersect_many(meshes, o, d, full=True))
        assert set_accel(pick, ON) == RXR_OK      # (under _RANGED a standing tree is refitted only while the mode is on)
        pick.intersect(o, d)
        moved = [a, M.moved(b, 3), c]
        counts, v, idx, nr = M.pack([moved[1]])
        named = np.array([1], np.uint32)
        rc = pick.rxr.rxr_update_meshes(pick.ctx, named.ctypes.data, 1, counts.ctypes.data, v.ctypes.data, idx.ctypes.data, nr.ctypes.data, v.shape[1], idx.shape[1])
        assert rc == RXR_OK, pick.error()
        o2, d2 = aimed(moved, (0.0, 0.0, 1.0), rng, 300)
        ref = R.intersect_many(moved, o2, d2, full=True)
        assert set_wave(pick, W_FORCE) == RXR_OK
        w0 = wave_info(pick)
        first = pick.intersect(o2, d2, full=True)         # the query that rebuilds or refits walks the new tree a wave per ray
        assert wave_info(pick)["batches"] == w0["batches"] + 1
        bad = P.differences(first, ref, "the first query after the update:")
        assert bad is None, bad
        out = (C.c_uint64 * len(T.RAY_REFRESH_VERIFY))()
        assert pick.rxr.rxr_ray_refresh_verify(pick.ctx, out) == RXR_OK, pick.error()
        v = dict(zip(T.RAY_REFRESH_VERIFY, (int(x) for x in out)))
        assert (v["pick_words"], v["sorted_words"], v["nodes"], v["checked"]) == (0, 0, 0, 3), v
        wave_and_off(pick, moved, o2, d2, "after the update", ref=ref)
        assert (ref["mesh"] != R.MISS).sum() > 50
    finally:
        register(pick, [])
        assert set_refresh(pick, T.RAY_REFRESH_FULL) == RXR_OK and set_accel(pick, OFF) == RXR_OK and set_wave(pick, W_OFF) == RXR_OK


# ---- the path tracer -------------------------------------------------------------------------------------------------------------
def grid_in_the_room():
    """4 097 triangles hanging in the tests' room, in view of its camera"""
    g = grid(4097, 91)
    v = g["vertices"].copy()
    v[:, :3] = (v[:, :3] - v[:, :3].mean(axis=0)) * F(0.6) + np.array([4.0, 2.0, 4.5], F)
    return T.mesh(v, g["indices"], g["uvs"], g["normals"], source=S.PIXEL(90, 140, 220), material=S.MATTE_1)


@pytest.mark.parametrize("which", ("room", "grid"))
def test_trace_three_frames_of_eight_bounces(tracer, which):
    scene = S.diffuse_room() if which == "room" else S.room(material=S.MATTE_1, lights=[S.point_light((4.0, 3.0, 3.0), intensity=1.5)],
                                                          box_source=S.PIXEL(180, 160, 90), extra=[grid_in_the_room()])
    w, h, bounces, frames = 16, 9, 8, 3
    S.load(tracer, scene)
    cam = S.cameras(w, h)["firstp"]
    out = {}
    try:
        for accel, wave in ((OFF, W_OFF), (ON, W_OFF), (ON, W_FORCE), (OFF, W_FORCE)):
            tracer.ray_accel, tracer.ray_wave = accel, wave
            acc = T.AccumBuffer(w, h)
            w0, a0 = tracer.ray_wave_info(), tracer.ray_accel_info()
            tracer.trace(cam, acc, n_frames=frames, seed=5, bounces=bounces)
            w1, a1 = tracer.ray_wave_info(), tracer.ray_accel_info()
            out[accel, wave] = acc.pixels.copy()
            by_wave = accel == ON and wave == W_FORCE          # (with the accel mode off the switch does nothing)
            assert w1["batches"] - w0["batches"] == (frames * bounces if by_wave else 0), (which, accel, wave, w0, w1)
            assert w1["rays"] - w0["rays"] == (frames * bounces * w * h if by_wave else 0)
            assert a1["batches"] - a0["batches"] == (frames * bounces if (accel, wave) == (ON, W_OFF) else 0)
    finally:
        tracer.ray_accel, tracer.ray_wave = OFF, W_OFF
    base = out[OFF, W_OFF].view(np.uint32)
    for key, px in out.items():
        bits = px.view(np.uint32) == base
        assert bits.all(), f"{which}, accel {key[0]}, wave {key[1]}: {int((~bits).sum())} floats differ from the trace with both switches off"
    assert (out[OFF, W_OFF][..., :3] > 0).any() and len(np.unique(out[OFF, W_OFF][..., 0])) > 8


# ---- defaults, refusals, the rule ------------------------------------------------------------------------------------------------
def test_defaults_and_refusals():
    with P.PickContext() as ctx:
        assert wave_info(ctx) == dict(mode=W_OFF, batches=0, rays=0)
        assert set_wave(ctx, W_ON) == RXR_OK and wave_info(ctx)["mode"] == W_ON
        assert set_wave(ctx, 3) == RXR_ERR_INVALID and "rxr_set_ray_wave" in ctx.error()
        assert set_wave(ctx, 0xFFFFFFFF) == RXR_ERR_INVALID
        assert wave_info(ctx) == dict(mode=W_ON, batches=0, rays=0)
        assert set_accel(ctx, 3) == RXR_ERR_INVALID and "rxr_set_ray_accel" in ctx.error()     # (the accel switch keeps refusing mode 3)
        assert ctx.rxr.rxr_ray_wave_info(ctx.ctx, None) == RXR_ERR_INVALID and "rxr_ray_wave_info" in ctx.error()
        # with the accel mode off, FORCE sends nothing to the kernel and builds no tree
        meshes = [grid(100, 95)]
        ctx.set_meshes(meshes)
        o, d = aimed(meshes, (0.5, 7.0, 3.0), np.random.default_rng(96), 300)
        ref = R.intersect_many(meshes, o, d, full=True)
        assert set_wave(ctx, W_FORCE) == RXR_OK
        for n in (1, 64, 65, 300):
            assert P.differences(ctx.intersect(o[:n], d[:n], full=True), P.prefix(ref, n), f"accel off, FORCE, {n} rays:") is None
        assert wave_info(ctx) == dict(mode=W_FORCE, batches=0, rays=0) and accel_info(ctx)["builds"] == 0
        # under _ON a 64-ray batch on a 100-triangle scene takes neither tree route, and 65 rays take the thread walk as before
        assert set_accel(ctx, ON) == RXR_OK and set_wave(ctx, W_ON) == RXR_OK
        assert not V.takes(64, 100) and not V.takes(65, 100)
        assert P.differences(ctx.intersect(o[:64], d[:64], full=True), P.prefix(ref, 64), "ON, 64 rays:") is None
        assert wave_info(ctx)["batches"] == 0 and accel_info(ctx)["batches"] == 0
        assert P.differences(ctx.intersect(o[:65], d[:65], full=True), P.prefix(ref, 65), "ON, 65 rays:") is None
        assert wave_info(ctx)["batches"] == 0 and accel_info(ctx)["batches"] == 1


def test_under_on_the_rule_decides(pick):
    """32 769 triangles: batches that rxr_ray_wave_takes names go a wave per ray, the others as before"""
    ntri = 32769
    meshes, o, d, _ = sized_scene(ntri)
    register(pick, meshes, ("sized", ntri))
    reps = np.arange(4096) % len(o)
    o, d = o[reps], d[reps]
    assert set_accel(pick, OFF) == RXR_OK and set_wave(pick, W_OFF) == RXR_OK
    off = pick.intersect(o, d, full=True)
    assert set_accel(pick, ON) == RXR_OK and set_wave(pick, W_ON) == RXR_OK
    try:
        for n in (1, 64, 300, 4096):
            w0, a0 = wave_info(pick), accel_info(pick)
            got = pick.intersect(o[:n], d[:n], full=True)
            w1, a1 = wave_info(pick), accel_info(pick)
            by_wave = bool(pick.rxr.rxr_ray_wave_takes(n, ntri))
            assert by_wave == V.takes(n, ntri)
            assert (w1["batches"] - w0["batches"], w1["rays"] - w0["rays"]) == ((1, n) if by_wave else (0, 0)), (n, w0, w1)
            assert a1["batches"] - a0["batches"] == (1 if n > 64 and not by_wave else 0), (n, a0, a1)
            assert P.differences(got, P.prefix(off, n), f"ON, {n} rays:") is None
    finally:
        assert set_accel(pick, OFF) == RXR_OK and set_wave(pick, W_OFF) == RXR_OK


def test_scene_ray_wave_through_the_mirror(product):
    """Scene.ray_wave is handed to the context next to Scene.ray_accel: the same picks, and the info shows the batch"""
    meshes = [grid(600, 61), grid(50, 62, list=R.LIST_OVERLAY)]
    scene = P.host_scene(product, meshes)
    o, d = aimed(meshes, (0.3, 6.0, 2.0), np.random.default_rng(15), 200)
    ref = R.intersect_many(meshes, o, d, full=True)
    try:
        assert scene.ray_wave == W_OFF
        scene.ray_accel, scene.ray_wave = ON, W_FORCE
        w0, a0 = scene.ray_wave_info(), scene.ray_accel_info()
        got = scene.intersect(o, d, full=True)
        w1, a1 = scene.ray_wave_info(), scene.ray_accel_info()
        assert (w1["mode"], w1["batches"] - w0["batches"], w1["rays"] - w0["rays"]) == (W_FORCE, 1, 200) and a1["batches"] == a0["batches"]
        assert P.differences(got, ref, "the mirror:") is None
    finally:
        scene.ray_accel, scene.ray_wave = OFF, W_OFF
        scene.intersect(o[:1], d[:1])    # (hands the defaults back to the shared context)
