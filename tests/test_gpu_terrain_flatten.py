"""Flattened terrain heights on the device (rxr_set_terrain_flatten, rxr_flatten_terrain / rxr_flatten_terrain_to,
rxr_set_terrain_height_source: the Height pass of TerrainChunk::process_batch_modifiers) against the dictionary transcription of
tests/terrain_flatten_ref.py: every height word and every presence byte equal, a NaN where the reference has one, nothing left out.
Every call's arrays are filled with a sentinel first and carry a guard behind the last chunk, which must come back unchanged.

The cases are those of tests/terrain_flatten_ref.py (their answers computed once and shared with the CPU suite): chunk sizes on both
sides of a wave of cells and of a round of 256, the bound; active op counts around the ballot rounds with inactive sectors in
between; edge and segment counts around a round; order, presence and every quirk the header keeps; two fuzz scenes."""
import ctypes as C

import numpy as np
import pytest

import rusterix_amd
from rusterix_amd import binding as B
from rusterix_amd.abi import (RXR_ERR_INVALID, RXR_ERR_UNSUPPORTED, RXR_OK, RXR_TERRAIN_HEIGHTS_PROCESSED as PROCESSED,
                              RXR_TERRAIN_HEIGHTS_REGISTERED as REGISTERED)
from tests import terrain_flatten_ref as R
from tests.terrain_flatten_ref import F
from tests.terrain_hit_ref import HeightSpec

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5C3F00D
GUARD = 64
LAUNCH_CHUNKS = 256            # rxr_terrain_flatten.hip FLATTEN_LAUNCH_CHUNKS


def last_error(rxr, ctx):
    return (rxr.rxr_last_error(ctx) or b"").decode()


def set_heights(rxr, ctx, spec):
    keep, args = spec.arrays()
    return rxr.rxr_set_terrain_heights(ctx, *args)


def set_ops(rxr, ctx, sc):
    keep, args = sc.arrays()
    return rxr.rxr_set_terrain_flatten(ctx, *args)


def register(rxr, ctx, sc):
    assert set_heights(rxr, ctx, sc.spec) == RXR_OK, last_error(rxr, ctx)
    assert set_ops(rxr, ctx, sc) == RXR_OK, last_error(rxr, ctx)


def flatten(rxr, ctx, coords, cs, want_rc=RXR_OK):
    """rxr_flatten_terrain into sentinel-filled arrays: (heights [n][cs * cs], present) after the guards were checked"""
    cc = np.ascontiguousarray(np.asarray(coords, np.int32).reshape(-1, 2))
    n, per = len(cc), cs * cs
    h = np.full(n * per + GUARD, SENTINEL, np.uint32)
    p = np.full(n * per + GUARD, 0xA5, np.uint8)
    rc = rxr.rxr_flatten_terrain(ctx, cc.ctypes.data, n, cs, h.ctypes.data, p.ctypes.data)
    assert rc == want_rc, last_error(rxr, ctx)
    assert (h[n * per:] == SENTINEL).all() and (p[n * per:] == 0xA5).all(), "guard"
    if rc != RXR_OK:
        assert (h == SENTINEL).all() and (p == 0xA5).all(), "a refused call wrote"
    return h[: n * per].view(F).reshape(n, per), p[: n * per].reshape(n, per)


def expect(got, want, label):
    heights, present = got
    assert len(heights) == len(want), label
    for i, w in enumerate(want):
        d = R.first_difference(heights[i], present[i], *w)
        assert not d, f"{label} chunk {i}: {d}"


@pytest.fixture()
def dev(product):
    """the mirror's context, left as it was found: no flatten ops, the registered heights as the source"""
    rxr, ctx = rusterix_amd.rxr_abi(), C.c_void_p(product.lib.rxh_context())
    yield rxr, ctx
    assert rxr.rxr_set_terrain_height_source(ctx, REGISTERED) == RXR_OK
    assert rxr.rxr_set_terrain_flatten(ctx, None, None, None, 0, None, 0) == RXR_OK


@pytest.fixture()
def own():
    """a context of its own"""
    rxr, ctx = rusterix_amd.rxr_abi(), C.c_void_p()
    assert rxr.rxr_create(C.byref(ctx), 0) == RXR_OK
    yield rxr, ctx
    rxr.rxr_destroy(ctx)


# ---- every case ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_every_case_equals_the_transcription(dev, name):
    rxr, ctx = dev
    sc, coords, want = R.case(name)
    register(rxr, ctx, sc)
    cs = sc.spec.chunk_size
    expect(flatten(rxr, ctx, coords, cs), want, name)
    assert rxr.rxr_debug_terrain_flatten_launches(ctx) == 1
    # one chunk alone gives the same words as in the company of the others, and so does the reverse order
    last = len(coords) - 1
    expect(flatten(rxr, ctx, [coords[last]], cs), [want[last]], name + " alone")
    expect(flatten(rxr, ctx, coords[::-1], cs), want[::-1], name + " reversed")


def test_no_ops_copies_the_registered_cells(dev):
    rxr, ctx = dev
    sc, coords, _ = R.case("untouched_chunk")
    assert set_heights(rxr, ctx, sc.spec) == RXR_OK
    assert rxr.rxr_set_terrain_flatten(ctx, None, None, None, 0, None, 0) == RXR_OK
    plain = R.FlattenScene(sc.spec.scale, 8)
    plain.spec = sc.spec
    expect(flatten(rxr, ctx, coords + [(9, 9)], 8), [plain.dense(c) for c in coords + [(9, 9)]], "no ops")
    # either output may be left out
    cc = np.asarray(coords, np.int32)
    h = np.zeros(2 * 64, F)
    p = np.zeros(2 * 64, np.uint8)
    assert rxr.rxr_flatten_terrain(ctx, cc.ctypes.data, 2, 8, h.ctypes.data, None) == RXR_OK
    assert rxr.rxr_flatten_terrain(ctx, cc.ctypes.data, 2, 8, None, p.ctypes.data) == RXR_OK
    assert rxr.rxr_flatten_terrain(ctx, cc.ctypes.data, 2, 8, None, None) == RXR_OK
    expect((h.reshape(2, 64), p.reshape(2, 64)), [plain.dense(c) for c in coords], "one array at a time")


# ---- launches --------------------------------------------------------------------------------------------------------------------------
def test_a_forced_launch_split_gives_the_same_words(dev, monkeypatch):
    rxr, ctx = dev
    sc, coords, want = R.case("fuzz_1")
    register(rxr, ctx, sc)
    monkeypatch.setenv("RXR_TERRAIN_FLATTEN_LAUNCH_CHUNKS", "1")
    expect(flatten(rxr, ctx, coords, 8), want, "a chunk a launch")
    assert rxr.rxr_debug_terrain_flatten_launches(ctx) == len(coords)
    monkeypatch.setenv("RXR_TERRAIN_FLATTEN_LAUNCH_CHUNKS", "4")
    expect(flatten(rxr, ctx, coords, 8), want, "four chunks a launch")
    assert rxr.rxr_debug_terrain_flatten_launches(ctx) == 3
    monkeypatch.setenv("RXR_TERRAIN_FLATTEN_LAUNCH_CHUNKS", "100000")        # the variable lowers the bound, never raises it
    expect(flatten(rxr, ctx, coords, 8), want, "one launch")
    assert rxr.rxr_debug_terrain_flatten_launches(ctx) == 1


def test_more_chunks_than_one_launch_takes(dev):
    rxr, ctx = dev
    cs, n = 2, LAUNCH_CHUNKS + 44
    coords = [(k % 20 - 10, k // 20 - 7) for k in range(n)]
    sc = R.fill(R.FlattenScene((1.0, 1.5), cs), coords, density=0.8, seed=21)
    sc.sector(R.polygon(0.0, 1.0, 9.0, 5), bevel=2.0, floor_height=1.0)
    sc.linedefs([(-19.0, -13.0, 18.0, 12.0, 0.0, 3.0)], bevel=1.5)
    register(rxr, ctx, sc)
    expect(flatten(rxr, ctx, coords, cs), [sc.dense(c) for c in coords], "300 chunks")
    assert rxr.rxr_debug_terrain_flatten_launches(ctx) == 2


# ---- the processed grid and its readers ------------------------------------------------------------------------------------------------
def mesh_words(rxr, ctx, coords, cs):
    from tests.test_gpu_terrain_mesh import meshes

    return meshes(rxr, ctx, coords, cs)


def hit_words(rxr, ctx, o, d, md):
    from tests.test_gpu_terrain_hit import hits

    return hits(rxr, ctx, o, d, md)


def rays(sc, coords, n=200, seed=5):
    rng = np.random.default_rng(seed)
    cs = sc.spec.chunk_size
    xs = [c[0] * cs for c in coords] + [c[0] * cs + cs for c in coords]
    ys = [c[1] * cs for c in coords] + [c[1] * cs + cs for c in coords]
    o = np.stack([rng.uniform(min(xs) - 1, max(xs) + 1, n), rng.uniform(4.0, 9.0, n), rng.uniform(min(ys) - 1, max(ys) + 1, n)], axis=1).astype(F)
    d = np.stack([rng.uniform(-0.5, 0.5, n), rng.uniform(-1.0, -0.3, n), rng.uniform(-0.5, 0.5, n)], axis=1).astype(F)
    return np.ascontiguousarray(o), np.ascontiguousarray(d), 40.0


def same_meshes(a, b):
    from tests import terrain_mesh_ref as M

    return len(a) == len(b) and not any(M.first_difference(x, y, nan_as_nan=True) for x, y in zip(a, b))


def same_hits(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in a)


def test_the_processed_source_equals_a_context_registered_with_the_processed_heights(dev, own):
    """meshes and picks under RXR_TERRAIN_HEIGHTS_PROCESSED against a second context that never flattened and was handed the
    transcription's processed_heights by the host: every word.  Under _REGISTERED a flatten changes nothing; a registration resets
    the processed grid."""
    rxr, ctx = dev
    _, host = own
    sc, coords, want = R.case("road_over_sector")
    cs = sc.spec.chunk_size
    o, d, md = rays(sc, coords)
    register(rxr, ctx, sc)
    assert set_heights(rxr, host, sc.spec) == RXR_OK
    never_m, never_h = mesh_words(rxr, host, coords, cs), hit_words(rxr, host, o, d, md)
    expect(flatten(rxr, ctx, coords, cs), want, "the flatten")
    # REGISTERED (the default): as if nothing had been flattened
    assert same_meshes(mesh_words(rxr, ctx, coords, cs), never_m) and same_hits(hit_words(rxr, ctx, o, d, md), never_h)
    # PROCESSED: the host's processed_heights
    assert set_heights(rxr, host, sc.processed_spec(coords)) == RXR_OK
    host_m, host_h = mesh_words(rxr, host, coords, cs), hit_words(rxr, host, o, d, md)
    assert not same_meshes(host_m, never_m) and not same_hits(host_h, never_h), "the ops should show"
    assert rxr.rxr_set_terrain_height_source(ctx, PROCESSED) == RXR_OK
    assert same_meshes(mesh_words(rxr, ctx, coords, cs), host_m) and same_hits(hit_words(rxr, ctx, o, d, md), host_h)
    # only chunk (1, 0) flattened after a new registration: chunk (0, 0) of the processed grid is the registered cells again
    assert set_heights(rxr, ctx, sc.spec) == RXR_OK
    assert same_meshes(mesh_words(rxr, ctx, coords, cs), never_m), "a registration resets the processed grid"
    expect(flatten(rxr, ctx, coords[1:], cs), want[1:], "one chunk")
    assert set_heights(rxr, host, sc.processed_spec(coords[1:])) == RXR_OK
    assert same_meshes(mesh_words(rxr, ctx, coords, cs), mesh_words(rxr, host, coords, cs))
    assert same_hits(hit_words(rxr, ctx, o, d, md), hit_words(rxr, host, o, d, md))
    # the source stays across a registration, and anything but the two values is refused
    assert rxr.rxr_set_terrain_height_source(ctx, 2) == RXR_ERR_INVALID and "rxr_set_terrain_height_source" in last_error(rxr, ctx)
    assert rxr.rxr_set_terrain_height_source(ctx, REGISTERED) == RXR_OK
    assert same_meshes(mesh_words(rxr, ctx, coords, cs), never_m)


def test_to_form_then_a_mesh_build_on_the_callers_stream(own):
    """rxr_flatten_terrain_to on a stream of the caller's, at once rxr_terrain_meshes_to behind it on that stream under
    _PROCESSED, at once a pick on ANOTHER stream: the blocking forms' words"""
    import torch

    from tests.test_gpu_terrain_mesh import to_buffers, to_host, unpack

    rxr, ctx = own
    sc, coords, want = R.case("size_9")
    cs, n = 9, len(coords)
    o, d, md = rays(sc, coords, n=64)
    register(rxr, ctx, sc)
    assert rxr.rxr_set_terrain_height_source(ctx, PROCESSED) == RXR_OK
    cc = np.ascontiguousarray(np.asarray(coords, np.int32))
    s, other = torch.cuda.Stream(), torch.cuda.Stream()
    dh = torch.full((n * cs * cs + GUARD,), -7.0, dtype=torch.float32, device="cuda")
    dp = torch.full((n * cs * cs + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    buf = to_buffers(n, cs)
    do, dd = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    hit = torch.zeros(64, dtype=torch.int32, device="cuda")
    wp = torch.zeros((64, 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    assert rxr.rxr_flatten_terrain_to(ctx, cc.ctypes.data, n, cs, dh.data_ptr(), dp.data_ptr(), C.c_void_p(s.cuda_stream)) == RXR_OK, last_error(rxr, ctx)
    rc = rxr.rxr_terrain_meshes_to(ctx, cc.ctypes.data, n, cs, *(buf[k].data_ptr() for k in ("counts", "vertices", "indices", "normals")), C.c_void_p(s.cuda_stream))
    assert rc == RXR_OK, last_error(rxr, ctx)
    assert rxr.rxr_terrain_hits_to(ctx, do.data_ptr(), dd.data_ptr(), 64, md, hit.data_ptr(), None, wp.data_ptr(), None, C.c_void_p(other.cuda_stream)) == RXR_OK
    cc[:] = 12345                                                # (the coordinates were read before the calls returned)
    s.synchronize()
    other.synchronize()
    gh, gp = dh.cpu().numpy(), dp.cpu().numpy()
    assert (gh[n * cs * cs:] == -7.0).all() and (gp[n * cs * cs:] == 0xA5).all(), "guard"
    expect((gh[: n * cs * cs].reshape(n, -1), gp[: n * cs * cs].reshape(n, -1)), want, "_to")
    streamed = unpack(to_host(buf), n, cs)
    expect(flatten(rxr, ctx, coords, cs), want, "blocking")
    assert same_meshes(streamed, mesh_words(rxr, ctx, coords, cs))
    blocking_hits = hit_words(rxr, ctx, o, d, md)
    assert hit.cpu().numpy().view(np.uint32).tobytes() == blocking_hits["hit"].tobytes()
    assert wp.cpu().numpy().tobytes() == blocking_hits["world_pos"].tobytes()
    # ... and a context the host registered with the processed heights
    rxr2, host = rusterix_amd.rxr_abi(), C.c_void_p()
    assert rxr2.rxr_create(C.byref(host), 0) == RXR_OK
    try:
        assert set_heights(rxr2, host, sc.processed_spec(coords)) == RXR_OK
        assert same_meshes(streamed, mesh_words(rxr2, host, coords, cs))
    finally:
        rxr2.rxr_destroy(host)
    # the default stream; without outputs; host memory where device memory is expected; a misaligned pointer
    coords_again = np.ascontiguousarray(np.asarray(coords, np.int32))
    assert rxr.rxr_flatten_terrain_to(ctx, coords_again.ctypes.data, n, cs, None, None, None) == RXR_OK
    assert rxr.rxr_synchronize(ctx) == RXR_OK
    host_h = np.zeros(n * cs * cs, F)
    assert rxr.rxr_flatten_terrain_to(ctx, coords_again.ctypes.data, n, cs, host_h.ctypes.data, None, None) == RXR_ERR_INVALID and "dev_heights" in last_error(rxr, ctx)
    assert rxr.rxr_flatten_terrain_to(ctx, coords_again.ctypes.data, n, cs, None, host_h.ctypes.data, None) == RXR_ERR_INVALID and "dev_present" in last_error(rxr, ctx)
    assert rxr.rxr_flatten_terrain_to(ctx, coords_again.ctypes.data, n, cs, dh.data_ptr() + 2, None, None) == RXR_ERR_INVALID and "aligned" in last_error(rxr, ctx)
    assert rxr.rxr_synchronize(ctx) == RXR_OK and not host_h.any()


# ---- lifetime, refusals, handles -------------------------------------------------------------------------------------------------------
def test_registration_lifetime(dev):
    """the arrays are read before the call returns; the list outlives a registration of heights; a refused list leaves the resident
    one as it was; n_ops == 0 clears it"""
    rxr, ctx = dev
    sc, coords, want = R.case("two_nodes_on_one_sector")
    assert set_heights(rxr, ctx, sc.spec) == RXR_OK
    keep, args = sc.arrays()
    assert rxr.rxr_set_terrain_flatten(ctx, *args) == RXR_OK, last_error(rxr, ctx)
    for a in keep.values():
        a.view(np.uint8)[:] = 0xFF
    expect(flatten(rxr, ctx, coords, 8), want, "after the arrays were overwritten")
    assert set_heights(rxr, ctx, HeightSpec((1.0, 1.0), 8).height(100, 100, 1.0)) == RXR_OK
    assert set_heights(rxr, ctx, sc.spec) == RXR_OK
    expect(flatten(rxr, ctx, coords, 8), want, "after other heights")
    bad = np.array([9], np.uint32)
    keep, args = sc.arrays()
    assert rxr.rxr_set_terrain_flatten(ctx, bad.ctypes.data, *args[1:]) == RXR_ERR_INVALID and "kind 9" in last_error(rxr, ctx)
    rg = keep["ranges"].copy()
    rg[1] = (0, len(keep["records"]) + 1)
    assert rxr.rxr_set_terrain_flatten(ctx, args[0], args[1], rg.ctypes.data, *args[3:]) == RXR_ERR_INVALID and "range" in last_error(rxr, ctx)
    assert rxr.rxr_set_terrain_flatten(ctx, args[0], args[1], args[2], rusterix_amd.abi.RXR_TERRAIN_FLATTEN_MAX_OPS + 1, args[4], args[5]) == RXR_ERR_UNSUPPORTED
    expect(flatten(rxr, ctx, coords, 8), want, "after refused lists")
    assert rxr.rxr_set_terrain_flatten(ctx, None, None, None, 0, None, 0) == RXR_OK
    plain = R.FlattenScene((1.0, 1.0), 8)
    plain.spec = sc.spec
    expect(flatten(rxr, ctx, coords, 8), [plain.dense(c) for c in coords], "cleared")


def test_refusals_queue_nothing(dev, own):
    rxr, fresh = own
    zero = [(0, 0)]
    got = flatten(rxr, fresh, zero, 4, RXR_ERR_INVALID)
    assert "no terrain heights" in last_error(rxr, fresh)
    sc, coords, want = R.case("overlap_first_order")
    register(rxr, fresh, sc)
    expect(flatten(rxr, fresh, coords, 8), want, "first")
    assert rxr.rxr_debug_terrain_flatten_launches(fresh) == 1
    for cs, rc, word in ((0, RXR_ERR_INVALID, "chunk_size"), (-3, RXR_ERR_INVALID, "chunk_size"), (65, RXR_ERR_UNSUPPORTED, "RXR_TERRAIN_MESH_MAX_CHUNK_SIZE")):
        h = np.full(65 * 65, SENTINEL, np.uint32)
        cc = np.zeros((1, 2), np.int32)
        assert rxr.rxr_flatten_terrain(fresh, cc.ctypes.data, 1, cs, h.ctypes.data, None) == rc and word in last_error(rxr, fresh)
        assert (h == SENTINEL).all()
    for bad in ([2 ** 28, 0], [0, -(2 ** 28) - 1], [2 ** 31 - 1, 0]):
        flatten(rxr, fresh, [[0, 0], bad], 4, RXR_ERR_INVALID)
        assert "2^30" in last_error(rxr, fresh), bad
    flatten(rxr, fresh, [(0, 0), (1, 0), (0, 0)], 8, RXR_ERR_INVALID)
    assert "named twice" in last_error(rxr, fresh) and "chunk 2" in last_error(rxr, fresh)
    assert rxr.rxr_flatten_terrain(fresh, None, 1, 8, None, None) == RXR_ERR_INVALID and "chunk_coords" in last_error(rxr, fresh)
    assert rxr.rxr_flatten_terrain(fresh, None, 0, 8, None, None) == RXR_OK                    # n == 0 does nothing
    assert rxr.rxr_debug_terrain_flatten_launches(fresh) == 1, "a refused call launched"
    # the processed grid is what the first call left: the refused ones wrote nothing
    assert rxr.rxr_set_terrain_height_source(fresh, PROCESSED) == RXR_OK
    rxr2, host = dev
    assert set_heights(rxr2, host, sc.processed_spec(coords)) == RXR_OK
    assert same_meshes(mesh_words(rxr, fresh, coords, 8), mesh_words(rxr2, host, coords, 8))
    edge = [(2 ** 28 - 1, -(2 ** 28))]                                                      # the last chunk before +2^30
    h, p = flatten(rxr, fresh, edge, 4)
    assert not p.any() and not h.any()


def test_multi_device_handles(own):
    rxr, _ = own
    sc, coords, want = R.case("overlap_other_order")
    multi = C.c_void_p()
    devs = (C.c_int * 2)(0, 0)
    assert rxr.rxr_create_multi(C.byref(multi), devs, 2) == RXR_OK
    try:
        flatten(rxr, multi, coords, 8, RXR_ERR_INVALID)
        assert "no terrain heights" in last_error(rxr, multi)
        register(rxr, multi, sc)
        expect(flatten(rxr, multi, coords, 8), want, "member 0")
        assert rxr.rxr_debug_terrain_flatten_launches(multi) == 1
        cc = np.asarray(coords, np.int32)
        assert rxr.rxr_flatten_terrain_to(multi, cc.ctypes.data, 1, 8, None, None, None) == RXR_ERR_UNSUPPORTED and "multi-device" in last_error(rxr, multi)
        assert rxr.rxr_set_terrain_height_source(multi, PROCESSED) == RXR_OK
        assert rxr.rxr_set_terrain_height_source(multi, 7) == RXR_ERR_INVALID and "rxr_set_terrain_height_source" in last_error(rxr, multi)
        bad = np.array([3], np.uint32)
        keep, args = sc.arrays()
        assert rxr.rxr_set_terrain_flatten(multi, bad.ctypes.data, *args[1:]) == RXR_ERR_INVALID and "kind 3" in last_error(rxr, multi)
    finally:
        rxr.rxr_destroy(multi)


# ---- through the mirror ----------------------------------------------------------------------------------------------------------------
def test_the_mirror_registers_ops_and_heights_only_when_they_changed(product):
    sc, coords, want = R.case("fuzz_2")
    t = sc.product(product)
    h0, f0 = t.registrations()
    expect(t.process_heights(coords), want, "the device form")
    assert t.registrations() == (h0 + 1, f0 + 1)
    expect(t.process_heights(coords[:2]), want[:2], "again")
    expect(t.process_heights_cpu(coords), want, "the CPU form")
    assert t.registrations() == (h0 + 1, f0 + 1), "unchanged heights and ops were registered again"
    x, y = sorted(sc.spec.heights)[0]
    t.set_height(x, y, 7.5)
    t.process_heights(coords[:1])
    assert t.registrations() == (h0 + 2, f0 + 1)
    keep, _ = sc.arrays()
    t.set_flatten_ops(keep["kinds"][:1], keep["params"][:1], keep["ranges"][:1], keep["records"])
    one = R.FlattenScene(sc.spec.scale, sc.spec.chunk_size)
    one.spec.heights = dict(sc.spec.heights)
    one.spec.height(x, y, 7.5)
    one.ops = sc.ops[:1]
    expect(t.process_heights(coords), [one.dense(c) for c in coords], "one op, one edit")
    assert t.registrations() == (h0 + 2, f0 + 2)
    with pytest.raises(B.RasterizeError) as e:
        sc.product(product).process_heights([(0, 0), (0, 0)])
    assert e.value.code == RXR_ERR_INVALID


CS = 16
COORDS = [(0, 0), (1, 0), (0, 1), (1, 1)]
W, H = 256, 160


def chain_scene(api, terrain):
    """four chunks of 16 with one terrain_batch3d each, built by `terrain`; returns (scene, render)"""
    scene = api.Scene.empty()
    for k, mesh in enumerate(terrain.build_meshes(COORDS)):
        scene.add_chunk().terrain_batch3d(mesh.source(B.PixelSource.Pixel((40 + 50 * k, 200 - 40 * k, 90, 255))))
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

    return scene, render


def chain_case(edits=()):
    sc = R.fill(R.FlattenScene((1.0, 1.0), CS), COORDS, seed=31)
    for (x, y), dh in edits:
        sc.height(x, y, sc.spec.heights[(x, y)] + F(dh))
    sc.sector(R.polygon(22.0, 7.0, 5.0, 6), bevel=1.5, floor_height=2.0)
    sc.linedefs([(2.0, 3.0, 29.0, 12.0, 0.5, 1.5), (29.0, 12.0, 12.0, 30.0, 1.5, 0.0)], bevel=1.5)
    return sc


def test_a_height_stroke_through_the_chain_under_device_modifiers(product):
    """flatten -> meshes -> update through Scene::rebuild_terrain_meshes with Terrain::device_modifiers, against a scene the host
    registered with the transcription's processed heights: the same frame"""
    api = product
    stroke = [((x, y), 2.5) for y in range(3, 9) for x in range(18, 26)]                       # chunk (1, 0) only, no cell added
    api.lib.rxh_set_device_projection(1)
    try:
        before, after = chain_case(), chain_case(stroke)
        # the host's route: processed_heights registered as plain heights, every chunk built from them
        want_first = chain_scene(api, before.processed_spec(COORDS).product(api))[1]()
        want = chain_scene(api, after.processed_spec(COORDS).product(api))[1]()
        assert want.tobytes() != want_first.tobytes(), "the stroke should show"
        t = before.product(api).set_device_modifiers(True)
        scene, render = chain_scene(api, t)
        assert render().tobytes() == want_first.tobytes(), "build_meshes under device_modifiers"
        for (x, y), dh in stroke:
            t.set_height(x, y, float(after.spec.heights[(x, y)]))
        assert scene.rebuild_terrain_meshes(t, [(1, 0)], [1]) == 0
        got = render()
        assert got.tobytes() == want.tobytes(), int((got != want).any(axis=2).sum())
        # the option off: the registered heights, as before this feature
        t.set_device_modifiers(False)
        assert scene.rebuild_terrain_meshes(t, [(1, 0)], [1]) == 0
        render()
        plain_scene, plain_render = chain_scene(api, after.spec.product(api))
        rxr = rusterix_amd.rxr_abi()
        lo, hi, lo2, hi2 = (C.c_float * 3)(), (C.c_float * 3)(), (C.c_float * 3)(), (C.c_float * 3)()
        assert rxr.rxr_mesh_bounds(api.lib.rxh_context(), 1, lo, hi) == RXR_OK
        plain_render()
        assert rxr.rxr_mesh_bounds(api.lib.rxh_context(), 1, lo2, hi2) == RXR_OK
        assert list(lo) == list(lo2) and list(hi) == list(hi2), "without device_modifiers the chunk is built from the registered heights"
    finally:
        api.lib.rxh_set_device_projection(0)
