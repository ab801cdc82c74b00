"""Terrain chunk meshes on the device (rxr_terrain_meshes / rxr_terrain_meshes_to, TerrainChunk::build_mesh) against the dictionary
transcription of tests/terrain_mesh_ref.py with the oracle's normals: every output word equal, no tolerance (one test with NaN and
infinite heights asks for a NaN where the reference has one and for the bits elsewhere).  Every call's buffers are filled with a
sentinel first: the words past each chunk's counts and a guard region behind the last chunk must come back unchanged.

Shapes are the smallest at which the kernel can go wrong: chunk sizes on both sides of a wave of cells (8 / 9), of a round of 256
cells (16 / 17), the bound (64) and one above it; per size every presence shape of terrain_mesh_ref.masks side by side in one
terrain, so that a chunk's rim reads its neighbours' heights where they are listed and 0.0 where not, at negative coordinates and
on the edge of the heights' rectangle; more chunks than one launch takes."""
import ctypes as C

import numpy as np
import pytest

import rusterix_amd
from rusterix_amd import binding as B
from rusterix_amd import scenes
from tests import terrain_hit_ref as H
from tests import terrain_mesh_ref as M
from tests.terrain_hit_ref import RXR_ERR_INVALID, RXR_ERR_UNSUPPORTED, RXR_OK
from tests.terrain_mesh_ref import F, HeightSpec

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5C3F00D
GUARD = 64                     # words behind the last chunk of every array
LAUNCH_CHUNKS = 256            # rxr_terrain_mesh.hip MESH_LAUNCH_CHUNKS


def context_of(product):
    return C.c_void_p(product.lib.rxh_context())


def last_error(rxr, ctx):
    return (rxr.rxr_last_error(ctx) or b"").decode()


def set_heights(rxr, ctx, spec):
    keep, args = spec.arrays()
    return rxr.rxr_set_terrain_heights(ctx, *args)


def strides(cs):
    return (cs + 1) ** 2, 2 * cs * cs


def buffers(n, cs, make):
    vs, ts = strides(cs)
    return dict(counts=make(n * 2 + GUARD), vertices=make(n * vs * 4 + GUARD), indices=make(n * ts * 3 + GUARD), normals=make(n * vs * 3 + GUARD))


def unpack(buf, n, cs):
    """the chunks' meshes out of the four arrays (uint32 words), after checking that no word past a chunk's counts, and none of the
    guard behind the last chunk, was written"""
    vs, ts = strides(cs)
    counts = buf["counts"][: 2 * n].reshape(n, 2)
    assert (buf["counts"][2 * n:] == SENTINEL).all(), "counts: guard"
    out = []
    for key, stride, width, which in (("vertices", vs, 4, 0), ("indices", ts, 3, 1), ("normals", vs, 3, 0)):
        body = buf[key][: n * stride * width].reshape(n, stride * width)
        assert (buf[key][n * stride * width:] == SENTINEL).all(), f"{key}: guard"
        for i in range(n):
            used = int(counts[i, which]) * width
            assert used <= stride * width, f"chunk {i}: count {counts[i, which]} exceeds the stride"
            assert (body[i, used:] == SENTINEL).all(), f"{key}: chunk {i} wrote past its count"
    for i in range(n):
        nv, nt = int(counts[i, 0]), int(counts[i, 1])
        out.append(dict(vertices=buf["vertices"][i * vs * 4: i * vs * 4 + nv * 4].view(F).reshape(nv, 4),
                        indices=buf["indices"][i * ts * 3: i * ts * 3 + nt * 3].reshape(nt, 3),
                        normals=buf["normals"][i * vs * 3: i * vs * 3 + nv * 3].view(F).reshape(nv, 3)))
    return out


def meshes(rxr, ctx, coords, cs):
    cc = np.ascontiguousarray(np.asarray(coords, np.int32).reshape(-1, 2))
    n = len(cc)
    buf = buffers(n, cs, lambda words: np.full(words, SENTINEL, np.uint32))
    rc = rxr.rxr_terrain_meshes(ctx, cc.ctypes.data, n, cs, *(buf[k].ctypes.data for k in ("counts", "vertices", "indices", "normals")))
    assert rc == RXR_OK, last_error(rxr, ctx)
    return unpack(buf, n, cs)


def expect(got, want, label="", nan_as_nan=False):
    assert len(got) == len(want), label
    for i, (g, w) in enumerate(zip(got, want)):
        d = M.first_difference(g, w, nan_as_nan)
        assert not d, f"{label} chunk {i}: {d}"


@pytest.fixture()
def dev(product):
    rxr, ctx = rusterix_amd.rxr_abi(), context_of(product)

    def register(spec):
        assert set_heights(rxr, ctx, spec) == RXR_OK, last_error(rxr, ctx)
        return spec

    return rxr, ctx, register


# ---- one terrain per chunk size: every presence shape side by side ---------------------------------------------------------------------
_TERRAINS = {}


def shapes_terrain(cs, scale, oracle):
    """(spec, coords, reference meshes), computed once: the shapes of M.masks(cs) as the chunks (k - 5, -1), and for the smaller
    sizes in reverse order as the chunks (k - 5, 0) below them.  The upper row's bottom rim reads the lower row's heights where
    listed; the lower row's (and, for size 64, the only row's) lies outside the heights' rectangle and reads 0.0, like the last
    chunk's right rim."""
    key = (cs, scale)
    if key not in _TERRAINS:
        all_masks = M.masks(cs)
        names = sorted(all_masks)
        rows = [(-1, names)] + ([(0, names[::-1])] if cs <= 17 else [])
        spec = HeightSpec(scale, cs)
        coords = []
        for cy, order in rows:
            for k, name in enumerate(order):
                cx = k - 5
                coords.append((cx, cy))
                mask = all_masks[name]
                for ly, lx in zip(*np.nonzero(mask)):
                    x, y = cx * cs + int(lx), cy * cs + int(ly)
                    spec.height(x, y, M.height_at(x, y, cs))
        _TERRAINS[key] = (spec, coords, [M.build_mesh(spec, c, oracle) for c in coords])
    return _TERRAINS[key]


@pytest.mark.parametrize("scale", [(1.0, 1.0), (0.75, 1.5)])
@pytest.mark.parametrize("cs", [1, 2, 3, 5, 8, 9, 16, 17, 64])
def test_every_presence_shape(dev, oracle, cs, scale):
    rxr, ctx, register = dev
    spec, coords, want = shapes_terrain(cs, scale, oracle)
    register(spec)
    got = meshes(rxr, ctx, coords, cs)
    expect(got, want, f"size {cs}")
    names = sorted(M.masks(cs))
    full, empty = want[names.index("full")], want[names.index("empty")]
    assert len(full["vertices"]) == (cs + 1) ** 2 and len(full["indices"]) == 2 * cs * cs
    assert len(empty["vertices"]) == 0 and len(empty["indices"]) == 0
    # one chunk alone gives the same words as in the company of the others
    one = len(coords) // 2
    expect(meshes(rxr, ctx, [coords[one]], cs), [want[one]], f"size {cs} alone")


def test_chunk_sizes_beyond_the_bound_and_other_refusals(dev):
    rxr, ctx, register = dev
    register(HeightSpec().height(0, 0, 1.0))
    zero = np.zeros((1, 2), np.int32)
    big = buffers(1, 65, lambda words: np.full(words, SENTINEL, np.uint32))
    ptrs = [big[k].ctypes.data for k in ("counts", "vertices", "indices", "normals")]
    assert rxr.rxr_terrain_meshes(ctx, zero.ctypes.data, 1, 65, *ptrs) == RXR_ERR_UNSUPPORTED and "RXR_TERRAIN_MESH_MAX_CHUNK_SIZE" in last_error(rxr, ctx)
    assert rxr.rxr_terrain_meshes(ctx, zero.ctypes.data, 1, 0, *ptrs) == RXR_ERR_INVALID and "chunk_size" in last_error(rxr, ctx)
    assert rxr.rxr_terrain_meshes(ctx, zero.ctypes.data, 1, -3, *ptrs) == RXR_ERR_INVALID
    assert rxr.rxr_terrain_meshes(ctx, None, 1, 4, *ptrs) == RXR_ERR_INVALID and "chunk_coords" in last_error(rxr, ctx)
    for missing in range(4):
        p = list(ptrs)
        p[missing] = None
        assert rxr.rxr_terrain_meshes(ctx, zero.ctypes.data, 1, 4, *p) == RXR_ERR_INVALID and "NULL" in last_error(rxr, ctx)
    # cells beyond +-2^30: chunk 2^28 of size 4 starts at 2^30 and ends 3 cells beyond it; chunk 2^28 - 1 ends at 2^30 - 1
    for bad in ([2 ** 28, 0], [0, -(2 ** 28) - 1], [2 ** 31 - 1, 0]):
        cc = np.array([[0, 0], bad], np.int32)
        assert rxr.rxr_terrain_meshes(ctx, cc.ctypes.data, 2, 4, *ptrs) == RXR_ERR_INVALID and "2^30" in last_error(rxr, ctx), bad
    edge = np.array([[2 ** 28 - 1, -(2 ** 28)]], np.int32)
    assert rxr.rxr_terrain_meshes(ctx, edge.ctypes.data, 1, 4, *ptrs) == RXR_OK, last_error(rxr, ctx)
    assert big["counts"][:2].tolist() == [0, 0]
    assert rxr.rxr_terrain_meshes(ctx, None, 0, 4, None, None, None, None) == RXR_OK          # n == 0 does nothing
    assert all((big[k][2 if k == "counts" else 0:] == SENTINEL).all() for k in big)


def test_a_mesh_at_the_coordinate_bound(dev, oracle):
    """the last chunk before +2^30 and the first after -2^30: f32 is 64 apart there, the chunk's corners all share one x and one z,
    every triangle has no area and every normal is 0 / 0 -- kept as in the reference; a NaN needs a NaN, the other words their bits"""
    rxr, ctx, register = dev
    cs = 4
    for coord in ((2 ** 28 - 1, 2 ** 28 - 1), (-(2 ** 28), -(2 ** 28))):
        spec = M.masked_spec(np.random.default_rng(4).random((cs, cs)) < 0.7, coord, (1.0, 1.0), seed=2, neighbours=False)
        register(spec)
        want = M.build_mesh(spec, coord, oracle)
        assert len(np.unique(want["vertices"][:, 0])) == 1 and np.isnan(want["normals"]).all()
        expect(meshes(rxr, ctx, [coord], cs), [want], f"chunk {coord}", nan_as_nan=True)


def test_more_chunks_than_one_launch_takes(dev, oracle):
    rxr, ctx, register = dev
    cs, n = 3, LAUNCH_CHUNKS + 44
    rng = np.random.default_rng(21)
    spec = HeightSpec((0.75, 1.5), cs)
    coords = [(int(k % 20) - 10, int(k // 20) - 7) for k in range(n)]
    for i, (cx, cy) in enumerate(coords):
        density = 0.0 if i % 7 == 3 else rng.choice([0.3, 0.6, 1.0])          # every seventh chunk has no cell, between two that have
        for ly, lx in zip(*np.nonzero(rng.random((cs, cs)) < density)):
            spec.height(cx * cs + int(lx), cy * cs + int(ly), M.height_at(cx * cs + int(lx), cy * cs + int(ly), 5))
    register(spec)
    want = [M.build_mesh(spec, c, oracle) for c in coords]
    assert len(want[3]["vertices"]) == 0 and len(want[2]["vertices"]) and len(want[4]["vertices"])
    expect(meshes(rxr, ctx, coords, cs), want, "300 chunks")
    assert rxr.rxr_debug_terrain_mesh_launches(ctx) == 2
    expect(meshes(rxr, ctx, coords[:LAUNCH_CHUNKS], cs), want[:LAUNCH_CHUNKS], "a full launch")
    assert rxr.rxr_debug_terrain_mesh_launches(ctx) == 1
    # the same chunk asked for twice in one call
    expect(meshes(rxr, ctx, [coords[0], coords[5], coords[0]], cs), [want[0], want[5], want[0]], "twice")


def test_nan_and_infinite_heights(dev, oracle):
    rxr, ctx, register = dev
    cs = 5
    spec = M.masked_spec(np.random.default_rng(6).random((cs, cs)) < 0.8, (0, 0), (1.0, 1.0), seed=3)
    keys = sorted(spec.heights)
    for k, h in zip(keys[::7], [float("nan"), float("inf"), -float("inf"), float("nan"), 3.0e38, -3.0e38]):
        spec.height(k[0], k[1], h)
    register(spec)
    want = M.build_mesh(spec, (0, 0), oracle)
    assert np.isnan(want["normals"]).any() and not np.isnan(want["normals"]).all()
    expect(meshes(rxr, ctx, [(0, 0)], cs), [want], "special heights", nan_as_nan=True)


def test_a_coordinate_listed_twice_is_present_and_a_listed_zero_is_a_cell(dev, oracle):
    rxr, ctx, _ = dev
    spec = HeightSpec((1.0, 1.0), 2).height(0, 0, 0.0).height(1, 1, 2.0)
    keep, args = spec.arrays()
    xy, hh = np.concatenate([keep["xy"], keep["xy"][:1]]), np.concatenate([keep["h"], np.array([4.0], F)])
    assert rxr.rxr_set_terrain_heights(ctx, args[0], xy.ctypes.data, hh.ctypes.data, len(hh)) == RXR_OK, last_error(rxr, ctx)
    spec.height(0, 0, 4.0)                                    # the later entry wins, as for the picks
    want = M.build_mesh(spec, (0, 0), oracle)
    assert len(want["indices"]) == 4
    expect(meshes(rxr, ctx, [(0, 0)], 2), [want], "listed twice")
    assert set_heights(rxr, ctx, HeightSpec((1.0, 1.0), 2).height(0, 0, 0.0)) == RXR_OK
    got = meshes(rxr, ctx, [(0, 0), (1, 0)], 2)
    assert len(got[0]["indices"]) == 2 and len(got[1]["indices"]) == 0


# ---- through the mirror -------------------------------------------------------------------------------------------------------------------
def geometry(batch):
    v, i, uv, n = batch.geometry()
    assert uv.shape == (len(v), 2) and not uv.any()
    return dict(vertices=v, indices=i, normals=n)


def test_the_mirror_builds_on_the_device_and_registers_its_heights_when_they_changed(product, oracle):
    spec, coords, want = shapes_terrain(9, (0.75, 1.5), oracle)
    t = spec.product(product)
    expect([geometry(b) for b in t.build_meshes(coords)], want, "first")
    expect([geometry(b) for b in t.build_meshes_cpu(coords[:4])], want[:4], "the CPU's")
    x, y = sorted(spec.heights)[0]
    t.set_height(x, y, 9.0)                                   # an edit: registered again by the generation stamp
    spec2 = HeightSpec((0.75, 1.5), 9)
    spec2.heights = dict(spec.heights)
    spec2.height(x, y, 9.0)
    c = (x // 9, y // 9)
    want2 = M.build_mesh(spec2, c, oracle)
    assert M.first_difference(want2, want[coords.index(c)])
    expect([geometry(t.build_meshes([c])[0])], [want2], "after set_height")
    assert t.build_meshes([]) == []
    product.Scene.empty().add_chunk().terrain_batch3d(t.build_meshes([c])[0])
    with pytest.raises(B.RasterizeError) as e:
        HeightSpec((1.0, 1.0), 65).height(0, 0, 1.0).product(product).build_meshes([(0, 0)])
    assert e.value.code == RXR_ERR_UNSUPPORTED


# ---- stream and lifetime -------------------------------------------------------------------------------------------------------------------
def to_buffers(n, cs):
    import torch

    return buffers(n, cs, lambda words: torch.full((words,), SENTINEL - (1 << 32), dtype=torch.int32, device="cuda"))


def to_host(buf):
    return {k: v.cpu().numpy().view(np.uint32) for k, v in buf.items()}


def test_to_form_between_a_pick_and_a_re_registration(product, oracle):
    """on a context of its own: a pick queued on stream A, at once the mesh build on stream B, at once other heights
    (rxr_set_terrain_heights waits for both); then the blocking forms on the new heights"""
    import torch

    rxr = rusterix_amd.rxr_abi()
    ctx = C.c_void_p()
    assert rxr.rxr_create(C.byref(ctx), 0) == RXR_OK
    try:
        spec, coords, want = shapes_terrain(9, (1.0, 1.0), oracle)
        other, other_coords, other_want = shapes_terrain(5, (0.75, 1.5), oracle)
        _, o, d, md, _ = H.fuzz_case(2)
        o, d = o[:300], d[:300]
        want_hits = spec.hits(o, d, md)
        assert set_heights(rxr, ctx, spec) == RXR_OK, last_error(rxr, ctx)
        n = len(coords)
        cc = np.ascontiguousarray(np.asarray(coords, np.int32))
        a, b = torch.cuda.Stream(), torch.cuda.Stream()
        do, dd = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
        hit = torch.zeros(300, dtype=torch.int32, device="cuda")
        wp = torch.zeros((300, 3), dtype=torch.float32, device="cuda")
        buf = to_buffers(n, 9)
        torch.cuda.synchronize()
        assert rxr.rxr_terrain_hits_to(ctx, do.data_ptr(), dd.data_ptr(), 300, md, hit.data_ptr(), None, wp.data_ptr(), None, C.c_void_p(a.cuda_stream)) == RXR_OK
        rc = rxr.rxr_terrain_meshes_to(ctx, cc.ctypes.data, n, 9, *(buf[k].data_ptr() for k in ("counts", "vertices", "indices", "normals")), C.c_void_p(b.cuda_stream))
        assert rc == RXR_OK, last_error(rxr, ctx)
        cc[:] = 12345                                            # (the coordinates were read before the call returned)
        assert set_heights(rxr, ctx, other) == RXR_OK, last_error(rxr, ctx)
        a.synchronize()
        b.synchronize()
        expect(unpack(to_host(buf), n, 9), want, "_to")
        assert np.array_equal(hit.cpu().numpy().view(np.uint32), want_hits["hit"])
        assert np.array_equal(M.bits(wp.cpu().numpy()), M.bits(want_hits["world_pos"]))
        expect(meshes(rxr, ctx, other_coords, 5), other_want, "the new heights")
        # a refused registration leaves mask and heights as they were
        assert set_heights(rxr, ctx, HeightSpec((0.0, 1.0)).height(0, 0, 1)) == RXR_ERR_INVALID
        expect(meshes(rxr, ctx, other_coords[:3], 5), other_want[:3], "after a refused registration")
        # the default stream; host memory where device memory is expected; a misaligned pointer; NULL
        buf2 = to_buffers(len(other_coords), 5)
        torch.cuda.synchronize()
        oc = np.ascontiguousarray(np.asarray(other_coords, np.int32))
        ptrs = [buf2[k].data_ptr() for k in ("counts", "vertices", "indices", "normals")]
        assert rxr.rxr_terrain_meshes_to(ctx, oc.ctypes.data, len(oc), 5, *ptrs, None) == RXR_OK, last_error(rxr, ctx)
        assert rxr.rxr_synchronize(ctx) == RXR_OK
        expect(unpack(to_host(buf2), len(oc), 5), other_want, "_to on the context's stream")
        host = buffers(len(oc), 5, lambda words: np.full(words, SENTINEL, np.uint32))
        for i, key in enumerate(("counts", "vertices", "indices", "normals")):
            p = list(ptrs)
            p[i] = host[key].ctypes.data
            assert rxr.rxr_terrain_meshes_to(ctx, oc.ctypes.data, len(oc), 5, *p, None) == RXR_ERR_INVALID and "dev_" + key in last_error(rxr, ctx)
            p[i] = ptrs[i] + 2
            assert rxr.rxr_terrain_meshes_to(ctx, oc.ctypes.data, len(oc), 5, *p, None) == RXR_ERR_INVALID and "aligned" in last_error(rxr, ctx)
            p[i] = None
            assert rxr.rxr_terrain_meshes_to(ctx, oc.ctypes.data, len(oc), 5, *p, None) == RXR_ERR_INVALID
        assert rxr.rxr_terrain_meshes_to(ctx, oc.ctypes.data, 1, 65, *ptrs, None) == RXR_ERR_UNSUPPORTED
        assert rxr.rxr_terrain_meshes_to(ctx, None, 0, 5, None, None, None, None, None) == RXR_OK
        assert rxr.rxr_synchronize(ctx) == RXR_OK
        assert all((v == SENTINEL).all() for v in host.values())
    finally:
        rxr.rxr_destroy(ctx)


def test_no_heights_registered_and_multi_device_handles(product, oracle):
    rxr = rusterix_amd.rxr_abi()
    cs = 3
    spec = M.masked_spec(np.ones((cs, cs), bool))
    want = [M.build_mesh(spec, (0, 0), oracle)]
    zero = np.zeros((1, 2), np.int32)
    buf = buffers(1, cs, lambda words: np.full(words, SENTINEL, np.uint32))
    ptrs = [buf[k].ctypes.data for k in ("counts", "vertices", "indices", "normals")]
    ctx = C.c_void_p()
    assert rxr.rxr_create(C.byref(ctx), 0) == RXR_OK
    try:
        assert rxr.rxr_terrain_meshes(ctx, zero.ctypes.data, 1, cs, *ptrs) == RXR_ERR_INVALID and "no terrain heights" in last_error(rxr, ctx)
        assert rxr.rxr_terrain_meshes_to(ctx, zero.ctypes.data, 1, cs, *ptrs, None) == RXR_ERR_INVALID and "no terrain heights" in last_error(rxr, ctx)
        assert set_heights(rxr, ctx, HeightSpec()) == RXR_OK     # the empty terrain: every chunk is empty
        assert rxr.rxr_terrain_meshes(ctx, zero.ctypes.data, 1, cs, *ptrs) == RXR_OK, last_error(rxr, ctx)
        assert buf["counts"][:2].tolist() == [0, 0]
    finally:
        rxr.rxr_destroy(ctx)
    multi = C.c_void_p()
    devs = (C.c_int * 2)(0, 0)
    assert rxr.rxr_create_multi(C.byref(multi), devs, 2) == RXR_OK
    try:
        assert rxr.rxr_terrain_meshes(multi, zero.ctypes.data, 1, cs, *ptrs) == RXR_ERR_INVALID and "no terrain heights" in last_error(rxr, multi)
        assert set_heights(rxr, multi, spec) == RXR_OK, last_error(rxr, multi)
        assert rxr.rxr_terrain_meshes_to(multi, zero.ctypes.data, 1, cs, *ptrs, None) == RXR_ERR_UNSUPPORTED and "multi-device" in last_error(rxr, multi)
        expect(meshes(rxr, multi, [(0, 0)], cs), want, "member 0")
        assert rxr.rxr_debug_terrain_mesh_launches(multi) == 1
    finally:
        rxr.rxr_destroy(multi)


# ---- next to the other terrain queries and the renderer -----------------------------------------------------------------------------------
def test_picks_return_the_same_bytes_after_a_mesh_build(dev, oracle):
    from tests.test_gpu_terrain_hit import hits

    rxr, ctx, register = dev
    spec, o, d, md, want_hits = H.fuzz_case(1)
    register(spec)
    before = hits(rxr, ctx, o, d, md)
    assert not H.first_difference(before, want_hits)
    cs = 8
    coords = [(-1, -1), (0, 0), (1, -1), (40, 40)]
    got = meshes(rxr, ctx, coords, cs)
    expect(got, [M.build_mesh(spec, c, oracle, cs) for c in coords], "the picks' terrain")
    assert sum(len(g["indices"]) for g in got[:3]) > 0 and len(got[3]["indices"]) == 0
    after = hits(rxr, ctx, o, d, md)
    assert all(before[k].tobytes() == after[k].tobytes() for k in H.KEYS)


def mesh_frame(api, texture, mesh):
    """terrain_frame of tests/test_gpu_terrain.py with `mesh` (vertices, indices, normals) as the chunk's terrain batch"""
    from tests.test_gpu_terrain import H as FH, W as FW

    scene = api.Scene.empty()
    chunk = scene.add_chunk()
    chunk.terrain(texture, origin=(0, 0), size=8)
    batch = mesh if isinstance(mesh, api.Batch3D) else api.Batch3D.new(mesh["vertices"], mesh["indices"], np.zeros((len(mesh["vertices"]), 2), F)).normals(mesh["normals"]).source(B.PixelSource.Terrain())
    chunk.terrain_batch3d(batch)
    cam = api.D3OrbitCamera.new()
    cam.set_parameter_f32("distance", 9.0)
    cam.center = (4.0, 0.0, 4.0)
    cam.azimuth, cam.elevation = 0.9, 0.8

    def setup():
        v, p = cam.matrices(float(FW), float(FH))
        return api.Rasterizer.setup(None, v, p).ambient((1.0, 1.0, 1.0, 1.0))

    return scenes._result(api, scene, api.Assets.default(), setup, FW, FH, 40, "terrain-mesh-frame", chunk=chunk)


@pytest.mark.parametrize("exact", [0, 1])
def test_a_frame_of_the_device_built_mesh(product, oracle, exact):
    """a chunk whose terrain batch is the mesh the device built, under a given terrain texture, renders the oracle's frame of the
    reference's mesh byte for byte; the batch is unlit, so both light modes give the same bytes"""
    from tests import terrain_ref as R

    tex = R.uniform_scene(R.RADIUS, 1, chunk_size=8, seed=9).bake((0, 0), 8)
    given = B.Texture(tex.reshape(-1).copy(), 64, 64)
    mask = np.ones((8, 8), bool)
    mask[2, 5] = mask[6, 1] = False
    spec = HeightSpec((1.0, 1.0), 8)
    for ly, lx in zip(*np.nonzero(mask)):
        spec.height(int(lx), int(ly), F(0.6 * np.sin(lx / 1.5) * np.cos(ly / 2.0)))
    want = M.build_mesh(spec, (0, 0), oracle)
    ref_frame = scenes.render(mesh_frame(oracle, given, want)).copy()
    assert len(np.unique(ref_frame.reshape(-1, 4), axis=0)) > 100, "the terrain texture should be visible"
    built = spec.product(product).build_meshes([(0, 0)])[0]
    expect([geometry(built)], [want], "the frame's mesh")
    product.lib.rxh_set_light_math_exact(exact)
    try:
        got = scenes.render(mesh_frame(product, given, built))
    finally:
        product.lib.rxh_set_light_math_exact(0)
    assert np.array_equal(got, ref_frame)
