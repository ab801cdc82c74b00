"""Near-plane clipping on the device (rxr_project.hip) with something to scan: the packed (vertices, fan triangles) append counts of
triangles that cross z_view = -0.1, scanned across k_proj_scan's chunks of 8192 entries and across k_proj_small's rounds of 256.

tests/test_gpu_thresholds.py and tests/test_gpu_device_projection.py reach these paths with all-zero append tables or with a single
chunk / a single round; here every case first proves on the CPU (view-space z in numpy, cross-checked with the host mirror's counts)
that appending triangles sit where the case aims -- in every chunk, on both sides of a chunk boundary, behind the first round of 64
chunks, in every round of 256 -- and then compares, byte for byte, every mesh's projected arrays with the C++ host mirror's
(Scene::project, pinned to the oracle by the CPU tests) and the device-projected frame with the host-projected frame.

The scenes are built in the view space of a home pose: a lattice of small far triangles per mesh (nothing to append), and a few
triangles between a pool of vertices in front of the near plane and a pool behind it (3 appended vertices with one corner in front, 4
with two).  A pose is the eye's displacement in home view coordinates: (0, 0, 2) backs out until nothing crosses the plane."""
import ctypes as C
import hashlib
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import rusterix_amd
from rusterix_amd import binding as B
from rusterix_amd import scenes
from tests.test_gpu_device_projection import devproj  # noqa: F401  (devproj: the fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 8192        # RXR_PROJ_SCAN_CHUNK: entries per workgroup of k_proj_scan
ROUND = 256         # entries per round of k_proj_small's scan
SMALL_MAX = 1024    # RXR_PROJ_SMALL_MAX
NEAR = 0.1
W, H = 384, 216
PLAIN, CLIP3, CLIP4, BEHIND = 0, 3, 4, 9     # what a triangle is built to be at the home pose
HOME, OUTSIDE = (0.0, 0.0, 0.0), (0.0, 0.0, 2.0)
KEYS = ("projected_vertices", "clipped_uvs", "clipped_normals", "clipped_indices", "edges", "bounding_box")


# ---- scenes --------------------------------------------------------------------------------------------------------------------
def mesh(kinds, cull=B.CULL_OFF, slot_x=0.0, far_away=False, pad_verts_to=None, gmax=64, no_verts=False):
    return types.SimpleNamespace(kinds=np.asarray(kinds, np.int8), cull=cull, slot_x=slot_x, far_away=far_away, pad_verts_to=pad_verts_to,
                                 gmax=gmax, no_verts=no_verts)


def kinds_with_clips(n, every=37, first=5, force=()):
    """n triangles, every `every`-th from `first` on crossing the near plane (3 and 4 appended vertices in turn, now and then one wholly
    behind the plane), and those at `force`"""
    k = np.zeros(n, np.int8)
    at = np.unique(np.concatenate([np.arange(first, n, every), np.asarray([f for f in force if 0 <= f < n], np.int64)])).astype(np.int64)
    k[at] = np.where(np.arange(len(at)) % 2 == 0, CLIP3, CLIP4)
    k[at[7::11]] = BEHIND
    return k


def _mesh_geometry(rng, m):
    """view-space (home pose) vertices [n, 3], indices [t, 3] of one mesh"""
    n = len(m.kinds)
    plain = np.nonzero(m.kinds == PLAIN)[0]
    G = int(min(max(2, np.ceil(np.sqrt(max(len(plain), 1))) + 1), m.gmax))
    gy, gx = np.mgrid[0:G, 0:G]
    ox, oy = rng.uniform(-0.3, 0.3, 2)
    lat = np.stack([ox + (gx.ravel() / (G - 1) - 0.5) * 4.4, oy + (gy.ravel() / (G - 1) - 0.5) * 2.4, -3.0 - rng.random(G * G)], axis=1)
    lvl_front, lvl_back = np.array([-0.16, -0.22, -0.30, -0.36]), np.array([0.05, 0.12, 0.20, 0.28])
    pool_xy = lambda: np.stack([m.slot_x + rng.uniform(-0.04, 0.04, 4), rng.uniform(-0.04, 0.04, 4)], axis=1)
    front = np.concatenate([pool_xy(), rng.permutation(lvl_front)[:, None]], axis=1)
    back = np.concatenate([pool_xy(), rng.permutation(lvl_back)[:, None]], axis=1)
    verts = np.concatenate([lat, front, back])
    F, K = G * G, G * G + 4
    idx = np.zeros((n, 3), np.int64)
    j = np.arange(len(plain))
    q = j % ((G - 1) * (G - 1))
    p = (q // (G - 1)) * G + q % (G - 1)     # (a cell of the lattice: its corner, the one to the right, the one below)
    flip = (j % 2 == 1)[:, None]
    idx[plain] = np.where(flip, np.stack([p, p + G, p + 1], axis=1), np.stack([p, p + 1, p + G], axis=1))
    for kind in (CLIP3, CLIP4, BEHIND):
        at = np.nonzero(m.kinds == kind)[0]
        a, b = rng.integers(0, 4, len(at)), rng.integers(0, 4, len(at))
        a2, b2 = (a + 1 + rng.integers(0, 3, len(at))) % 4, (b + 1 + rng.integers(0, 3, len(at))) % 4
        if kind == CLIP3:
            tri = np.stack([F + a, K + b, K + b2], axis=1)
        elif kind == CLIP4:
            tri = np.stack([F + a, F + a2, K + b], axis=1)
        else:
            tri = np.stack([K + b, K + (b + 1) % 4, K + (b + 2) % 4], axis=1)
        rot = (np.arange(3)[None, :] + (at % 3)[:, None]) % 3     # (the corner in front is the first, second or third)
        idx[at] = np.take_along_axis(tri, rot, axis=1)
    if n:
        used, inv = np.unique(idx.ravel(), return_inverse=True)
        verts, idx = verts[used], inv.reshape(n, 3)
    else:
        verts = verts[:0] if m.no_verts else verts[:3]
    if m.pad_verts_to is not None:
        extra = m.pad_verts_to - len(verts)
        assert extra >= 0
        verts = np.concatenate([verts, np.stack([rng.uniform(-2, 2, extra), rng.uniform(-1, 1, extra), rng.uniform(-4, -3, extra)], axis=1)])
    if m.far_away:
        verts = verts + np.array([500.0, 0.0, 0.0])
    return verts, idx


def world_of(spec, seed):
    """plain numpy arrays of the whole scene (world space), built once per case and replayed into every Scene of the case"""
    cam = rusterix_amd.load().D3OrbitCamera.new()
    cam.set_parameter_f32("distance", 3.0)
    v, p = cam.matrices(float(W), float(H))
    home = v.reshape(4, 4).T.astype(np.float64)
    inv = np.linalg.inv(home)
    rng = np.random.default_rng([0x52585231, 1717, seed])
    out = []
    for m in spec:
        vs, idx = _mesh_geometry(rng, m)
        v4 = np.concatenate([vs, np.ones((len(vs), 1))], axis=1) @ inv.T
        v4[:, 3] = 1.0
        out.append((v4.astype(np.float32), idx.astype(np.uint32), rng.uniform(0.0, 2.0, (len(vs), 2)).astype(np.float32), m))
    return types.SimpleNamespace(meshes=out, home=home, proj=p, n_tris=sum(len(m.kinds) for m in spec), n_verts=sum(len(o[0]) for o in out))


def view_matrix(world, pose):
    t = np.eye(4)
    t[:3, 3] = -np.asarray(pose, np.float64)
    return np.ascontiguousarray((t @ world.home).astype(np.float32).T).reshape(16)


def make_cfg(api, world, pose=HOME):
    scene = api.Scene.empty()
    for k, (v4, idx, uv, m) in enumerate(world.meshes):
        b = api.Batch3D.new(v4, idx, uv).with_computed_normals().cull_mode(m.cull)
        if k % 3 == 2:
            b.source(B.PixelSource.Pixel((40 + 50 * (k % 4), 250 - 30 * (k % 7), 90 + 20 * (k % 5), 255)))
        else:
            b.source(B.PixelSource.StaticTileIndex(k % 2)).repeat_mode(B.REPEAT_REPEAT_XY)
        scene.add_d3_static(b)
    assets = api.Assets.default().textures([B.Tile.from_texture(scenes.noise_texture(300 + k)) for k in range(2)])
    cfg = scenes._result(api, scene, assets, None, W, H, 40, "projection-clip", pose=pose)
    cfg.setup = lambda: api.Rasterizer.setup(None, view_matrix(world, cfg.pose), world.proj).ambient((1.0, 1.0, 1.0, 1.0))
    return cfg


# ---- the CPU side: what appends where -------------------------------------------------------------------------------------------
def append_counts(world, pose, refs):
    """per original triangle of the frame, the vertices it appends (0, 3 or 4): batch3d.rs:586-669 on view-space coordinates in
    float64 (no coordinate lies within 1e-3 of the plane, no orientation within 1e-9 of zero: float32 agrees), 0 for the meshes the
    host mirror rejected; cross-checked with the mirror's appended vertex and triangle counts mesh by mesh"""
    vm = view_matrix(world, pose).reshape(4, 4).T.astype(np.float64)
    out = []
    for i, (v4, idx, _, m) in enumerate(world.meshes):
        nv = np.zeros(len(idx), np.int64)
        rejected = refs[i]["bounding_box"][0] == 0.0 and len(v4) > 0
        if len(idx) and not rejected:
            vs = v4.astype(np.float64) @ vm.T
            z = vs[:, 2][idx]
            assert np.abs(z + NEAR).min() > 1e-3, (i, "a vertex too close to the near plane for a float64 precondition")
            inn = z < -NEAR
            nv = inn.sum(axis=1) + (inn != np.roll(inn, -1, axis=1)).sum(axis=1)
            nv[inn.all(axis=1) | ~inn.any(axis=1)] = 0
            if m.cull != B.CULL_OFF:
                x, y = vs[:, 0][idx], vs[:, 1][idx]
                orient = (x[:, 1] - x[:, 0]) * (y[:, 2] - y[:, 0]) - (y[:, 1] - y[:, 0]) * (x[:, 2] - x[:, 0])
                assert np.abs(orient).min() > 1e-9, (i, "a degenerate triangle in a culled mesh")
                front = orient > 0.0
                nv[front if m.cull == B.CULL_BACK else ~front] = 0
        assert set(np.unique(nv)) <= {0, 3, 4}
        if not rejected:
            got_v, got_t = refs[i]["projected_vertices"].shape[0] - len(v4), refs[i]["clipped_indices"].shape[0] - len(idx)
            assert (got_v, got_t) == (int(nv.sum()), int((nv[nv > 0] - 2).sum())), (i, "numpy and the host mirror disagree", got_v, got_t)
        out.append(nv)
    return out


def per_bin(nv_all, size):
    """(entries, triangles appending 3 vertices, triangles appending 4) for every `size` entries of the table of n_tris + 1"""
    n = len(nv_all) + 1
    rows = []
    for b in range((n + size - 1) // size):
        part = nv_all[b * size:(b + 1) * size]
        rows.append((min(n, (b + 1) * size) - b * size, int((part == 3).sum()), int((part == 4).sum())))
    return rows


def host_projection(product, world, pose):
    """the host mirror's Scene::project of the pose -- CPU only -- and what it says about the frame"""
    cfg = make_cfg(product, world, pose)
    cfg.setup().project(cfg.scene, W, H)
    refs = [cfg.scene.projected_batch3d(B.LIST_STATIC, i) for i in range(len(world.meshes))]
    nv = append_counts(world, pose, refs)
    small = world.n_verts <= SMALL_MAX and world.n_tris < SMALL_MAX and len(world.meshes) <= SMALL_MAX
    return types.SimpleNamespace(cfg=cfg, refs=refs, nv=nv, nv_all=np.concatenate(nv) if nv else np.zeros(0, np.int64), small=small,
                                 rejected=[r["bounding_box"][0] == 0.0 and len(w[0]) > 0 for r, w in zip(refs, world.meshes)])


def assert_knobs_untouched():
    assert "RXR_PROJ_SMALL" not in os.environ and "RXR_PROJ_FUSED_EDGES" not in os.environ


def assert_bins_append(hp, size, what, both_kinds=True):
    rows = per_bin(hp.nv_all, size)
    print(f"{what}: {len(hp.nv_all)} triangles, {len(rows)} x {size}: (entries, 3-vertex, 4-vertex) = {rows}")
    for b, (entries, n3, n4) in enumerate(rows):
        if b * size < len(hp.nv_all):     # (a last bin that holds the sentinel alone has no triangle)
            assert (n3 > 0 and n4 > 0) if both_kinds else (n3 + n4 > 0), (what, "bin", b, "appends", n3, n4)
    return rows


# ---- the GPU side ---------------------------------------------------------------------------------------------------------------
_rxr = None


def read_mesh(product, index, cap_v, cap_t):
    """rxr_read_projected_mesh into numpy buffers (the Edges records as [n, 10] float32 with `visible` converted, like the host mirror's copy)"""
    global _rxr
    if _rxr is None:
        _rxr = rusterix_amd.rxr_abi()
    counts = (C.c_uint32 * 2)()
    pv, uv, nr = np.zeros((cap_v, 4), np.float32), np.zeros((cap_v, 2), np.float32), np.zeros((cap_v, 3), np.float32)
    idx, ed, bb = np.zeros((cap_t, 3), np.uint32), np.zeros((cap_t, 10), np.uint32), np.zeros(5, np.float32)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    rc = _rxr.rxr_read_projected_mesh(product.lib.rxh_context(), index, counts, fp(pv), fp(uv), fp(nr), idx.ctypes.data_as(C.POINTER(C.c_uint32)),
                                      ed.ctypes.data, fp(bb), cap_v, cap_t)
    assert rc == 0, (index, rc)
    nv, nt = counts[0], counts[1]
    edges = ed[:nt].view(np.float32).copy()
    edges[:, 9] = ed[:nt, 9].astype(np.float32)
    return dict(projected_vertices=pv[:nv], clipped_uvs=uv[:nv], clipped_normals=nr[:nv], clipped_indices=idx[:nt], edges=edges, bounding_box=bb)


def assert_arrays(product, hp, what):
    """every mesh of the device-projected frame just rendered against the host mirror's arrays"""
    for i, ref in enumerate(hp.refs):
        nv, nt = ref["projected_vertices"].shape[0], ref["clipped_indices"].shape[0]
        if ref["bounding_box"][0] == 0.0:      # frustum-rejected (or without vertices): everything cleared on both sides
            got = read_mesh(product, i, 8, 8)
            assert nv == 0 and nt == 0
            if hp.rejected[i]:
                assert got["bounding_box"][0] == 0.0, (what, i)
            assert got["projected_vertices"].shape[0] == 0 and got["clipped_indices"].shape[0] == 0, (what, i, "a rejected mesh is not cleared")
            continue
        got = read_mesh(product, i, nv + 16, nt + 16)
        for key in KEYS:
            assert got[key].shape == ref[key].shape, (what, "mesh", i, key, got[key].shape, ref[key].shape)
            if got[key].tobytes() != ref[key].tobytes():
                a, b = got[key].reshape(len(got[key]), -1).view(np.uint32), ref[key].reshape(len(ref[key]), -1).view(np.uint32)
                slot = int(np.nonzero((a != b).any(axis=1))[0][0])
                raise AssertionError(f"{what}: mesh {i} of {len(hp.refs)}, {key}: first differing slot {slot} of {len(a)} "
                                     f"(originals: {len(hp.nv[i])} triangles), device {got[key][slot].tolist()}, host mirror {ref[key][slot].tolist()}")


def render_pair(product, devproj, world, hp, what):
    """the host-projected frame, the device-projected frame of a scene of its own, its arrays against the mirror's; returns the frame"""
    devproj.off()
    want = scenes.render(hp.cfg).copy()
    devproj.on()
    cfg = make_cfg(product, world, hp.cfg.pose)
    got = scenes.render(cfg).copy()
    assert_arrays(product, hp, what)
    assert np.array_equal(got, want), f"{what}: {(got != want).any(axis=2).sum()} pixels of the device-projected frame differ from the host-projected one"
    return got


def run_case(product, devproj, world, what, small, size):
    assert_knobs_untouched()
    hp = host_projection(product, world, HOME)
    assert hp.small == small, (what, world.n_verts, world.n_tris, len(world.meshes))
    rows = assert_bins_append(hp, size, what, both_kinds=size == CHUNK)    # (a last round may hold a single triangle: one kind there)
    assert sum(r[1] for r in rows) > 0 and sum(r[2] for r in rows) > 0
    got = render_pair(product, devproj, world, hp, what)
    assert (got[..., :3].max(axis=2) > 0).mean() > 0.05
    return hp


# ---- A: chunk boundaries of k_proj_scan ------------------------------------------------------------------------------------------
def chunk_layout(total):
    """meshes of 3000 triangles, a mesh without triangles and a frustum-rejected mesh (whose triangles would append) behind the first;
    appending triangles every 37th, at both sides of every chunk boundary and at the last triangle"""
    sizes, left = [], total - 40
    while left > 0:
        sizes.append(min(3000, left))
        left -= sizes[-1]
    force = [0, total - 1] + [c * CHUNK + d for c in range(1, total // CHUNK + 1) for d in (-1, 0)]
    spec, at = [], 0
    for k, n in enumerate(sizes):
        spec.append(mesh(kinds_with_clips(n, first=5 + k, force=[f - at for f in force]), slot_x=0.03 * (k % 5 - 2)))
        at += n
        if k == 0:
            spec.append(mesh([]))
            spec.append(mesh(kinds_with_clips(40, every=3, first=0), far_away=True))
            at += 40
    return spec


@pytest.mark.parametrize("total", [8191, 8192, 16383, 11000, 19000])
def test_append_scan_across_chunk_boundaries(product, devproj, total):
    """n_tris_in + 1 = 8192 (one full chunk), 8193 (the sentinel alone in a chunk), 16384 (two full chunks), and two and three chunks
    of triangles: every chunk_base[c > 0] is a non-zero sum of both words"""
    world = world_of(chunk_layout(total), total)
    assert world.n_tris == total
    hp = run_case(product, devproj, world, f"{total} triangles", small=False, size=CHUNK)
    starts = np.cumsum([0] + [len(n) for n in hp.nv])
    bounds = [c * CHUNK for c in range(1, (total - 1) // CHUNK + 1)]     # boundaries with triangles on both sides
    assert len(bounds) == {8191: 0, 8192: 0, 16383: 1, 11000: 1, 19000: 2}[total]
    assert hp.rejected[2] and not any(hp.rejected[:2]) and len(hp.nv[1]) == 0 and hp.nv[0].any() and hp.nv[3].any()
    if bounds:
        straddles = [i for i in range(len(hp.nv)) for b in bounds
                     if starts[i] < b < starts[i + 1] and hp.nv[i][:b - starts[i]].any() and hp.nv[i][b - starts[i]:].any()]
        behind = [i for i in range(len(hp.nv)) if starts[i] >= bounds[0] and hp.nv[i].any()]
        assert straddles and behind, (straddles, behind)
        for b in bounds:
            assert hp.nv_all[b - 1] and hp.nv_all[b], b
    assert hp.nv_all[total - 1] and hp.nv_all[0]


# ---- B: more than 64 chunks ----------------------------------------------------------------------------------------------------
def test_append_scan_across_more_than_64_chunks(product, devproj):
    """65 chunks: the last workgroup turns chunk totals into bases 64 at a time, the carry out of the first 64 is non-zero and used"""
    total = 64 * CHUNK + 300
    sizes = [40000] * 13 + [total - 13 * 40000]
    force = {0: [0], 6: [7, 8], 13: [64 * CHUNK - 13 * 40000 - 1, 64 * CHUNK - 13 * 40000, sizes[13] - 1]}
    spec = [mesh(kinds_with_clips(n, every=4001, first=11 + k, force=force.get(k, ())), slot_x=0.02 * (k % 5 - 2)) for k, n in enumerate(sizes)]
    world = world_of(spec, 65)
    assert world.n_tris == total and (total + 1 + CHUNK - 1) // CHUNK == 65
    assert_knobs_untouched()
    hp = host_projection(product, world, HOME)
    assert not hp.small
    rows = per_bin(hp.nv_all, CHUNK)
    print("65 chunks: (entries, 3-vertex, 4-vertex) of chunk 0, chunks 1..63 summed, chunk 64 =", rows[0], np.sum(rows[1:64], axis=0).tolist(), rows[64])
    assert sum(rows[0][1:]) > 0 and all(sum(r[1:]) > 0 for r in rows[1:64]) and sum(rows[64][1:]) > 0
    assert hp.nv_all[64 * CHUNK - 1] and hp.nv_all[64 * CHUNK] and hp.nv_all[total - 1]
    render_pair(product, devproj, world, hp, "65 chunks")


# ---- C: k_proj_small's rounds and limits ---------------------------------------------------------------------------------------
def _round_force(total):
    return [0, total - 1] + [r * ROUND + d for r in range(1, total // ROUND + 1) for d in (-1, 0)]


def one_mesh(total, cull=B.CULL_OFF, pad_verts_to=None):
    return [mesh(kinds_with_clips(total, every=29, first=3, force=_round_force(total)), cull=cull, gmax=24, pad_verts_to=pad_verts_to)]


def split(total, sizes, cull=B.CULL_OFF, gmax=16, clip_in=lambda k: True):
    assert sum(sizes) == total
    force, spec, at = _round_force(total), [], 0
    for k, n in enumerate(sizes):
        spec.append(mesh(kinds_with_clips(n, every=29, first=3 + k % 5, force=[f - at for f in force]) if clip_in(k) or any(at <= f < at + n for f in force)
                         else np.zeros(n, np.int8), cull=cull, gmax=gmax, slot_x=0.03 * (k % 5 - 2)))
        at += n
    return spec


SMALL_CASES = {
    "255 in one mesh": (lambda: one_mesh(255), True),
    "256 in one mesh": (lambda: one_mesh(256), True),
    "257 in one mesh": (lambda: one_mesh(257), True),
    "511 in one mesh": (lambda: one_mesh(511), True),
    "513 in one mesh": (lambda: one_mesh(513), True),
    "1023 in one mesh": (lambda: one_mesh(1023), True),
    "1024 in one mesh": (lambda: one_mesh(1024), False),
    "1025 in one mesh": (lambda: one_mesh(1025), False),
    "300 + 300 + 300": (lambda: split(900, [300, 300, 300]), True),
    "341 + 341 + 341": (lambda: split(1023, [341, 341, 341]), True),
    "200 meshes of 5": (lambda: split(1000, [5] * 200, gmax=2, clip_in=lambda k: k % 5 == 0), True),
    "1024 vertices": (lambda: one_mesh(300, pad_verts_to=1024), True),
    "1025 vertices": (lambda: one_mesh(300, pad_verts_to=1025), False),
}


def _many_meshes(n_meshes):
    """`n_meshes` meshes, every fourth of one triangle (every second of those crosses the plane), the others without triangles or vertices"""
    spec, t = [], 0
    for k in range(n_meshes):
        if k % 4 == 1:
            spec.append(mesh([(CLIP3, PLAIN, CLIP4, PLAIN)[t % 4]], gmax=2, slot_x=0.03 * (t % 5 - 2)))
            t += 1
        else:
            spec.append(mesh([], no_verts=True))
    return spec


SMALL_CASES["1024 meshes"] = (lambda: _many_meshes(1024), True)
SMALL_CASES["1025 meshes"] = (lambda: _many_meshes(1025), False)


@pytest.mark.parametrize("name", list(SMALL_CASES))
def test_one_workgroup_projection_rounds_and_limits(product, devproj, name):
    """k_proj_small's scan in rounds of 256 with a carry (appending triangles in every round, at both sides of every round's end and at
    the last triangle), and each of its three limits from both sides"""
    build, small = SMALL_CASES[name]
    spec = build()
    world = world_of(spec, len(name) * 1000 + len(spec))
    hp = run_case(product, devproj, world, name, small=small, size=ROUND)
    if "in one mesh" in name:
        assert world.n_tris == int(name.split()[0]) and hp.nv_all[-1] and hp.nv_all[0]
    if "vertices" in name:
        assert world.n_verts == int(name.split()[0]) and world.n_tris < SMALL_MAX
    if "meshes" in name and "of" not in name:
        assert len(world.meshes) == int(name.split()[0]) and world.n_verts <= SMALL_MAX and world.n_tris < SMALL_MAX


@pytest.mark.parametrize("cull", [B.CULL_OFF, B.CULL_FRONT, B.CULL_BACK])
@pytest.mark.parametrize("total", [511, 1024])
def test_culled_triangles_append_nothing(product, devproj, total, cull):
    """both projection paths under each cull mode: a culled triangle that crosses the plane appends nothing, one that survives does"""
    world = world_of(split(total, [total // 2, total - total // 2], cull=cull, gmax=20), total * 10 + cull)
    hp = run_case(product, devproj, world, f"{total} triangles, cull mode {cull}", small=total < SMALL_MAX, size=ROUND)
    built = np.concatenate([m.kinds for _, _, _, m in world.meshes])
    crossing = (built == CLIP3) | (built == CLIP4)
    if cull == B.CULL_OFF:
        assert (hp.nv_all[crossing] > 0).all()
    else:
        assert (hp.nv_all[crossing] == 0).sum() >= 5 and (hp.nv_all[crossing] > 0).sum() >= 5, "the cull mode removes none or all of the crossing triangles"


# ---- D: frame sequences on resident meshes -----------------------------------------------------------------------------------------
def sequence_spec(total, gmax):
    """mixed meshes around three meshes of near triangles only (small boxes around the eye: a sideways step rejects them)"""
    near_only = lambda k: mesh([CLIP3, CLIP4, CLIP3, BEHIND, CLIP4, CLIP3], slot_x=0.05 * (k - 1), gmax=2)
    sizes = [total // 3, total // 3, total - 2 * (total // 3) - 18]
    force = [0, total - 1] + [c * CHUNK + d for c in range(1, total // CHUNK + 1) for d in (-1, 0)]
    spec, at = [], 0
    for k, n in enumerate(sizes):
        spec.append(mesh(kinds_with_clips(n, every=23, first=2 + k, force=[f - at for f in force]), gmax=gmax, slot_x=0.03 * (k - 1)))
        at += n
        spec.append(near_only(k))
        at += 6
    return spec


# (0.35 back: three of the four levels behind the plane come to lie in front of it; 2 to the side: the boxes of the near-only meshes leave
# the frustum, the lattices do not)
POSES = [("outside", OUTSIDE), ("inside", HOME), ("inside, fewer", (0.0, 0.0, 0.35)), ("a step to the side", (2.0, 0.0, 0.0)), ("outside again", OUTSIDE),
         ("inside again", HOME)]


@pytest.mark.parametrize("total,gmax", [(9500, 64), (700, 14)], ids=["two chunks", "one workgroup"])
def test_camera_walks_in_and_out_of_resident_meshes(product, devproj, total, gmax):
    """one registration, six poses: nothing clipped -> clipped -> fewer clipped -> a clipped mesh frustum-rejected -> nothing -> clipped.
    ticket[1] is cleared and raised again, ticket[0] is reset by a scan that ran, and the slots behind a mesh_live that shrank keep
    records of the frame before: every frame equals a fresh host-projected render of its pose"""
    assert_knobs_untouched()
    world = world_of(sequence_spec(total, gmax), total)
    assert world.n_tris == total
    hps = [host_projection(product, world, pose) for _, pose in POSES]
    fans = lambda nv: int((nv[nv > 0] - 2).sum())
    appended = [fans(hp.nv_all) for hp in hps]
    print(f"{total} triangles: appended fan triangles per pose {dict(zip([n for n, _ in POSES], appended))}, rejected meshes in the step aside: {hps[3].rejected}")
    assert all(hp.small == (total < SMALL_MAX) for hp in hps)
    assert appended[0] == 0 and appended[4] == 0 and appended[1] == appended[5] > appended[2] > 0
    size = ROUND if hps[0].small else CHUNK
    assert_bins_append(hps[1], size, f"{total} triangles, inside")
    assert_bins_append(hps[2], size, f"{total} triangles, inside with fewer", both_kinds=False)
    shrunk = [i for i in range(len(world.meshes)) if 0 < fans(hps[2].nv[i]) < fans(hps[1].nv[i])]   # (stale fan slots behind the live ones)
    assert len(shrunk) >= 3, shrunk
    clipped_then_rejected = [i for i in range(len(world.meshes)) if hps[3].rejected[i] and hps[2].nv[i].any()]
    assert clipped_then_rejected and (hps[3].nv_all > 0).any() and not any(hps[1].rejected)
    devproj.off()
    wants = [scenes.render(hp.cfg).copy() for hp in hps]     # (first: nothing comes between the frames of the resident meshes)
    devproj.on()
    cfg = make_cfg(product, world)
    for (name, pose), hp, want in zip(POSES, hps, wants):
        cfg.pose = pose
        got = scenes.render(cfg).copy()
        assert_arrays(product, hp, f"{total} triangles, {name}")
        assert np.array_equal(got, want), f"{total} triangles, {name}: {(got != want).any(axis=2).sum()} pixels differ from the host-projected frame"
        # the frame-level shortcut is in the state the frame calls for (a flag left raised costs a frame that clips nothing its scan and
        # its emit pass, and changes no byte), and the scan's arrival counter is back at zero
        ticket = (C.c_uint32 * 2)()
        assert _rxr.rxr_debug_projection_ticket(C.c_void_p(product.lib.rxh_context()), ticket) == 0
        assert list(ticket) == [0, 1 if (hp.nv_all > 0).any() else 0], (total, name, list(ticket))


def test_a_smaller_scene_after_a_heavily_clipped_large_one(oracle, product, devproj):
    """a different, smaller device-projected scene right after a clipped one of three chunks (the pools keep the large scene's records
    behind the small one's): equal to the oracle"""
    assert_knobs_untouched()
    world = world_of(chunk_layout(19000), 19000)
    hp = host_projection(product, world, HOME)
    assert (hp.nv_all > 0).sum() > 400
    devproj.on()
    scenes.render(make_cfg(product, world))
    kw = dict(width=333, height=211, distance=0.7, textured=True, logo_size=64)
    got = scenes.render(scenes.cube_scene(product, **kw)).copy()
    ref = scenes.render(scenes.cube_scene(oracle, **kw))
    assert np.array_equal(got, ref), f"{(got != ref).any(axis=2).sum()} pixels differ from the oracle"
    small = world_of(one_mesh(300), 300)
    hp = host_projection(product, small, HOME)
    assert hp.small and (hp.nv_all > 0).sum() > 8
    render_pair(product, devproj, small, hp, "300 triangles after 19000")


# ---- E: the two static knobs, each in a process of its own ----------------------------------------------------------------------
def knob_digest(product):
    """device-projected frames and arrays of one small clipped scene and one clipped scene of two chunks, as one line of hashes"""
    product.lib.rxh_set_device_projection(1)
    out = []
    try:
        for what, spec, seed in (("small", split(900, [300, 300, 300]), 900), ("two chunks", chunk_layout(11000), 11000)):
            world = world_of(spec, seed)
            frame = scenes.render(make_cfg(product, world))
            h = hashlib.sha256(frame.tobytes())
            for i, (v4, idx, _, _) in enumerate(world.meshes):
                got = read_mesh(product, i, 2 * len(v4) + 64, 3 * len(idx) + 64)
                for key in KEYS:
                    h.update(got[key].tobytes())
            out.append(f"{what}={h.hexdigest()}")
    finally:
        product.lib.rxh_set_device_projection(0)
    return "DIGEST " + " ".join(out)


CHILD = "import sys; sys.path.insert(0, %r); import rusterix_amd; from tests.test_gpu_projection_clip import knob_digest; print(knob_digest(rusterix_amd.load()))" % ROOT


def test_static_knobs_change_no_byte(product, devproj):
    """RXR_PROJ_SMALL=0 (the small scene takes the multi-launch path) and RXR_PROJ_FUSED_EDGES=0 (k_proj_edges fills the Edges pool the
    set-up reads): read once per process, so each runs in a child of its own, one after the other"""
    assert_knobs_untouched()
    for spec, seed, small in ((split(900, [300, 300, 300]), 900, True), (chunk_layout(11000), 11000, False)):
        world = world_of(spec, seed)
        hp = host_projection(product, world, HOME)
        assert hp.small == small
        assert_bins_append(hp, ROUND if small else CHUNK, f"knobs, {world.n_tris} triangles")
        render_pair(product, devproj, world, hp, f"default knobs, {world.n_tris} triangles")
    want = knob_digest(product)
    for knob in ("RXR_PROJ_SMALL", "RXR_PROJ_FUSED_EDGES"):
        pr = subprocess.run([sys.executable, "-c", CHILD], capture_output=True, text=True, timeout=240, env=dict(os.environ, **{knob: "0"}), cwd=ROOT)
        assert pr.returncode == 0, (knob, pr.stdout[-2000:], pr.stderr[-4000:])
        lines = [l for l in pr.stdout.splitlines() if l.startswith("DIGEST")]
        assert lines and lines[-1] == want, (knob, lines, want)


# ---- F: members ----------------------------------------------------------------------------------------------------------------
def test_two_chunk_clipped_scene_on_three_members(product, devproj):
    from tests.test_gpu_multi import use_members

    assert_knobs_untouched()
    world = world_of(chunk_layout(11000), 11000)
    hp = host_projection(product, world, HOME)
    assert not hp.small
    assert_bins_append(hp, CHUNK, "members, 11000 triangles")
    try:
        product.lib.rxh_set_device(0)
        devproj.on()
        cfg = make_cfg(product, world)
        ref = scenes.render(cfg).copy()
        use_members(product, 3)
        devproj.on()
        got = scenes.render(cfg).copy()
        assert np.array_equal(got, ref), f"3 members: {(got != ref).any(axis=2).sum()} pixels differ from the single-context frame"
        assert_arrays(product, hp, "3 members (member 0's arrays)")
    finally:
        product.lib.rxh_set_device(0)
        product.lib.rxh_set_device_projection(0)
