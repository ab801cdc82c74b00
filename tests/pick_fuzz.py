"""Seeded scenes and rays for ray picking (rxr_intersect), shared by tests/test_intersect_cpu.py (the generator against the numpy
reference alone), tests/test_gpu_intersect_fuzz.py and tools/intersect_fuzz_sweep.py (the device against the reference).

random_pick_scene(seed) returns mesh dicts in rxr_set_meshes order (tests/intersect_ref.py's form, plus `chunk` and `transform`);
random_rays(meshes, seed, n) the rays.  A scene reaches the device either through the host mirror (host_scene) or, since the
mirror has no way to push a batch without vertices, straight through rxr_set_meshes on a context of its own (PickContext).

segments(meshes) restates how rxr_intersect.hip groups the meshes (isect_prepare): a run of plain-rule meshes is one segment, a
RXR_LIST_CHUNK mesh with a profile id and every overlay mesh a segment of its own, meshes without triangles belong to none."""
import ctypes as C
import os
import re

import numpy as np

from rusterix_amd.abi import rxr_mesh3d as Mesh3D
from tests import intersect_ref as R

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED_KEY = 0x52585231
EDGE_SIZES = (0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)
MAX_TRIANGLES = 6000
SPECIALS = (0.0, -0.0, np.nan, np.inf, -np.inf, 1e-40, 1e30, 3e38, -3e38)

# the seeds tests/test_intersect_cpu.py holds to the generator's conditions and tests/test_gpu_intersect_fuzz.py runs
SEEDS = tuple(range(1, 25))


def kernel_constants():
    """ISECT_WG, ISECT_FEW_RAYS, ISECT_RAYS_PER_Y, ISECT_KEYS_MAX as rxr_intersect.hip defines them"""
    src = open(os.path.join(ROOT, "rusterix_amd", "csrc", "rxr_intersect.hip")).read()
    out = {}
    for name in ("ISECT_WG", "ISECT_FEW_RAYS", "ISECT_RAYS_PER_Y", "ISECT_KEYS_MAX"):
        m = re.search(rf"constexpr uint\d+_t {name} = ([^;]+);", src)
        expr = re.sub(r"(\d+)(ull|u)\b", r"\1", m.group(1))
        assert re.fullmatch(r"[\d\s<>*+()]+", expr), expr
        out[name] = int(eval(expr))
    return out


def expected_batches(n_rays, nseg, k=None):
    """isect_run's split of `n_rays` rays over `nseg` segments: the ray count of every batch"""
    k = k or kernel_constants()
    per = n_rays
    if nseg and n_rays * nseg > k["ISECT_KEYS_MAX"]:
        per = max(k["ISECT_WG"], k["ISECT_KEYS_MAX"] // nseg // k["ISECT_WG"] * k["ISECT_WG"])
    return [min(per, n_rays - r0) for r0 in range(0, n_rays, per)]


def segments(meshes):
    """[(first global triangle, end, first mesh, end mesh, rule)] with rule 'plain', 'pid' or 'overlay'"""
    segs, g = [], 0
    for i, m in enumerate(meshes):
        n = len(m["indices"])
        if not n:
            continue
        rule = "overlay" if m["list"] == R.LIST_OVERLAY else "pid" if (m["list"] == R.LIST_CHUNK and m.get("has_pid")) else "plain"
        if rule == "plain" and segs and segs[-1][4] == "plain":
            segs[-1] = (segs[-1][0], g + n, segs[-1][2], i + 1, "plain")
        else:
            segs.append((g, g + n, i, i + 1, rule))
        g += n
    return segs


def mesh(vertices, indices, uvs=None, normals=None, list=R.LIST_STATIC, chunk=-1, pid=None, transform=None):
    v = np.ascontiguousarray(np.asarray(vertices, F).reshape(-1, 4))
    i = np.ascontiguousarray(np.asarray(indices, np.uint32).reshape(-1, 3))
    uv = np.ascontiguousarray(v[:, :2] if uvs is None else np.asarray(uvs, F).reshape(-1, 2))
    nr = np.ascontiguousarray(np.tile(np.array([0, 0, -1], F), (len(v), 1)) if normals is None else np.asarray(normals, F).reshape(-1, 3))
    return dict(vertices=v, indices=i, uvs=uv, normals=nr, list=int(list), chunk=int(chunk), has_pid=pid is not None,
                pid=0 if pid is None else int(pid), transform=None if transform is None else np.asarray(transform, F).reshape(16))


def scene_eyes(seed):
    """the ray origins of a seed: three outside the geometry, two inside (the scene builds grazing triangles through them)"""
    rng = np.random.default_rng([SEED_KEY, 4243, seed])
    out = rng.standard_normal((3, 3))
    out = out / np.linalg.norm(out, axis=1)[:, None] * rng.uniform(7.0, 12.0, (3, 1))
    return np.concatenate([out, rng.standard_normal((2, 3)) * 0.8]).astype(F)


def _soup(rng, n, eyes):
    c = rng.standard_normal((n, 1, 3)) * 2.0
    v = (c + rng.standard_normal((n, 3, 3)) * rng.uniform(0.2, 1.2)).astype(F).reshape(-1, 3)
    idx = np.arange(3 * n, dtype=np.uint32).reshape(n, 3)
    for k in np.nonzero(rng.random(n) < 0.04)[0]:
        # a triangle whose plane holds an eye: the rays from that eye at its points run along it (|a| < 1e-6 or near it)
        e = eyes[rng.integers(len(eyes))].astype(np.float64)
        along, side = rng.standard_normal(3), rng.standard_normal(3)
        along *= rng.uniform(2.0, 6.0) / np.linalg.norm(along)
        v[3 * k:3 * k + 3] = (e[None, :] + rng.uniform(0.7, 1.3, (3, 1)) * along[None, :] + rng.uniform(-0.6, 0.6, (3, 1)) * side[None, :]).astype(F)
    return v, idx


def _grid(rng, n):
    """a jittered, randomly oriented grid of shared vertices: the first n of its 2 * cx * cy triangles"""
    cx = max(1, int(np.ceil(np.sqrt(n / 2))))
    cy = max(1, int(np.ceil(n / (2 * cx))))
    xs, ys = np.meshgrid(np.linspace(-1, 1, cx + 1), np.linspace(-1, 1, cy + 1))
    p = np.stack([xs.ravel(), ys.ravel(), rng.standard_normal(xs.size) * 0.05], axis=1) * rng.uniform(1.0, 4.0)
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    v = (p @ q.T + rng.standard_normal(3) * 1.5).astype(F)
    i0 = (np.arange(cy)[:, None] * (cx + 1) + np.arange(cx)[None, :]).ravel()
    tris = np.stack([np.stack([i0, i0 + 1, i0 + cx + 2], 1), np.stack([i0, i0 + cx + 2, i0 + cx + 1], 1)], 1).reshape(-1, 3)
    return v, tris[:n].astype(np.uint32)


def _random_mesh(rng, n, eyes, **kw):
    if n == 0:
        nv = int(rng.integers(0, 4))    # no triangles: with or without vertices
        v3, idx = rng.standard_normal((nv, 3)).astype(F), np.zeros((0, 3), np.uint32)
    elif rng.random() < 0.5:
        v3, idx = _soup(rng, n, eyes)
    else:
        v3, idx = _grid(rng, n)
    idx = idx.copy()
    for k in np.nonzero(rng.random(n) < 0.02)[0]:
        idx[k, 2] = idx[k, 0]           # zero area
    nv = len(v3)
    v = np.concatenate([v3, np.ones((nv, 1), F)], axis=1)
    transform = rng.standard_normal(16).astype(F) if rng.random() < 0.3 else None   # (ignored by Scene::intersect)
    return mesh(v, idx, rng.uniform(-2, 3, (nv, 2)), rng.standard_normal((nv, 3)), transform=transform, **kw)


def random_pick_scene(seed):
    """5 to 60 meshes: one to three chunks (opacity, plain, terrain batches), then static, dynamic and overlay batches"""
    rng = np.random.default_rng([SEED_KEY, 4242, seed])
    eyes = scene_eyes(seed)
    n_meshes = int(rng.integers(5, 61))
    n_chunks = int(rng.integers(1, 4))
    mode = int(rng.integers(0, 4))
    # the list of every mesh, in rxr_set_meshes order
    slots = []
    for c in range(n_chunks):
        n_op, n_ch = int(rng.integers(0, 3)), int(rng.integers(1, 5))
        if c == 0 and mode == 1:
            n_op, n_ch = 1, max(n_ch, 2)
        if c == 0 and mode == 2:
            n_op, n_ch = 2, 4
        slots += [(R.LIST_CHUNK_OPACITY, c)] * n_op + [(R.LIST_CHUNK, c)] * n_ch + [(R.LIST_CHUNK_TERRAIN, c)] * int(rng.integers(0, 2))
    rest = max(n_meshes - len(slots), 3)
    cut = np.sort(rng.integers(0, rest + 1, 2))
    per = [int(cut[0]), int(cut[1] - cut[0]), int(rest - cut[1])]
    if per[2] == 0:     # (always an overlay mesh)
        big = int(np.argmax(per[:2]))
        per[2], per[big] = 1, per[big] - 1
    for lst, k in zip((R.LIST_STATIC, R.LIST_DYNAMIC, R.LIST_OVERLAY), per):
        slots += [(lst, -1)] * k
    if rng.random() < 0.5 and len(slots) < 52:   # more chunk meshes in some seeds: runs of profile-id segments
        at = max(i for i, s in enumerate(slots) if s[0] == R.LIST_CHUNK) + 1
        slots[at:at] = [(R.LIST_CHUNK, slots[at - 1][1])] * int(rng.integers(2, 8))
    # forced sizes and profile ids (None: no id) of the first meshes
    forced = {}
    if mode == 1:       # segments that end at 1024 and 2048 global triangles: opacity 1023 + chunk 1 (one plain run), chunk 1024 with an id
        forced = {0: (1023, None), 1: (1, None), 2: (1024, 1)}
    elif mode == 2:     # meshes without triangles before, inside and after a plain run (opacity, opacity, chunk x 4)
        forced = {0: (0, None), 1: (7, None), 2: (0, None), 3: (64, None), 4: (0, None), 5: (5, 2)}
    meshes, total = [], 0
    for i, (lst, chunk) in enumerate(slots):
        pid = int(rng.integers(0, 3)) if rng.random() < (0.7 if lst == R.LIST_CHUNK else 0.4) else None
        if i in forced:
            n, pid = forced[i]
        elif rng.random() < 0.45:
            n = int(rng.choice(EDGE_SIZES))
        else:
            n = int(rng.integers(1, 40))
        if i not in forced and total + n > MAX_TRIANGLES:
            n = int(rng.integers(1, 12))
        total += n
        copies = [m for m in meshes if 0 < len(m["indices"]) <= 300]
        if i not in forced and copies and rng.random() < 0.2:
            # the exact geometry of an earlier mesh under this slot's list and profile id: equal t across meshes and segments
            src = copies[int(rng.integers(len(copies)))]
            total += len(src["indices"]) - n
            meshes.append(dict(src, list=int(lst), chunk=int(chunk), has_pid=pid is not None, pid=0 if pid is None else pid))
            continue
        meshes.append(_random_mesh(rng, n, eyes, list=lst, chunk=chunk, pid=pid))
    return meshes


def random_rays(meshes, seed, n):
    """n rays, un-normalised (lengths 1e-3 .. 1e3): two thirds aimed at centroids, edge midpoints and vertices of random triangles
    from the scene's eyes, the rest in random directions; one in 50 with a special value in one coordinate"""
    rng = np.random.default_rng([SEED_KEY, 4244, seed])
    eyes = scene_eyes(seed)
    live = [m for m in meshes if len(m["indices"])]
    o = eyes[rng.integers(0, len(eyes), n)].copy()
    d = rng.standard_normal((n, 3)).astype(F)
    aimed = rng.random(n) < 2.0 / 3.0
    which, kind, tri = rng.integers(0, max(len(live), 1), n), rng.integers(0, 3, n), rng.random(n)
    if live:
        for r in np.nonzero(aimed)[0]:
            m = live[which[r]]
            k = int(tri[r] * len(m["indices"]))
            v = m["vertices"][m["indices"][k].astype(np.int64), :3]
            target = (v[0] + v[1] + v[2]) / F(3.0) if kind[r] == 0 else (v[0] + v[1]) * F(0.5) if kind[r] == 1 else v[0]
            d[r] = target - o[r]
    with np.errstate(all="ignore"):
        length = np.sqrt((d.astype(np.float64) ** 2).sum(axis=1))
        scale = 10.0 ** rng.uniform(-3.0, 3.0, n) / np.where(length > 0, length, 1.0)
        d = (d * scale[:, None]).astype(F)
    special = np.nonzero(rng.random(n) < 0.02)[0]
    vals, where, coord = rng.integers(0, len(SPECIALS), n), rng.random(n) < 0.7, rng.integers(0, 3, n)
    for r in special:
        (d if where[r] else o)[r, coord[r]] = F(SPECIALS[vals[r]])
    return np.ascontiguousarray(o, F), np.ascontiguousarray(d, F)


def host_scene(api, meshes):
    """the scene through the host mirror (meshes without vertices cannot be pushed there: see PickContext)"""
    scene = api.Scene.empty()
    chunks = {}
    for m in meshes:
        b = api.Batch3D.new(m["vertices"], m["indices"], m["uvs"]).normals(m["normals"])
        if m.get("has_pid"):
            b.profile_id(m["pid"])
        if m.get("transform") is not None:
            b.transform(m["transform"])
        lst = m["list"]
        if lst in (R.LIST_CHUNK_OPACITY, R.LIST_CHUNK, R.LIST_CHUNK_TERRAIN):
            while m["chunk"] not in chunks:
                chunks[len(chunks)] = scene.add_chunk()
            ch = chunks[m["chunk"]]
            {R.LIST_CHUNK_OPACITY: ch.add_batch3d_opacity, R.LIST_CHUNK: ch.add_batch3d, R.LIST_CHUNK_TERRAIN: ch.terrain_batch3d}[lst](b)
        else:
            {R.LIST_STATIC: scene.add_d3_static, R.LIST_DYNAMIC: scene.add_d3_dynamic, R.LIST_OVERLAY: scene.add_d3_overlay}[lst](b)
    return scene


IDENTITY = (C.c_float * 16)(*np.eye(4, dtype=F).ravel())


def mesh_array(meshes):
    """(the rxr_mesh3d array, the numpy arrays it points into)"""
    arr = (Mesh3D * max(len(meshes), 1))()
    keep = []
    for a, m in zip(arr, meshes):
        v, i, uv, nr = (np.ascontiguousarray(m[k], t) for k, t in (("vertices", F), ("indices", np.uint32), ("uvs", F), ("normals", F)))
        keep += [v, i, uv, nr]
        a.vertices, a.indices, a.uvs, a.normals = v.ctypes.data, i.ctypes.data, uv.ctypes.data, nr.ctypes.data
        a.n_vertices, a.n_triangles = len(v.reshape(-1, 4)), len(i.reshape(-1, 3))
        a.transform_3d = IDENTITY if m.get("transform") is None else (C.c_float * 16)(*m["transform"])
        a.shader = -1
        a.has_profile_id, a.profile_id = (1, m["pid"]) if m.get("has_pid") else (0, 0)
        a.list, a.chunk = m["list"], m.get("chunk", -1)
    return arr, keep


class PickContext:
    """a device context of its own (rxr_create) holding `meshes` through rxr_set_meshes: intersect as Scene.intersect returns it"""

    def __init__(self, meshes=None, device=0):
        import rusterix_amd

        self.rxr = rusterix_amd.rxr_abi()
        self.ctx = C.c_void_p()
        rc = self.rxr.rxr_create(C.byref(self.ctx), device)
        if rc != 0:
            raise RuntimeError(f"rxr_create failed ({rc})")
        if meshes is not None:
            self.set_meshes(meshes)

    def error(self):
        return (self.rxr.rxr_last_error(self.ctx) or b"").decode()

    def set_meshes(self, meshes):
        arr, keep = mesh_array(meshes)
        rc = self.rxr.rxr_set_meshes(self.ctx, C.cast(arr, C.c_void_p), len(meshes))
        assert rc == 0, f"rxr_set_meshes failed ({rc}): {self.error()}"
        del keep    # (copied by the call)

    def intersect(self, origins, dirs, full=False):
        o = np.ascontiguousarray(np.asarray(origins, F).reshape(-1, 3))
        d = np.ascontiguousarray(np.asarray(dirs, F).reshape(-1, 3))
        n = len(o)
        # (poisoned, so that an output the call leaves unwritten shows)
        out = dict(t=np.full(n, -7.0, F), mesh=np.full(n, 0xABABABAB, np.uint32), triangle=np.full(n, 0xABABABAB, np.uint32),
                   hitpoint=np.full((n, 3), -7.0, F))
        if full:
            out["uv"], out["normal"] = np.full((n, 2), -7.0, F), np.full((n, 3), -7.0, F)
        p = lambda k: out[k].ctypes.data if k in out else None
        rc = self.rxr.rxr_intersect(self.ctx, o.ctypes.data, d.ctypes.data, n, 1 if full else 0, p("t"), p("mesh"), p("triangle"),
                                    p("hitpoint"), p("uv"), p("normal"))
        assert rc == 0, f"rxr_intersect failed ({rc}): {self.error()}"
        return out

    def intersect_to(self, origins, dirs, full=False, stream=None):
        """rxr_intersect_to on torch tensors and `stream` (a torch stream; None: the context's); the outputs, not yet synchronised"""
        import torch

        n = len(origins)
        dev = dict(o=torch.from_numpy(np.ascontiguousarray(origins, F)).cuda(), d=torch.from_numpy(np.ascontiguousarray(dirs, F)).cuda())
        shapes = dict(t=(n,), mesh=(n,), triangle=(n,), hitpoint=(n, 3), **(dict(uv=(n, 2), normal=(n, 3)) if full else {}))
        for k, shp in shapes.items():
            dev[k] = torch.full(shp, -7, dtype=torch.int32 if k in ("mesh", "triangle") else torch.float32, device="cuda")
        torch.cuda.synchronize()    # (the fills above run on torch's stream)
        p = lambda k: dev[k].data_ptr() if k in dev else None
        rc = self.rxr.rxr_intersect_to(self.ctx, p("o"), p("d"), n, 1 if full else 0, p("t"), p("mesh"), p("triangle"), p("hitpoint"),
                                       p("uv"), p("normal"), stream.cuda_stream if stream is not None else None)
        assert rc == 0, f"rxr_intersect_to failed ({rc}): {self.error()}"
        return dev

    def close(self):
        if self.ctx:
            self.rxr.rxr_destroy(self.ctx)
            self.ctx = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def to_host(dev):
    """the outputs of PickContext.intersect_to as numpy arrays (after the stream was synchronised)"""
    return {k: (v.cpu().numpy().view(np.uint32) if k in ("mesh", "triangle") else v.cpu().numpy()) for k, v in dev.items() if k not in ("o", "d")}


def differences(got, ref, label=""):
    """None, or a description of the first output that is not `ref` bit for bit (NaN equals NaN)"""
    for k in ref:
        if not R.same(got[k], ref[k]):
            a, b = np.asarray(got[k]), np.asarray(ref[k])
            if a.dtype == np.float32:
                eq = (np.isnan(a) & np.isnan(b)) | (a.view(np.uint32) == b.view(np.uint32))
            else:
                eq = a == b
            bad = np.nonzero(~np.all(eq.reshape(len(ref["t"]), -1), axis=1))[0]
            r = int(bad[0])
            return (f"{label} {k}: {len(bad)} of {len(ref['t'])} rays differ; ray {r}: got {a[r]!r} (mesh {got['mesh'][r]}, triangle "
                    f"{got['triangle'][r]}), expected {b[r]!r} (mesh {ref['mesh'][r]}, triangle {ref['triangle'][r]})")
    return None


def prefix(res, n):
    return {k: v[:n] for k, v in res.items()}


def plain_of(res):
    """what a call without RXR_INTERSECT_FULL returns, from a full result (full mode changes no choice of hit)"""
    return {k: res[k] for k in ("t", "mesh", "triangle", "hitpoint")}


RAY_COUNTS = (1, 8, 9, 64, 65, 256, 257, 3000)


def check_seed(seed, ctx=None, n_rays=3000):
    """the device against intersect_many on random_pick_scene(seed): every count of RAY_COUNTS (prefixes of one ray set), plain and
    full; and rays 0..63 sent alone (k_isect_by_tri) against the same rays as part of 65 (k_isect_by_ray).  None or the first
    difference."""
    meshes = random_pick_scene(seed)
    o, d = random_rays(meshes, seed, n_rays)
    ref = R.intersect_many(meshes, o, d, full=True)
    own = ctx is None
    ctx = ctx or PickContext()
    try:
        ctx.set_meshes(meshes)
        got = {}
        for n in RAY_COUNTS:
            for full in (False, True):
                got[n, full] = ctx.intersect(o[:n], d[:n], full=full)
                want = prefix(ref if full else plain_of(ref), n)
                bad = differences(got[n, full], want, f"seed {seed}, {n} rays, full={full}:")
                if bad:
                    return bad
        for full in (False, True):
            bad = differences(prefix(got[65, full], 64), got[64, full], f"seed {seed}, rays 0..63 of 65 against 64 alone, full={full}:")
            if bad:
                return bad
    finally:
        if own:
            ctx.close()
    return None
