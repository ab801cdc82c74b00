"""numpy float32 restatement of Scene::intersect (reference src/scene.rs:216-276) over Batch3D::intersect (src/batch/batch3d.rs:844-948),
the ground truth of tests/test_intersect_cpu.py, tests/test_gpu_intersect.py, tests/test_gpu_intersect_fuzz.py and
tools/intersect_bench.py's CPU baseline: `intersect` a ray at a time, `intersect_many` the same bits for all rays at once.

Every operation is one IEEE float32 operation in the reference's order (numpy neither contracts nor reorders), so the device must
agree bit for bit.  Meshes are dicts with `vertices` [n][4], `indices` [m][3], `uvs` [n][2], `normals` [n][3], `list` (RXR_LIST_*),
`has_pid`, `pid`, in rxr_set_meshes order."""
import contextlib

import numpy as np

F = np.float32
LIST_CHUNK_OPACITY, LIST_CHUNK, LIST_CHUNK_TERRAIN, LIST_STATIC, LIST_DYNAMIC, LIST_OVERLAY = range(6)
FLT_MAX = np.finfo(np.float32).max
MISS = 0xFFFFFFFF


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def normalized(a):
    return a / np.sqrt(dot(a, a))[..., None]


def tri_records(mesh):
    """(p0, edge1, edge2) per triangle, object space (transform_3d is ignored, as in the reference)"""
    v = np.asarray(mesh["vertices"], F).reshape(-1, 4)[:, :3]
    i = np.asarray(mesh["indices"], np.int64).reshape(-1, 3)
    p0, p1, p2 = v[i[:, 0]], v[i[:, 1]], v[i[:, 2]]
    return p0, p1 - p0, p2 - p0


def mt(o, d, p0, e1, e2):
    """Moeller-Trumbore of one ray (o, normalised d: [3]) against triangles [m]: (accepted mask, t, u, v)"""
    with np.errstate(all="ignore"):
        h = cross(d[None, :], e2)
        a = dot(e1, h)
        ok = ~(np.abs(a) < F(1e-6))
        f = F(1.0) / a
        s = o[None, :] - p0
        u = f * dot(s, h)
        ok &= (u >= F(0.0)) & (u <= F(1.0))
        q = cross(s, e1)
        v = f * dot(d[None, :], q)
        ok &= ~((v < F(0.0)) | (u + v > F(1.0)))
        t = f * dot(e2, q)
        ok &= t > F(1e-4)
    return ok, t, u, v


def mesh_hit(rec, o, d):
    """Batch3D::intersect's closest hit: (t, triangle, u, v) or None (strict <: the earliest triangle on equal t)"""
    p0, e1, e2 = rec
    if len(p0) == 0:
        return None
    ok, t, u, v = mt(o, d, p0, e1, e2)
    idx = np.nonzero(ok)[0]
    if len(idx) == 0:
        return None
    tt = t[idx]
    k = idx[np.argmin(tt)]  # (argmin: the first minimum)
    return t[k], int(k), u[k], v[k]


def intersect(meshes, origins, dirs, full=False, records=None):
    """Scene::intersect for every ray: dict of t, mesh, triangle, hitpoint (+ uv, normal)"""
    origins = np.asarray(origins, F).reshape(-1, 3)
    dirs = np.asarray(dirs, F).reshape(-1, 3)
    n = len(origins)
    recs = records if records is not None else [tri_records(m) for m in meshes]
    out = dict(t=np.full(n, FLT_MAX, F), mesh=np.full(n, MISS, np.uint32), triangle=np.zeros(n, np.uint32),
               hitpoint=np.zeros((n, 3), F))
    if full:
        out["uv"] = np.zeros((n, 2), F)
        out["normal"] = np.zeros((n, 3), F)
    for r in range(n):
        o, dir_ = origins[r], dirs[r]
        with np.errstate(all="ignore"):
            d = normalized(dir_)
        best_t, best_m, best_tri, best_pid, best_uv = FLT_MAX, MISS, 0, None, None
        for mi, m in enumerate(meshes):
            hit = mesh_hit(recs[mi], o, d)
            if hit is None:
                continue
            t, k, u, v = hit
            pid = m["pid"] if m.get("has_pid") else None
            lst = m["list"]
            if lst == LIST_OVERLAY:
                take = True
            elif lst == LIST_CHUNK:
                take = t < best_t and not (pid is not None and pid == best_pid)
            else:
                take = t < best_t
            if take:
                best_t, best_m, best_tri, best_pid, best_uv = t, mi, k, pid, (u, v)
        if best_m == MISS:
            continue
        out["t"][r], out["mesh"][r], out["triangle"][r] = best_t, best_m, best_tri
        with np.errstate(all="ignore"):
            out["hitpoint"][r] = o + dir_ * best_t
            if full:
                m = meshes[best_m]
                u, v = best_uv
                w = (F(1.0) - u) - v
                i0, i1, i2 = (int(x) for x in np.asarray(m["indices"]).reshape(-1, 3)[best_tri])
                uvs = np.asarray(m["uvs"], F).reshape(-1, 2)
                out["uv"][r] = (w * uvs[i0] + u * uvs[i1]) + v * uvs[i2]
                nr = np.asarray(m["normals"], F).reshape(-1, 3)
                nn = normalized((nr[i0] * w + nr[i1] * u) + nr[i2] * v)
                if dot(nn, dir_) > F(0.0):
                    nn = -nn
                out["normal"][r] = nn
    return out


def same(a, b):
    """bitwise equality; any NaN equals any NaN (the device's default NaN is positive, x86's negative)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return False
    if a.dtype == np.float32:
        nan = np.isnan(a) & np.isnan(b)
        return bool(np.all(nan | (a.view(np.uint32) == b.view(np.uint32))))
    return bool(np.array_equal(a, b))


NO_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)


def intersect_many(meshes, origins, dirs, full=False, max_pairs=4_000_000):
    """`intersect`, vectorised over rays: the same float32 operations in the same order on [rays, triangles] arrays (blocks of rays,
    at most `max_pairs` ray-triangle pairs at a time), so the same bits -- tests/test_intersect_cpu.py pins it to `intersect`.

    Per mesh the closest accepted hit is the minimum of (t's unsigned bits, triangle index): an accepted t is > 1e-4, so it orders
    like its bits, +inf (huge coordinates) included -- it beats a rejected triangle and loses to every finite t -- and the index
    makes the first triangle win on equal t.  The fold over the meshes is `intersect`'s, a ray per array element; full mode uses the
    u and v of the winning test."""
    origins = np.ascontiguousarray(np.asarray(origins, F).reshape(-1, 3))
    dirs = np.ascontiguousarray(np.asarray(dirs, F).reshape(-1, 3))
    n = len(origins)
    out = dict(t=np.full(n, FLT_MAX, F), mesh=np.full(n, MISS, np.uint32), triangle=np.zeros(n, np.uint32),
               hitpoint=np.zeros((n, 3), F))
    if full:
        out["uv"] = np.zeros((n, 2), F)
        out["normal"] = np.zeros((n, 3), F)
    recs = [tri_records(m) for m in meshes]
    counts = np.array([len(r[0]) for r in recs], np.int64)
    live = np.nonzero(counts)[0]            # (a mesh without triangles is never hit)
    if n == 0 or len(live) == 0:
        return out
    p0, e1, e2 = (np.concatenate([recs[i][k] for i in live]) for k in range(3))
    ntri = len(p0)
    starts = np.concatenate([[0], np.cumsum(counts[live])[:-1]]).astype(np.int64)
    local = np.arange(ntri, dtype=np.int64) - np.repeat(starts, counts[live])
    lists = [int(meshes[i]["list"]) for i in live]
    has = [bool(meshes[i].get("has_pid")) for i in live]
    pids = [int(meshes[i].get("pid", 0)) for i in live]
    if full:
        nverts = [len(np.asarray(meshes[i]["vertices"]).reshape(-1, 4)) for i in live]
        vbase = np.concatenate([[0], np.cumsum(nverts)[:-1]]).astype(np.int64)
        idx = np.concatenate([np.asarray(meshes[i]["indices"], np.int64).reshape(-1, 3) + vb for i, vb in zip(live, vbase)])
        uvs = np.concatenate([np.asarray(meshes[i]["uvs"], F).reshape(-1, 2) for i in live])
        nrm = np.concatenate([np.asarray(meshes[i]["normals"], F).reshape(-1, 3)[:nv] for i, nv in zip(live, nverts)])
    tri_ids = np.arange(ntri, dtype=np.uint64)
    block = max(1, int(max_pairs) // ntri)
    for b0 in range(0, n, block):
        o, dr = origins[b0:b0 + block], dirs[b0:b0 + block]
        nb = len(o)
        with np.errstate(all="ignore"):
            d = normalized(dr)
            # Batch3D::intersect's test, every ray of the block against every triangle (`mt`, one more axis)
            h = cross(d[:, None, :], e2[None, :, :])
            a = dot(e1[None, :, :], h)
            ok = ~(np.abs(a) < F(1e-6))
            f = F(1.0) / a
            s = o[:, None, :] - p0[None, :, :]
            u = f * dot(s, h)
            ok &= (u >= F(0.0)) & (u <= F(1.0))
            q = cross(s, e1[None, :, :])
            del s, h
            v = f * dot(d[:, None, :], q)
            ok &= ~((v < F(0.0)) | (u + v > F(1.0)))    # (a NaN v does not reject)
            t = np.ascontiguousarray(f * dot(e2[None, :, :], q))
            del q, f, a
            ok &= t > F(1e-4)
            key = np.where(ok, (t.view(np.uint32).astype(np.uint64) << np.uint64(32)) | tri_ids[None, :], NO_KEY)
            del ok, t
            kmin = np.minimum.reduceat(key, starts, axis=1)    # [rays, live meshes]
            del key
            bt = np.full(nb, FLT_MAX, F)
            bm = np.full(nb, -1, np.int64)      # (index into `live`)
            bg = np.zeros(nb, np.int64)
            bhas = np.zeros(nb, bool)
            bpid = np.zeros(nb, np.int64)
            for j in np.nonzero((kmin != NO_KEY).any(axis=0))[0]:
                k = kmin[:, j]
                hit = k != NO_KEY
                tj = (k >> np.uint64(32)).astype(np.uint32).view(F)
                if lists[j] == LIST_OVERLAY:
                    take = hit
                else:
                    take = hit & (tj < bt)
                    if lists[j] == LIST_CHUNK and has[j]:
                        take &= ~(bhas & (bpid == pids[j]))
                bt = np.where(take, tj, bt)
                bm = np.where(take, j, bm)
                bg = np.where(take, (k & np.uint64(0xFFFFFFFF)).astype(np.int64), bg)
                bhas = np.where(take, has[j], bhas)
                bpid = np.where(take, pids[j], bpid)
            hit = bm >= 0
            rows = np.nonzero(hit)[0]
            g = bg[rows]
            sl = slice(b0, b0 + nb)
            out["t"][sl] = bt
            out["mesh"][sl][rows] = live[bm[rows]]
            out["triangle"][sl][rows] = local[g]
            out["hitpoint"][sl][rows] = o[rows] + dr[rows] * bt[rows, None]
            if full and len(rows):
                uu, vv = u[rows, g][:, None], v[rows, g][:, None]
                w = (F(1.0) - uu) - vv
                i0, i1, i2 = idx[g, 0], idx[g, 1], idx[g, 2]
                out["uv"][sl][rows] = (w * uvs[i0] + uu * uvs[i1]) + vv * uvs[i2]
                nn = normalized((nrm[i0] * w + nrm[i1] * uu) + nrm[i2] * vv)
                flip = dot(nn, dr[rows]) > F(0.0)
                out["normal"][sl][rows] = np.where(flip[:, None], -nn, nn)
            del u, v
    return out


_ORDER = {LIST_CHUNK_OPACITY: 0, LIST_CHUNK: 1, LIST_CHUNK_TERRAIN: 2}


@contextlib.contextmanager
def recording(api):
    """Records every 3D batch pushed into a scene of `api` (with its profile id) so that `meshes_of(scene)` can list the scene's
    meshes in rxr_set_meshes order: per chunk opacity, batches, terrain; then static, dynamic, overlay."""
    raw = api.raw
    push, set_pid, free = raw.scene_push_batch3d, raw.batch3d_set_profile_id, raw.batch3d_free
    pids, log = {}, {}

    def set_pid_rec(h, has, pid):
        pids[h] = (bool(has), int(pid))
        return set_pid(h, has, pid)

    def free_rec(h):
        pids.pop(h, None)  # (a later batch may get the same address)
        return free(h)

    def push_rec(sh, bh, lst, chunk):
        rc = push(sh, bh, lst, chunk)
        if rc == 0:
            b = api.Batch3D.__new__(api.Batch3D)
            b._h = bh
            v, i, uv, n = b.geometry()
            b._h = None  # (not owned)
            has, pid = pids.get(bh, (False, 0))
            entries = log.setdefault(sh, [])
            if lst == LIST_CHUNK_TERRAIN:
                entries[:] = [e for e in entries if not (e["list"] == lst and e["chunk"] == chunk)]
            entries.append(dict(vertices=v, indices=i, uvs=uv, normals=n, list=int(lst), chunk=int(chunk), has_pid=has, pid=pid))
        return rc

    raw.scene_push_batch3d, raw.batch3d_set_profile_id, raw.batch3d_free = push_rec, set_pid_rec, free_rec

    def meshes_of(scene):
        entries = log.get(scene._h, [])
        key = lambda e: (0, e["chunk"], _ORDER[e["list"]]) if e["list"] in _ORDER else (1, e["list"] - LIST_STATIC, 0)
        return sorted(entries, key=key)  # (stable: insertion order within a list)

    try:
        yield meshes_of
    finally:
        raw.scene_push_batch3d, raw.batch3d_set_profile_id, raw.batch3d_free = push, set_pid, free
