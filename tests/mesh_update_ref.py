"""numpy references and small builders for the in-place mesh update (rxr_update_meshes, include/rxr.h): the object-space box with
f32::min / f32::max semantics (np.fmin / np.fmax drop a NaN operand, as the host loop's std::fmin / std::fmax and the kernel's
fminf / fmaxf do), the caller's strided arrays, and what the packed pools must hold afterwards.

A mesh is a dict in tests/intersect_ref.py's form: vertices [n][4], indices [m][3], uvs [n][2], normals [n][3], list (+ chunk ...)."""
import numpy as np

F = np.float32


def box(vertices):
    """(lo[3], hi[3]) over the xyz of vertices [n][4]: from +inf / -inf, a NaN coordinate ignored (batch3d.rs:494-507)"""
    v = np.asarray(vertices, F).reshape(-1, 4)
    lo, hi = np.full(3, np.inf, F), np.full(3, -np.inf, F)
    for p in v:            # (the host loop's order; min and max do not depend on it for non-NaN values, up to the sign of zero)
        lo = np.fmin(lo, p[:3])
        hi = np.fmax(hi, p[:3])
    return lo, hi


def box_fast(vertices):
    """the same without the Python loop (large meshes)"""
    v = np.asarray(vertices, F).reshape(-1, 4)[:, :3]
    if not len(v):
        return np.full(3, np.inf, F), np.full(3, -np.inf, F)
    return (np.fmin.reduce(np.concatenate([v, np.full((1, 3), np.inf, F)]), axis=0),
            np.fmax.reduce(np.concatenate([v, np.full((1, 3), -np.inf, F)]), axis=0))


def pack(meshes, vstride=None, tstride=None, slack=False):
    """the caller's arrays for an update to `meshes` (a list): counts [n][2], vertices [n][VS][4], indices [n][TS][3], normals
    [n][VS][3].  Strides default to the largest counts.  slack=True fills the slots past each mesh's counts with what must never be
    read: 0xFFFFFFFF indices, NaN / 1e30 vertices and normals."""
    n = len(meshes)
    nv = [len(np.asarray(m["vertices"]).reshape(-1, 4)) for m in meshes]
    nt = [len(np.asarray(m["indices"]).reshape(-1, 3)) for m in meshes]
    vs = max(nv + [0]) if vstride is None else vstride
    ts = max(nt + [0]) if tstride is None else tstride
    counts = np.array(list(zip(nv, nt)), np.uint32).reshape(n, 2)
    vertices, normals = np.zeros((n, vs, 4), F), np.zeros((n, vs, 3), F)
    indices = np.zeros((n, ts, 3), np.uint32)
    if slack:
        vertices[:] = np.array([np.nan, 1e30, -1e30, np.nan], F)
        normals[:] = np.array([np.nan, 1e30, -1e30], F)
        indices[:] = 0xFFFFFFFF
    for i, m in enumerate(meshes):   # (a stride below a count -- a call the library refuses unread -- cuts the mesh off; counts stay)
        vertices[i, :nv[i]] = np.asarray(m["vertices"], F).reshape(-1, 4)[:vs]
        normals[i, :nv[i]] = np.asarray(m["normals"], F).reshape(-1, 3)[:vs]
        indices[i, :nt[i]] = np.asarray(m["indices"], np.uint32).reshape(-1, 3)[:ts]
    return counts, vertices, indices, normals


def expected_pools(meshes):
    """the packed object-space pools rxr_set_meshes lays out for `meshes`: vertices [sum nv][4], indices [sum nt][3] (mesh-local),
    normals [sum nv][3] -- what they must hold after any sequence of updates that ends in this geometry"""
    v = [np.asarray(m["vertices"], F).reshape(-1, 4) for m in meshes]
    i = [np.asarray(m["indices"], np.uint32).reshape(-1, 3) for m in meshes]
    nr = [np.asarray(m["normals"], F).reshape(-1, 3) for m in meshes]
    return np.concatenate(v), np.concatenate(i), np.concatenate(nr)


# ---- small meshes -----------------------------------------------------------------------------------------------------------------------
def grid_mesh(nv, nt, seed, centre=(0.0, 0.0, -6.0), extent=2.0, lst=3):
    """nv vertices scattered in a box of half-size `extent` around `centre`, nt triangles over seeded vertex triples, unit normals"""
    rng = np.random.default_rng(seed)
    v = np.ones((nv, 4), F)
    v[:, :3] = (rng.random((nv, 3), dtype=F) * 2 - 1) * F(extent) + np.asarray(centre, F)
    idx = rng.integers(0, max(nv, 1), (nt, 3)).astype(np.uint32)
    nr = rng.standard_normal((nv, 3)).astype(F)
    nr /= np.maximum(np.linalg.norm(nr, axis=1, keepdims=True), F(1e-6))
    return dict(vertices=v, indices=idx, uvs=rng.random((nv, 2), dtype=F), normals=nr.astype(F), list=lst)


def moved(mesh, seed, centre=None, extent=None):
    """the same counts and uvs, new vertices, indices and normals"""
    nv, nt = len(mesh["vertices"]), len(mesh["indices"])
    c = np.asarray(mesh["vertices"], F)[:, :3].mean(axis=0) if centre is None and nv else (centre if centre is not None else (0, 0, -6))
    e = 2.0 if extent is None else extent
    new = grid_mesh(nv, nt, seed, centre=c, extent=e, lst=mesh["list"])
    new["uvs"] = mesh["uvs"]
    for k in mesh:
        new.setdefault(k, mesh[k])
    return new
