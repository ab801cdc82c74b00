"""numpy references and small builders for rxr_resize_meshes (include/rxr.h), on top of tests/mesh_update_ref.py: the caller's strided
arrays with the uv array the resize adds, meshes of other counts at the same place, and the layout arithmetic of rxr_set_meshes
(rusterix_amd/csrc/rxr_mesh_resize.h) restated over numpy integers."""
import numpy as np

from tests import mesh_update_ref as M

F = np.float32
SLOT_LIMIT = 1 << 31


def pack(meshes, vstride=None, tstride=None, slack=False):
    """mesh_update_ref.pack plus uvs [n][VS][2]: (counts, vertices, uvs, indices, normals); slack=True poisons the uv slack with NaN words too"""
    counts, vertices, indices, normals = M.pack(meshes, vstride=vstride, tstride=tstride, slack=slack)
    uvs = np.zeros((len(meshes), vertices.shape[1], 2), F)
    if slack:
        uvs.view(np.uint32)[:] = 0x7FC0BEEF
    for i, m in enumerate(meshes):
        uv = np.asarray(m["uvs"], F).reshape(-1, 2)[:vertices.shape[1]]
        uvs[i, :len(uv)] = uv
    return counts, vertices, uvs, indices, normals


def resized(mesh, nv, nt, seed, extent=1.0, centre=None):
    """a mesh of other counts where `mesh` was: new vertices, indices, uvs and normals; list, chunk and the rest as they were"""
    old_v = np.asarray(mesh["vertices"], F).reshape(-1, 4)
    c = centre if centre is not None else (old_v[:, :3].mean(axis=0) if len(old_v) else (0.0, 0.0, -6.0))
    new = M.grid_mesh(nv, nt, seed, centre=c, extent=extent, lst=mesh["list"])
    for k in mesh:
        new.setdefault(k, mesh[k])
    return new


def bases(counts):
    """rxr_resize_bases over counts [n][2] in Python integers: (reached, bases [n][4] as far as written, totals [4])"""
    vin = tin = vout = tout = 0
    out = np.zeros((len(counts), 4), np.uint32)
    reached = len(counts)
    for i, (nv, nt) in enumerate((int(a), int(b)) for a, b in counts):
        out[i] = (vin & 0xFFFFFFFF, tin & 0xFFFFFFFF, vout & 0xFFFFFFFF, tout & 0xFFFFFFFF)
        vin, tin, vout, tout = vin + nv, tin + nt, vout + nv + 4 * nt, tout + 3 * nt
        if vout >= SLOT_LIMIT or tout >= SLOT_LIMIT:
            reached = i
            break
    return reached, out, (vin, tin, vout, tout)


def bases_numpy(counts):
    """the same for counts that fit, as numpy prefix sums in 64 bits (the restatement the arithmetic is held to)"""
    c = np.asarray(counts, np.uint64).reshape(-1, 2)
    per = np.stack([c[:, 0], c[:, 1], c[:, 0] + np.uint64(4) * c[:, 1], np.uint64(3) * c[:, 1]], axis=1)
    incl = np.cumsum(per, axis=0, dtype=np.uint64)
    excl = incl - per
    return excl, (incl[-1] if len(c) else np.zeros(4, np.uint64))
