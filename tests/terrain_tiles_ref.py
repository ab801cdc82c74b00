"""A numpy-float32 transcription of the generated terrain's last step (reference src/chunkbuilder/terrain_generator.rs:
partition_by_tiles :954-1034 over the (vertices, indices, uvs) apply_exclusions returns, :747-825, uvs[i] = [v.x, v.z] :882-888) and of
what its consumer runs on every group (fix_winding, src/chunkbuilder/surface_mesh_builder.rs:201-239, called at
src/chunkbuilder/d3chunkbuilder.rs:1705 with the normal (0, 1, 0)), every operation rounded to f32, on top of
tests/terrain_exclusion_ref.apply_exclusions.  The vertex lists are built by the reference's dictionary walk; `first_use_closed_form`
is the closed form the device uses in its place (tests/test_terrain_tiles_cpu.py holds the two against each other).

The one thing this module defines and the reference does not: the groups of a box come in ASCENDING TILE SLOT (the reference
iterates a hash map).  The caller resolves pixel sources to tiles; here a cell has a tile SLOT, slot 0 being the default tile."""
import numpy as np

from tests import terrain_exclusion_ref as X
from tests.terrain_gen_ref import F, triangulate

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


class Tiles:
    """a tile override map {(x, z): slot}, flattened as rxr_set_terrain_tiles takes it (in the dict's order: the library sorts)"""

    def __init__(self, overrides=None, n_tiles=None):
        self.map = {(int(x), int(z)): int(s) for (x, z), s in (overrides or {}).items()}
        self.cells = np.array(list(self.map.keys()), np.int32).reshape(-1, 2)
        self.slots = np.array(list(self.map.values()), np.uint32)
        self.n_tiles = int(n_tiles) if n_tiles is not None else int(max(self.map.values(), default=0)) + 1

    def args(self):
        """keyword arguments of the product's TerrainGenerator.set_tiles"""
        return dict(cells=self.cells, slots=self.slots, n_tiles=self.n_tiles)

    def slot(self, cell):
        return self.map.get(cell, 0)


def floor_as_i32(x):
    """`x.floor() as i32` over an array: saturating, a NaN is 0"""
    with np.errstate(all="ignore"):
        f = np.floor(np.asarray(x, F)).astype(np.float64)
    f = np.where(np.isnan(f), 0.0, np.clip(f, I32_MIN, I32_MAX))
    return f.astype(np.int64)


def mesh_of(res):
    """(grid point of every vertex [V], indices [T][3]) as apply_exclusions returns them: the shared layout with triangulate's indices,
    or the unshared one (a kept triangle's three vertices one after the other)"""
    sx, sy = res["counts"][0], res["counts"][1]
    if res["keep"] is None:
        tris = triangulate(sx, sy) if sx > 0 and sy > 0 else np.zeros((0, 3), np.uint32)
        return np.arange(sx * sy, dtype=np.int64), tris.astype(np.int64)
    v = res["vertex_points"]
    return v, np.arange(len(v), dtype=np.int64).reshape(-1, 3)


def triangle_cells(uvs, indices):
    """:972-980 for every triangle: the tile cell [T][2]"""
    uv = np.asarray(uvs, F)[indices]   # [T][3][2]
    with np.errstate(all="ignore"):
        center = ((uv[:, 0] + uv[:, 1]).astype(F) + uv[:, 2]).astype(F) / F(3.0)
    return floor_as_i32(center.astype(F))


def partition_by_tiles(uvs, indices, tiles):
    """:954-1034.  Returns the groups in ascending slot: dicts of slot, triangles (ids into `indices`, ascending), vertex_ids (the old
    index of every new vertex, in first-use order) and indices [t][3] (remapped)"""
    cells = triangle_cells(uvs, indices) if len(indices) else np.zeros((0, 2), np.int64)
    per_tile = {}
    for t, (cu, cv) in enumerate(cells):
        per_tile.setdefault(tiles.slot((int(cu), int(cv))), []).append(t)
    out = []
    for slot in sorted(per_tile):
        remap, vertex_ids, remapped = {}, [], []
        for t in per_tile[slot]:
            for old in indices[t]:
                old = int(old)
                if old not in remap:
                    remap[old] = len(vertex_ids)
                    vertex_ids.append(old)
                remapped.append(remap[old])
        out.append(dict(slot=slot, triangles=np.array(per_tile[slot], np.int64), vertex_ids=np.array(vertex_ids, np.int64),
                        indices=np.array(remapped, np.uint32).reshape(-1, 3)))
    return out


def tile_meshes(gen, excl, tiles, box):
    """one chunk box through apply_exclusions and partition_by_tiles.  Returns the apply_exclusions dict with box_counts = (steps_x,
    steps_y, active_sectors, n_groups) and groups: per group slot, points (the GRID POINT of every vertex, in order: x and z are
    res["points"][points], y is that grid point's height), uvs [V][2], indices [T][3], triangles (ids in triangulate's order)"""
    res = X.apply_exclusions(gen, excl, box)
    vertex_points, indices = mesh_of(res)
    pts = res["points"]
    uvs = pts[vertex_points] if len(vertex_points) else np.zeros((0, 2), F)
    groups = partition_by_tiles(uvs, indices, tiles)
    kept = np.nonzero(res["keep"])[0] if res["keep"] is not None else np.arange(len(indices))
    for g in groups:
        g["points"] = vertex_points[g["vertex_ids"]]
        g["uvs"] = pts[g["points"]]
        g["triangles"] = kept[g["triangles"]]
    res["groups"] = groups
    res["box_counts"] = res["counts"][:3] + (len(groups),)
    return res


def first_use_closed_form(sx, sy, tri_slot):
    """the shared layout's vertex lists without a dictionary.  tri_slot [2 * cells]: every triangle's slot in triangulate's order.  A
    grid point (ix, iy) is named by at most six triangles, in ascending order: cell (ix-1, iy-1) triangle 1, cell (ix, iy-1) triangles
    0 and 1, cell (ix-1, iy) triangles 0 and 1, cell (ix, iy) triangle 0; a corner is a first use in its group iff no earlier one of
    them has the same slot.  Returns {slot: (vertex grid points in first-use order, indices [t][3])}"""
    cw, ch = sx - 1, sy - 1
    corners = {0: ((0, 0), (0, 1), (1, 0)), 1: ((1, 0), (0, 1), (1, 1))}   # (i0, i2, i1) and (i1, i2, i3) as cell offsets

    def users(ix, iy):
        for cx, cy, k in ((ix - 1, iy - 1, 1), (ix, iy - 1, 0), (ix, iy - 1, 1), (ix - 1, iy, 0), (ix - 1, iy, 1), (ix, iy, 0)):
            if 0 <= cx < cw and 0 <= cy < ch:
                yield 2 * (cy * cw + cx) + k

    def corner_points(t):
        cell, k = divmod(t, 2)
        cy, cx = divmod(cell, cw)
        return [(cx + dx, cy + dy) for dx, dy in corners[k]]

    def first_user(ix, iy, slot):
        return next(u for u in users(ix, iy) if tri_slot[u] == slot)

    n = 2 * cw * ch
    first = [[first_user(ix, iy, tri_slot[t]) == t for ix, iy in corner_points(t)] for t in range(n)]
    base, running = [0] * n, {}
    for t in range(n):   # (the device's ordered scan)
        base[t] = running.get(tri_slot[t], 0)
        running[tri_slot[t]] = base[t] + sum(first[t])
    out = {}
    for slot in sorted(set(tri_slot)):
        verts, idx = [], []
        for t in range(n):
            if tri_slot[t] != slot:
                continue
            for j, (ix, iy) in enumerate(corner_points(t)):
                if first[t][j]:
                    verts.append(iy * sx + ix)
                u = first_user(ix, iy, slot)
                c = corner_points(u).index((ix, iy))
                idx.append(base[u] + sum(first[u][:c]))
        out[slot] = (np.array(verts, np.int64), np.array(idx, np.uint32).reshape(-1, 3))
    return out


# ---- fix_winding (surface_mesh_builder.rs:201-239) ----
def fix_winding(vertices, indices, desired_normal=(0.0, 1.0, 0.0)):
    """vertices [V][4] f32, indices [T][3].  Returns (indices, swapped): the reference swaps the second and third index of EVERY
    triangle when the normalised sum of the first eight triangles' cross products points against desired_normal"""
    v = np.asarray(vertices, F)
    idx = np.array(indices, np.int64).reshape(-1, 3)
    if len(idx) == 0 or len(v) < 3:
        return idx, False
    with np.errstate(all="ignore"):
        avg = [F(0.0), F(0.0), F(0.0)]
        for a, b, c in idx[:min(len(idx), 8)]:
            if a >= len(v) or b >= len(v) or c >= len(v):
                continue
            e1 = [F(v[b][k] - v[a][k]) for k in range(3)]
            e2 = [F(v[c][k] - v[a][k]) for k in range(3)]
            cross = [F(F(e1[1] * e2[2]) - F(e1[2] * e2[1])), F(F(e1[2] * e2[0]) - F(e1[0] * e2[2])), F(F(e1[0] * e2[1]) - F(e1[1] * e2[0]))]
            avg = [F(avg[k] + cross[k]) for k in range(3)]
        mag = F(np.sqrt(F(F(F(avg[0] * avg[0]) + F(avg[1] * avg[1])) + F(avg[2] * avg[2]))))
        if mag < F(1e-8):
            return idx, False
        avg = [F(a / mag) for a in avg]
        d = [F(x) for x in desired_normal]
        if F(F(F(avg[0] * d[0]) + F(avg[1] * d[1])) + F(avg[2] * d[2])) < F(0.0):
            return idx[:, [0, 2, 1]], True
    return idx, False


# ---- the tile maps the CPU and the GPU tests share ----
def stripes(x0, x1, z0, z1, n_slots, width=1, vertical=True):
    """cells [x0, x1) x [z0, z1) in stripes of `width` cells, slots 0 .. n_slots - 1 in turn (slot 0 is left to the default)"""
    out = {}
    for x in range(x0, x1):
        for z in range(z0, z1):
            s = ((x - x0 if vertical else z - z0) // width) % n_slots
            if s:
                out[(x, z)] = s
    return out


def checkerboard(x0, x1, z0, z1, n_slots):
    return {(x, z): (x + 2 * z) % n_slots for x in range(x0, x1) for z in range(z0, z1) if (x + 2 * z) % n_slots}


def fuzz_tiles(seed):
    """random slots 1..5 on about 600 cells of [-2, 66)^2, four-slot stripes over [0, 16) x [48, 64) and a three-slot checkerboard
    over [48, 64) x [0, 16) (two of the chunk boxes of tests/terrain_exclusion_ref.fuzz_scene)"""
    rng = np.random.default_rng([0x7E44E8, seed])
    cells = rng.integers(-2, 66, (600, 2))
    slots = rng.integers(1, 6, 600)
    out = {(int(x), int(z)): int(s) for (x, z), s in zip(cells, slots)}
    for x in range(0, 16):
        for z in range(48, 64):
            out.pop((x, z), None)
    for x in range(48, 64):
        for z in range(0, 16):
            out.pop((x, z), None)
    out.update(stripes(0, 16, 48, 64, 4))
    out.update(checkerboard(48, 64, 0, 16, 3))
    return Tiles(out, n_tiles=6)
