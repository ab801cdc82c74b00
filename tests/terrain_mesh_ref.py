"""Ground truth of the terrain chunk mesh: TerrainChunk::build_mesh (reference src/terrain/chunk.rs:253-297) as a dictionary
transcription in Python / numpy float32 with the cells visited in ascending (ly, lx), row by row -- the order DESIGN.md section 13
fixes in place of the reference's hash order -- and its normals from the oracle's batch3d_compute_vertex_normals
(oracle/rusterix_oracle.cpp:329-350) through tests/oracle_api.py.  Nothing here uses the code under test.

A terrain is a tests/terrain_hit_ref.py HeightSpec: its `heights` keys are the present cells (what the caller lists in
rxr_set_terrain_heights; the mirror's Terrain.heights), `get_height` is Terrain::get_height.

`closed_form` is the second statement of the same mesh -- owner, scan and incident-triangle order, as the kernel computes it -- in
plain Python over a presence mask; tests/test_terrain_mesh_cpu.py holds the two against each other."""
import numpy as np

from tests.terrain_hit_ref import F, HeightSpec

CORNERS = ((0, 0), (1, 0), (0, 1), (1, 1))


def present_mask(spec, coord, cs):
    """[cs][cs] bool: cell (lx, ly) of chunk `coord` is a key of the heights"""
    ox, oy = coord[0] * cs, coord[1] * cs
    m = np.zeros((cs, cs), bool)
    for ly in range(cs):
        for lx in range(cs):
            m[ly, lx] = (ox + lx, oy + ly) in spec.heights
    return m


def transcription(mask):
    """:253-291 over a presence mask in row-major order, in chunk-local corners: (corners, triangles, incident) with corners a list of
    (px, py) by vertex index, triangles a list of index triples and incident[v] the triangles of vertex v in the order
    compute_vertex_normals adds them (ascending triangle index)"""
    cs = mask.shape[0]
    vertex_map, corners, triangles = {}, [], []
    for ly in range(cs):
        for lx in range(cs):
            if not mask[ly, lx]:
                continue
            for dx, dy in CORNERS:
                key = (lx + dx, ly + dy)
                if key not in vertex_map:
                    vertex_map[key] = len(corners)
                    corners.append(key)
            i0, i1, i2, i3 = (vertex_map[(lx + dx, ly + dy)] for dx, dy in CORNERS)
            triangles.append((i0, i2, i1))
            triangles.append((i1, i2, i3))
    incident = [[] for _ in corners]
    for t, tri in enumerate(triangles):
        for v in tri:
            incident[v].append(t)
    return corners, triangles, incident


def closed_form(mask):
    """the same three lists without a dictionary: owner = the first present cell among (px-1, py-1), (px, py-1), (px-1, py), (px, py);
    vertex index = corners owned by earlier cells + rank among the owner's own; triangles 2 rank(cell), 2 rank(cell) + 1; a vertex's
    triangles: cell (px-1, py-1) triangle 1, (px, py-1) triangles 0 and 1, (px-1, py) triangles 0 and 1, (px, py) triangle 0"""
    cs = mask.shape[0]

    def present(x, y):
        return 0 <= x < cs and 0 <= y < cs and bool(mask[y, x])

    def owner(px, py):
        for k, (x, y) in zip((3, 2, 1, 0), ((px - 1, py - 1), (px, py - 1), (px - 1, py), (px, py))):
            if present(x, y):
                return (x, y), k
        return None, None

    base, rank, owned = {}, {}, {}
    nv = nc = 0
    for ly in range(cs):
        for lx in range(cs):
            if not mask[ly, lx]:
                continue
            mine = [k for k, (dx, dy) in enumerate(CORNERS) if owner(lx + dx, ly + dy)[0] == (lx, ly)]
            base[(lx, ly)], rank[(lx, ly)], owned[(lx, ly)] = nv, nc, mine
            nv += len(mine)
            nc += 1

    def vertex(px, py):
        cell, k = owner(px, py)
        return base[cell] + owned[cell].index(k)

    corners = [None] * nv
    for py in range(cs + 1):
        for px in range(cs + 1):
            if owner(px, py)[0] is not None:
                corners[vertex(px, py)] = (px, py)
    triangles = [None] * (2 * nc)
    for (lx, ly), r in rank.items():
        i0, i1, i2, i3 = (vertex(lx + dx, ly + dy) for dx, dy in CORNERS)
        triangles[2 * r], triangles[2 * r + 1] = (i0, i2, i1), (i1, i2, i3)
    incident = []
    for px, py in corners:
        inc = []
        for (x, y), which in (((px - 1, py - 1), (1,)), ((px, py - 1), (0, 1)), ((px - 1, py), (0, 1)), ((px, py), (0,))):
            if present(x, y):
                inc += [2 * rank[(x, y)] + w for w in which]
        incident.append(inc)
    return corners, triangles, incident


def build_mesh(spec, coord, oracle, cs=None):
    """TerrainChunk::build_mesh for chunk `coord` of a HeightSpec: a dict of vertices [nv][4] f32, indices [nt][3] uint32 (chunk-local),
    uvs [nv][2] (zeros) and normals [nv][3] (the oracle's compute_vertex_normals over exactly these arrays)"""
    cs = spec.chunk_size if cs is None else cs
    corners, triangles, _ = transcription(present_mask(spec, coord, cs))
    nv, nt = len(corners), len(triangles)
    ox, oy = coord[0] * cs, coord[1] * cs
    v = np.zeros((nv, 4), F)
    if nv:
        px = np.array([ox + c[0] for c in corners], np.int64)
        py = np.array([oy + c[1] for c in corners], np.int64)
        v[:, 0] = px.astype(F) * spec.scale[0]          # px as f32 * terrain.scale.x: one multiplication
        v[:, 1] = spec.get_height(px, py)               # terrain-wide: the rim reads the neighbouring chunks, or 0.0
        v[:, 2] = py.astype(F) * spec.scale[1]
        v[:, 3] = 1.0
    i = np.array(triangles, np.uint32).reshape(nt, 3)
    uv = np.zeros((nv, 2), F)
    n = np.zeros((nv, 3), F)
    if nv:
        n = oracle.Batch3D.new(v, i, uv).with_computed_normals().geometry()[3]
        assert n.shape == (nv, 3)
    return dict(vertices=v, indices=i, uvs=uv, normals=n)


KEYS = ("vertices", "indices", "normals")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def first_difference(got, want, nan_as_nan=False):
    """'' when the three arrays are equal bit for bit (nan_as_nan: a NaN of the reference needs a NaN, everything else its bits)"""
    for k in KEYS:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        if g.shape != w.shape:
            return f"{k}: shape {g.shape} != {w.shape}"
        bad = bits(g) != bits(w)
        if nan_as_nan and g.dtype == F:
            bad &= ~(np.isnan(g) & np.isnan(w))
        if bad.any():
            at = tuple(int(x) for x in np.argwhere(bad)[0])
            return f"{k}{list(at)}: got {g[at]!r} ({bits(g)[at]:#x}), want {w[at]!r} ({bits(w)[at]:#x})"
    return ""


# ---- terrains ---------------------------------------------------------------------------------------------------------------------------
def height_at(x, y, seed=0):
    """a rolling field with a seeded ripple: finite, no two neighbours alike"""
    r = np.random.default_rng((seed * 1000003 + (x & 0xFFFF) * 65537 + (y & 0xFFFF)) & 0x7FFFFFFF).uniform(-0.3, 0.3)
    return F(2.0 * np.sin(x / 3.0) * np.cos(y / 4.0) + r)


def masked_spec(mask, coord=(0, 0), scale=(1.0, 1.0), seed=0, neighbours=True):
    """a HeightSpec whose chunk `coord` (of size len(mask)) has exactly the cells of `mask`; neighbours: the chunks to the right, below
    and diagonally below are full, so that the rim reads their heights (else it reads 0.0)"""
    cs = mask.shape[0]
    spec = HeightSpec(scale, cs)
    ox, oy = coord[0] * cs, coord[1] * cs
    for ly in range(cs):
        for lx in range(cs):
            if mask[ly, lx]:
                spec.height(ox + lx, oy + ly, height_at(ox + lx, oy + ly, seed))
    if neighbours:
        for k in range(cs + 1):
            spec.height(ox + cs, oy + k, height_at(ox + cs, oy + k, seed))
            spec.height(ox + k, oy + cs, height_at(ox + k, oy + cs, seed))
    return spec


def masks(cs):
    """name -> [cs][cs] presence: the shapes at which owner, scan and gather can go wrong"""
    full = np.ones((cs, cs), bool)
    out = {"empty": ~full, "full": full}
    for name, (y, x) in {"corner00": (0, 0), "corner10": (0, cs - 1), "corner01": (cs - 1, 0), "corner11": (cs - 1, cs - 1)}.items():
        m = ~full
        m[y, x] = True
        out[name] = m
    ys, xs = np.mgrid[0:cs, 0:cs]
    out["checker"] = (xs + ys) % 2 == 0
    hole = full.copy()
    hole[cs // 2, cs // 3] = False
    out["hole"] = hole
    for d in (0.2, 0.5, 0.9):
        out[f"random{d}"] = np.random.default_rng(cs * 100 + int(d * 10)).random((cs, cs)) < d
    return out
