"""Ground truth of the flattened terrain heights: the Height pass of TerrainChunk::process_batch_modifiers (reference
src/terrain/chunk.rs:144-208) with ShapeFX::sector_modify_heightmap (src/shapestack/shapefx.rs:414-478), linedef_modify_heightmap
(:682-820), Sector::signed_distance / is_inside (src/map/sector.rs:272-333), BBox (src/map/bbox.rs) and smoothstep (:2258-2261),
restated in numpy float32 scalars AS THE REFERENCE'S LOOPS OVER A DICTIONARY: `for y in min_y..=max_y`, `for ty in
tile_min.y..tile_max.y`, inserts into a dict -- not as per-cell predicates, so that the device's per-cell form is held to the loop
form.  Every operation once and in the reference's order; numpy casts do not saturate, `as_i32` of tests/terrain_ref.py does.

One liberty, which changes no inserted key: the sector loop's integer range is clipped to the chunk's cells +- CLIP before it is
walked (the reference walks the whole sector; a huge sector would take this file forever).  Every insert sits behind
chunk_bbox.contains((x as f32, y as f32)); `x as f32` differs from x by at most 64 for |x| <= 2^30 + 2^12 (the spacing of f32 there
is 128) and the bounds are origin as f32 .. + size - 1, so a cell more than 2 * 64 + 1 away from the chunk cannot pass.

The op list's order is the caller's (include/rxr.h); for the reference it is the sectors in sorted_sectors_by_area() order, then the
linedef groups.  FlattenScene is the neutral description the tests build with: it answers the reference (`process_chunk`), makes
the arrays of rxr_set_terrain_flatten (`arrays`) and feeds the mirror (`product`)."""
import numpy as np

from tests.terrain_hit_ref import HeightSpec
from tests.terrain_ref import as_i32

F = np.float32
F32_MAX = np.finfo(np.float32).max
SECTOR, LINEDEFS = 0, 1              # RXR_TERRAIN_FLATTEN_SECTOR / _LINEDEFS
OP_FLOATS, RECORD_FLOATS = 6, 10     # RXR_TERRAIN_FLATTEN_OP_FLOATS / _RECORD_FLOATS
CLIP = 130


# ---- src/map/bbox.rs ---------------------------------------------------------------------------------------------------------------
class BBox:
    def __init__(self, min_x, min_y, max_x, max_y):
        self.min = (F(min_x), F(min_y))
        self.max = (F(max_x), F(max_y))

    def contains(self, p):
        return bool(p[0] >= self.min[0] and p[0] <= self.max[0] and p[1] >= self.min[1] and p[1] <= self.max[1])

    def intersects(self, o):
        return bool(self.min[0] <= o.max[0] and self.max[0] >= o.min[0] and self.min[1] <= o.max[1] and self.max[1] >= o.min[1])

    def expanded(self, amount):
        half = F(F(amount) * F(0.5))
        return BBox(F(self.min[0] - half), F(self.min[1] - half), F(self.max[0] + half), F(self.max[1] + half))

    def floats(self):
        return [self.min[0], self.min[1], self.max[0], self.max[1]]


def sector_box(edges):
    """Sector::bounding_box (src/map/sector.rs:90-117): folds of f32::min / f32::max (which drop a NaN) over the start and end points"""
    lo, hi = [F(np.inf), F(np.inf)], [F(-np.inf), F(-np.inf)]
    for e in edges:
        for vx, vy in ((e[0], e[1]), (e[2], e[3])):
            lo = [np.fmin(lo[0], F(vx)), np.fmin(lo[1], F(vy))]
            hi = [np.fmax(hi[0], F(vx)), np.fmax(hi[1], F(vy))]
    return BBox(lo[0], lo[1], hi[0], hi[1])


def linedef_box(s):
    """Linedef::bounding_box (src/map/linedef.rs:68-80)"""
    return BBox(np.fmin(F(s[0]), F(s[2])), np.fmin(F(s[1]), F(s[3])), np.fmax(F(s[0]), F(s[2])), np.fmax(F(s[1]), F(s[3])))


def clamp01(t):
    """f32::clamp(0.0, 1.0): a NaN stays"""
    if t < F(0.0):
        return F(0.0)
    if t > F(1.0):
        return F(1.0)
    return t


def smoothstep(edge0, edge1, x):
    t = clamp01(F(F(x - edge0) / F(edge1 - edge0)))
    return F(F(t * t) * F(F(3.0) - F(F(2.0) * t)))


def magnitude(x, y):
    return F(np.sqrt(F(F(x * x) + F(y * y))))


# ---- the scene ---------------------------------------------------------------------------------------------------------------------
class Op:
    def __init__(self, kind, bevel, floor_height, records, box):
        self.kind, self.bevel, self.floor_height, self.records, self.box = kind, F(bevel), F(floor_height), records, box


class FlattenScene:
    def __init__(self, scale=(1.0, 1.0), chunk_size=16):
        self.spec = HeightSpec(scale, chunk_size)
        self.ops = []

    def height(self, x, y, h):
        self.spec.height(x, y, h)
        return self

    def sector(self, edges, bevel=0.5, floor_height=0.0, box=None):
        """one Flatten node on one sector: edges [(x0, y0, x1, y1)] in linedef order.  Passing another op's `records` list shares
        its range of the pool (two Flatten nodes on one sector)."""
        records = edges if edges and isinstance(edges[0], list) else [[F(v) for v in e] + [F(0.0)] * 6 for e in edges]
        self.ops.append(Op(SECTOR, bevel, floor_height, records, box or sector_box([r[:4] for r in records])))
        return self.ops[-1]

    def linedefs(self, segments, bevel=0.5):
        """one Flatten node on one group of linedefs: segments [(x0, y0, x1, y1, height_start, height_end)]"""
        records = [[F(v) for v in s] + linedef_box(s).floats() for s in segments]
        self.ops.append(Op(LINEDEFS, bevel, 0.0, records, BBox(0, 0, 0, 0)))
        return self.ops[-1]

    def arrays(self):
        """the arguments of rxr_check_terrain_flatten / rxr_set_terrain_flatten behind ctx, as a dict (which keeps the arrays alive)
        and a tuple.  Ops that share one records list share one range."""
        pool, where = [], {}
        kinds, params, ranges = [], [], []
        for op in self.ops:
            if id(op.records) not in where:
                where[id(op.records)] = len(pool)
                pool.extend(op.records)
            kinds.append(op.kind)
            params.append([op.bevel, op.floor_height] + op.box.floats())
            ranges.append([where[id(op.records)], len(op.records)])
        n = len(self.ops)
        keep = dict(kinds=np.array(kinds, np.uint32), params=np.array(params, np.float32).reshape(n, OP_FLOATS), ranges=np.array(ranges, np.uint32).reshape(n, 2),
                    records=np.array(pool, np.float32).reshape(len(pool), RECORD_FLOATS))
        ptr = lambda a: a.ctypes.data if a.size else None
        return keep, (ptr(keep["kinds"]), ptr(keep["params"]), ptr(keep["ranges"]), n, ptr(keep["records"]), len(pool))

    def product(self, api):
        t = self.spec.product(api)
        keep, _ = self.arrays()
        t.set_flatten_ops(keep["kinds"], keep["params"], keep["ranges"], keep["records"])
        return t

    # ---- the reference -------------------------------------------------------------------------------------------------------------
    def bounds(self, coord):
        """TerrainChunk::bounds (:130-134)"""
        cs = self.spec.chunk_size
        ox, oy = F(coord[0] * cs), F(coord[1] * cs)
        size = F(F(cs) - F(1.0))
        return BBox(ox, oy, F(ox + size), F(oy + size))

    def unprocessed(self, x, y):
        return self.spec.heights.get((x, y))

    def process_chunk(self, coord):
        """process_batch_modifiers' Height pass for one chunk: {(local x, local y): f32}, every key the reference inserts"""
        cs = self.spec.chunk_size
        origin = (coord[0] * cs, coord[1] * cs)
        with np.errstate(all="ignore"):
            processed = {(x - origin[0], y - origin[1]): h for (x, y), h in self.spec.heights.items()
                         if origin[0] <= x < origin[0] + cs and origin[1] <= y < origin[1] + cs}       # self.heights.clone()
            bbox = self.bounds(coord)
            for op in self.ops:
                if op.kind == SECTOR:
                    if bbox.intersects(op.box.expanded(2.0)):
                        self._sector(op, bbox, origin, processed)
                else:
                    group = [r for r in op.records if bbox.intersects(BBox(*r[6:10]).expanded(2.0))]
                    if group:
                        self._linedefs(op, group, bbox, origin, processed)
        return processed

    def dense(self, coord):
        """the chunk's own cells of process_chunk as rxr_flatten_terrain returns them: heights [cs * cs] (0.0 where absent) and present"""
        cs = self.spec.chunk_size
        d = self.process_chunk(coord)
        h, p = np.zeros(cs * cs, F), np.zeros(cs * cs, np.uint8)
        for (lx, ly), v in d.items():
            if 0 <= lx < cs and 0 <= ly < cs:
                h[ly * cs + lx] = v
                p[ly * cs + lx] = 1
        return h, p

    def processed_spec(self, coords):
        """a HeightSpec of processed_heights: the named chunks' processed cells, every other cell as registered"""
        cs = self.spec.chunk_size
        out = HeightSpec(self.spec.scale, cs)
        named = set(map(tuple, coords))
        for (x, y), h in self.spec.heights.items():
            if (x // cs, y // cs) not in named:
                out.height(x, y, h)
        for c in named:
            for (lx, ly), v in self.process_chunk(c).items():
                if 0 <= lx < cs and 0 <= ly < cs:
                    out.height(c[0] * cs + lx, c[1] * cs + ly, v)
        return out

    def _signed_distance(self, op, p):
        """Sector::signed_distance (:308-333) with is_inside (:272-305)"""
        min_dist = F(F32_MAX)
        for r in op.records:
            v0, v1 = (r[0], r[1]), (r[2], r[3])
            edge = (F(v1[0] - v0[0]), F(v1[1] - v0[1]))
            to_point = (F(p[0] - v0[0]), F(p[1] - v0[1]))
            t = F(F(F(to_point[0] * edge[0]) + F(to_point[1] * edge[1])) / F(F(edge[0] * edge[0]) + F(edge[1] * edge[1])))
            t_clamped = clamp01(t)
            closest = (F(v0[0] + F(edge[0] * t_clamped)), F(v0[1] + F(edge[1] * t_clamped)))
            dist = magnitude(F(p[0] - closest[0]), F(p[1] - closest[1]))
            min_dist = np.fmin(min_dist, dist)          # f32::min drops a NaN operand
        polygon = [(r[0], r[1]) for r in op.records]
        inside = False
        if len(polygon) >= 3:
            j = len(polygon) - 1
            for i in range(len(polygon)):
                if (polygon[i][1] > p[1]) != (polygon[j][1] > p[1]) and \
                        p[0] < F(F(F(F(polygon[j][0] - polygon[i][0]) * F(p[1] - polygon[i][1])) / F(polygon[j][1] - polygon[i][1])) + polygon[i][0]):
                    inside = not inside
                j = i
        return F(-min_dist) if inside else min_dist

    def _sector(self, op, bbox, origin, heights):
        cs = self.spec.chunk_size
        bevel, floor_height = op.bevel, op.floor_height
        expanded_bbox = bbox.expanded(bevel)            # `*bbox` after expand(bevel)
        chunk_bbox = bbox
        bounds = op.box.expanded(bevel)
        min_x, max_x = int(as_i32(np.floor(bounds.min[0]))), int(as_i32(np.ceil(bounds.max[0])))
        min_y, max_y = int(as_i32(np.floor(bounds.min[1]))), int(as_i32(np.ceil(bounds.max[1])))
        # (the liberty of the head comment)
        min_x, max_x = max(min_x, origin[0] - CLIP), min(max_x, origin[0] + cs + CLIP)
        min_y, max_y = max(min_y, origin[1] - CLIP), min(max_y, origin[1] + cs + CLIP)
        for y in range(min_y, max_y + 1):
            for x in range(min_x, max_x + 1):
                p = (F(x), F(y))
                if not expanded_bbox.contains(p):
                    continue
                sd = self._signed_distance(op, p)
                if sd < F(bevel * F(4.0)):
                    s = smoothstep(F(0.0), bevel, F(bevel - sd))
                    original = self.unprocessed(x, y)
                    if original is None:
                        original = floor_height
                    new_height = F(F(original * F(F(1.0) - s)) + F(floor_height * s))
                    if chunk_bbox.contains((F(x), F(y))):
                        heights[(x - origin[0], y - origin[1])] = new_height

    def _linedefs(self, op, segments, bbox, origin, heights):
        bevel = op.bevel
        scale = self.spec.scale
        chunk_bbox = bbox

        def point_to_line_segment(p, a, b):
            ab = (F(b[0] - a[0]), F(b[1] - a[1]))
            ap = (F(p[0] - a[0]), F(p[1] - a[1]))
            t = F(F(F(ap[0] * ab[0]) + F(ap[1] * ab[1])) / F(F(ab[0] * ab[0]) + F(ab[1] * ab[1])))
            t_clamped = clamp01(t)
            closest = (F(a[0] + F(ab[0] * t_clamped)), F(a[1] + F(ab[1] * t_clamped)))
            return magnitude(F(p[0] - closest[0]), F(p[1] - closest[1])), t_clamped

        def closest_segment(p):
            best = None
            for seg in segments:
                dist, t = point_to_line_segment(p, (seg[0], seg[1]), (seg[2], seg[3]))
                if best is None or dist < best[0]:
                    best = (dist, t, seg)
            return best

        mn = (F(bbox.min[0] - F(bevel * scale[0])), F(bbox.min[1] - F(bevel * scale[1])))
        mx = (F(bbox.max[0] + F(bevel * scale[0])), F(bbox.max[1] + F(bevel * scale[1])))
        tile_min = (int(as_i32(np.floor(F(mn[0] / scale[0])))), int(as_i32(np.floor(F(mn[1] / scale[1])))))
        tile_max = (int(as_i32(np.ceil(F(mx[0] / scale[0])))), int(as_i32(np.ceil(F(mx[1] / scale[1])))))
        for ty in range(tile_min[1], tile_max[1]):
            for tx in range(tile_min[0], tile_max[0]):
                tile_center = (F(F(F(tx) + F(0.5)) * scale[0]), F(F(F(ty) + F(0.5)) * scale[1]))
                found = closest_segment(tile_center)
                if found is None:
                    continue
                dist, t, seg = found
                if dist > bevel:
                    continue
                height = F(F(seg[4] * F(F(1.0) - t)) + F(seg[5] * t))
                blend = smoothstep(F(0.0), bevel, F(bevel - dist))
                if chunk_bbox.contains((F(tx), F(ty))):
                    original = self.unprocessed(tx, ty)
                    if original is None:
                        original = height
                    heights[(tx - origin[0], ty - origin[1])] = F(F(original * F(F(1.0) - blend)) + F(height * blend))


# ---- comparison --------------------------------------------------------------------------------------------------------------------
def first_difference(got_h, got_p, want_h, want_p):
    """'' when every presence byte and every height word are equal (a NaN needs a NaN), else where they first differ"""
    got_h, want_h = np.asarray(got_h, F).ravel(), np.asarray(want_h, F).ravel()
    got_p, want_p = np.asarray(got_p, np.uint8).ravel(), np.asarray(want_p, np.uint8).ravel()
    if got_h.shape != want_h.shape or got_p.shape != want_p.shape:
        return f"shapes {got_h.shape} {got_p.shape} against {want_h.shape} {want_p.shape}"
    bad = got_p != want_p
    if bad.any():
        i = int(np.nonzero(bad)[0][0])
        return f"presence of cell {i}: {got_p[i]} against {want_p[i]}"
    nan = np.isnan(want_h)
    bad = np.where(nan, ~np.isnan(got_h), got_h.view(np.uint32) != want_h.view(np.uint32))
    if bad.any():
        i = int(np.nonzero(bad)[0][0])
        return f"height of cell {i}: {got_h[i]!r} ({got_h.view(np.uint32)[i]:#x}) against {want_h[i]!r} ({want_h.view(np.uint32)[i]:#x})"
    return ""


# ---- scenes ------------------------------------------------------------------------------------------------------------------------
def polygon(cx, cy, radius, n, phase=0.0):
    """the n edges of a regular polygon, counter-clockwise"""
    pts = [(F(cx + radius * np.cos(phase + 2 * np.pi * k / n)), F(cy + radius * np.sin(phase + 2 * np.pi * k / n))) for k in range(n)]
    return [(pts[k][0], pts[k][1], pts[(k + 1) % n][0], pts[(k + 1) % n][1]) for k in range(n)]


def square(x0, y0, x1, y1):
    return [(x0, y0, x1, y0), (x1, y0, x1, y1), (x1, y1, x0, y1), (x0, y1, x0, y0)]


def fill(scene, coords, density=1.0, seed=0):
    """heights over the cells of `coords` (a share `density` of them), a smooth field plus noise"""
    rng = np.random.default_rng(seed)
    cs = scene.spec.chunk_size
    for cx, cy in coords:
        for ly in range(cs):
            for lx in range(cs):
                if density >= 1.0 or rng.random() < density:
                    x, y = cx * cs + lx, cy * cs + ly
                    scene.height(x, y, F(2.0 * np.sin(0.37 * x) + 1.5 * np.cos(0.23 * y) + rng.uniform(-0.25, 0.25)))
    return scene


def fuzz_scene(seed):
    """a seeded scene over 3 x 3 chunks of 8: some cells absent, sectors of 3..9 edges (some degenerate, some far away), roads, bevels
    of every sign, special values now and then; returns (scene, coords)"""
    rng = np.random.default_rng(seed)
    scale = [(1.0, 1.0), (2.0, 0.5), (0.5, 2.0), (1.0, 1.5)][int(rng.integers(4))]
    cs = 8
    base = (int(rng.integers(-3, 3)), int(rng.integers(-3, 3)))
    coords = [(base[0] + i, base[1] + j) for j in range(3) for i in range(3)]
    sc = fill(FlattenScene(scale, cs), coords, density=0.8, seed=seed)
    lo = (base[0] * cs, base[1] * cs)
    special = [np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-40, 3e38]

    def coordinate(axis):
        v = F(lo[axis] + rng.uniform(-4, 3 * cs + 4))
        return F(np.round(v)) if rng.random() < 0.3 else v

    if rng.random() < 0.5:
        k = list(sc.spec.heights)[int(rng.integers(len(sc.spec.heights)))]
        sc.height(k[0], k[1], special[int(rng.integers(len(special)))])
    for _ in range(int(rng.integers(3, 9))):
        bevel = F([0.5, 1.0, 2.5, 0.0, -1.0, 0.25][int(rng.integers(6))])
        if rng.random() < 0.6:
            n = int(rng.integers(3, 10))
            edges = polygon(coordinate(0), coordinate(1), rng.uniform(0.5, 6.0), n, rng.uniform(0, 6.28))
            if rng.random() < 0.2:                      # a zero-length edge
                e = edges[int(rng.integers(n))]
                edges.insert(0, (e[0], e[1], e[0], e[1]))
            if rng.random() < 0.1:
                edges = edges[:2]
            if rng.random() < 0.1:
                e = list(edges[0])
                e[int(rng.integers(4))] = F(special[int(rng.integers(3))])
                edges[0] = tuple(e)
            op = sc.sector(edges, bevel, F(rng.uniform(-3, 3)))
            if rng.random() < 0.25:                     # a second Flatten node on the same sector
                sc.sector(op.records, F(bevel * F(0.5)), F(rng.uniform(-3, 3)))
        else:
            segs = []
            x, y = coordinate(0), coordinate(1)
            for _ in range(int(rng.integers(1, 6))):
                nx, ny = (x, y) if rng.random() < 0.15 else (coordinate(0), coordinate(1))
                segs.append((x, y, nx, ny, F(rng.uniform(-2, 2)), F(rng.uniform(-2, 2))))
                x, y = nx, ny
            sc.linedefs(segs, bevel)
    return sc, coords


# ---- the cases of tests/test_terrain_flatten_cpu.py and tests/test_gpu_terrain_flatten.py ---------------------------------------------
FAR = 1000.0                         # a sector out there is listed but active for none of the cases' chunks


def _sizes_case(cs):
    """a pentagon over the corner of four chunks, a road across them and a second, shorter road; a hole of absent cells under both"""
    coords = [(0, 0)] if cs == 64 else [(-1, -1), (0, -1), (-1, 0), (0, 0)]
    sc = fill(FlattenScene((1.0, 1.0), cs), coords, seed=cs)
    r = max(1.0, cs * 0.45)
    for x in range(-1, 2):
        sc.spec.heights.pop((x, 0), None)
    sc.sector(polygon(0.3, 0.2, r, 5, 0.4), bevel=1.0, floor_height=-1.5)
    sc.linedefs([(-cs + 0.5, -0.7 * r, cs - 0.5, 0.6 * r, 1.0, 2.0), (0.0, 0.0, 0.4 * r, r, 2.0, 0.5)], bevel=1.25)
    return sc, coords


def _ops_case(n_active):
    """n_active small squares inside chunk (0, 0) of size 8, a far sector listed after each: order must survive the compaction"""
    sc = fill(FlattenScene((1.0, 1.0), 8), [(0, 0)], seed=n_active)
    for k in range(n_active):
        x0, y0 = 0.5 + (k * 3) % 5, 0.25 + (k * 5) % 6
        sc.sector(square(x0, y0, x0 + 1.5, y0 + 1.25), bevel=0.5, floor_height=F(0.125 * (k % 17) - 1.0))
        sc.sector(square(FAR + k, FAR, FAR + k + 1.0, FAR + 1.0), bevel=0.5, floor_height=9.0)
    return sc, [(0, 0)]


def _edges_case(n_edges):
    sc = fill(FlattenScene((1.0, 1.0), 16), [(0, 0)], seed=n_edges)
    sc.sector(polygon(7.3, 8.1, 5.0, n_edges, 0.1), bevel=1.0, floor_height=0.75)
    return sc, [(0, 0)]


def _segments_case(n_segments):
    """a zig-zag of n_segments over three chunks of 8 in a row: every chunk's filter drops the segments of the far end"""
    coords = [(0, 0), (1, 0), (2, 0)]
    sc = fill(FlattenScene((1.0, 1.0), 8), coords, density=0.9, seed=n_segments)
    xs = np.linspace(-3.0, 27.0, n_segments + 1).astype(F)
    segs = [(xs[k], F(2.0 + 3.0 * (k % 2)), xs[k + 1], F(2.0 + 3.0 * ((k + 1) % 2)), F(0.5 + 0.01 * k), F(1.0 - 0.02 * k)) for k in range(n_segments)]
    sc.linedefs(segs, bevel=1.5)
    return sc, coords


def _overlap_case(order):
    sc = fill(FlattenScene((1.0, 1.0), 8), [(0, 0)], seed=3)
    a = dict(edges=square(1.0, 1.0, 5.0, 5.0), bevel=1.0, floor_height=2.0)
    b = dict(edges=square(3.0, 2.0, 7.0, 6.0), bevel=0.5, floor_height=-2.0)
    for op in ((a, b) if order == 0 else (b, a)):
        sc.sector(**op)
    return sc, [(0, 0)]


def _road_over_sector_case():
    coords = [(0, 0), (1, 0)]
    sc = fill(FlattenScene((1.0, 1.0), 8), coords, seed=4)
    for x in range(2, 5):                       # absent cells inside the sector, and under the road at its far end
        sc.spec.heights.pop((x, 2), None)
    sc.spec.heights.pop((13, 4), None)
    sc.sector(square(0.5, 0.5, 9.5, 6.5), bevel=1.0, floor_height=1.0)
    sc.linedefs([(1.0, 4.4, 14.6, 4.6, 3.0, 4.0)], bevel=1.0)
    return sc, coords


def _two_nodes_case():
    sc = fill(FlattenScene((1.0, 1.0), 8), [(0, 0)], seed=5)
    first = sc.sector(polygon(3.5, 3.5, 3.0, 6), bevel=2.0, floor_height=1.0)
    sc.sector(first.records, bevel=0.5, floor_height=1.0)
    return sc, [(0, 0)]


def _untouched_chunk_case():
    coords = [(0, 0), (4, 4)]
    sc = fill(FlattenScene((1.0, 1.0), 8), coords, density=0.7, seed=6)
    sc.sector(square(1.0, 1.0, 4.0, 4.0), bevel=1.0, floor_height=0.5)
    sc.linedefs([(0.0, 6.0, 7.0, 6.5, 1.0, 1.0)], bevel=1.0)
    return sc, coords


def _filter_margin_case():
    """the sector's box starts 1.5 cells beyond chunk (0, 0)'s bounds: expanded(2.0) moves it by 1, so the chunk never sees it, though
    bevel * 4 = 32 would reach every cell; chunk (1, 0) does"""
    coords = [(0, 0), (1, 0)]
    sc = fill(FlattenScene((1.0, 1.0), 8), coords, seed=7)
    sc.sector(square(8.5, 1.0, 12.0, 5.0), bevel=8.0, floor_height=3.0)
    return sc, coords


def _neighbour_segments_case():
    """the short segment lies in chunk (1, 0) alone: cell (7, 4) of chunk (0, 0) is nearer to it than to the long one, and still takes
    the long one's height"""
    coords = [(0, 0), (1, 0)]
    sc = fill(FlattenScene((1.0, 1.0), 8), coords, seed=8)
    sc.linedefs([(0.0, 0.0, 16.0, 0.0, 1.0, 1.0), (10.0, 4.0, 12.0, 4.0, 5.0, 5.0)], bevel=6.0)
    return sc, coords


def _zero_bevel_case():
    """bevel == 0: inside the sector (x - 0) / (0 - 0) is +inf and clamps to 1; on the road, whose segment runs through tile centres,
    0 / 0 is a NaN; the road's loop leaves the chunk's last row and column out"""
    sc = fill(FlattenScene((1.0, 1.0), 8), [(0, 0)], seed=9)
    sc.sector(square(0.5, 0.5, 3.5, 3.5), bevel=0.0, floor_height=2.0)
    sc.linedefs([(0.5, 5.5, 7.5, 5.5, 1.0, 1.0), (7.5, 0.5, 7.5, 7.5, 1.0, 1.0)], bevel=0.0)
    return sc, [(0, 0)]


def _negative_bevel_case():
    sc = fill(FlattenScene((1.0, 1.0), 16), [(0, 0)], seed=10)
    sc.sector(square(1.0, 1.0, 14.0, 14.0), bevel=-1.0, floor_height=2.0)
    sc.linedefs([(0.5, 8.5, 15.5, 8.5, 1.0, 1.0)], bevel=-1.0)
    return sc, [(0, 0)]


def _two_vertices_case():
    sc = fill(FlattenScene((1.0, 1.0), 8), [(0, 0)], density=0.8, seed=11)
    sc.sector([(2.0, 2.0, 5.0, 4.0), (5.0, 4.0, 2.0, 2.0)], bevel=0.5, floor_height=1.0)
    return sc, [(0, 0)]


def _zero_length_edge_case():
    sc = fill(FlattenScene((1.0, 1.0), 8), [(0, 0)], seed=12)
    e = square(1.5, 1.5, 5.5, 5.5)
    sc.sector([e[0], (5.5, 1.5, 5.5, 1.5)] + e[1:], bevel=1.0, floor_height=-1.0)
    return sc, [(0, 0)]


def _degenerate_segment_case(place):
    sc = fill(FlattenScene((1.0, 1.0), 8), [(0, 0)], density=0.8, seed=13)
    good, point = (0.5, 3.5, 7.5, 3.5, 1.0, 2.0), (3.0, 3.0, 3.0, 3.0, 7.0, 7.0)
    sc.linedefs([point, good] if place == 0 else [good, point], bevel=1.5)
    return sc, [(0, 0)]


def _scale_case(scale):
    coords = [(0, 0), (1, 0), (0, 1)]
    sc = fill(FlattenScene(scale, 8), coords, density=0.85, seed=14)
    sc.sector(polygon(6.0, 5.0, 4.0, 7), bevel=1.0, floor_height=1.0)
    sc.linedefs([(1.0, 1.0, 9.0, 3.0, 0.0, 2.0), (9.0, 3.0, 4.0, 7.5, 2.0, 1.0)], bevel=1.5)
    return sc, coords


def _big_origin_case():
    """chunk origin x = 2^24 + 16: odd x round to their even neighbours as f32"""
    cs = 16
    coords = [(2 ** 20 + 1, 0)]
    sc = fill(FlattenScene((1.0, 1.0), cs), coords, density=0.9, seed=15)
    ox = 2 ** 24 + 16
    sc.sector(square(ox + 2.0, 2.0, ox + 10.0, 10.0), bevel=2.0, floor_height=1.0)
    sc.linedefs([(ox + 0.0, 12.0, ox + 15.0, 13.0, 1.0, 3.0)], bevel=2.0)
    return sc, coords


def _special_values_case():
    sc = fill(FlattenScene((1.0, 1.0), 8), [(0, 0)], density=0.9, seed=16)
    for k, v in enumerate([np.nan, np.inf, -np.inf, -0.0, 1e-40, 3e38]):
        sc.height(1 + k, 2, v)
        sc.height(1 + k, 5, v)
    sc.sector(square(0.5, 0.5, 7.0, 3.5), bevel=1.0, floor_height=1.0)
    e = square(1.0, 4.0, 6.0, 7.0)
    sc.sector([e[0], (6.0, 4.0, np.nan, 7.0)] + e[2:], bevel=1.0, floor_height=-1.0)
    sc.linedefs([(0.0, 5.5, np.nan, 5.5, 1.0, 1.0), (0.0, 6.5, 7.0, 6.5, np.inf, 1.0)], bevel=1.0)
    return sc, [(0, 0)]


CASES = {}
for _cs in (1, 8, 9, 16, 64):
    CASES[f"size_{_cs}"] = (lambda cs=_cs: _sizes_case(cs))
for _n in (1, 63, 64, 65, 129):
    CASES[f"active_ops_{_n}"] = (lambda n=_n: _ops_case(n))
for _n in (3, 64, 65):
    CASES[f"sector_edges_{_n}"] = (lambda n=_n: _edges_case(n))
for _n in (1, 64, 65):
    CASES[f"group_segments_{_n}"] = (lambda n=_n: _segments_case(n))
CASES.update({
    "overlap_first_order": lambda: _overlap_case(0), "overlap_other_order": lambda: _overlap_case(1),
    "road_over_sector": _road_over_sector_case, "two_nodes_on_one_sector": _two_nodes_case, "untouched_chunk": _untouched_chunk_case,
    "filter_margin": _filter_margin_case, "neighbour_segments": _neighbour_segments_case, "zero_bevel": _zero_bevel_case,
    "negative_bevel": _negative_bevel_case, "two_vertices": _two_vertices_case, "zero_length_edge": _zero_length_edge_case,
    "degenerate_first_segment": lambda: _degenerate_segment_case(0), "degenerate_second_segment": lambda: _degenerate_segment_case(1),
    "scale_2_half": lambda: _scale_case((2.0, 0.5)), "scale_half_2": lambda: _scale_case((0.5, 2.0)),
    "origin_2_24": _big_origin_case, "special_values": _special_values_case,
    "fuzz_1": lambda: fuzz_scene(1), "fuzz_2": lambda: fuzz_scene(2),
})
_BUILT = {}


def case(name):
    """(scene, coords, [(heights, present) per chunk]): built and answered by the transcription once, shared, never changed"""
    if name not in _BUILT:
        sc, coords = CASES[name]()
        _BUILT[name] = (sc, coords, [sc.dense(c) for c in coords])
    return _BUILT[name]
