"""A numpy-float32 transcription of the generated terrain's excluded sectors (reference src/chunkbuilder/terrain_generator.rs:
collect_excluded_sectors' box test :438-457 over BBox::intersects, src/map/bbox.rs:43-48; point_in_sector :891-950;
apply_exclusions :747-825 over triangulate :829-879), every operation rounded to f32, with vek's dot and magnitude as
tests/terrain_gen_ref.py restates them.  Nothing is hoisted or reordered.

`point_in_sector` is the text of the reference for one point, line by line.  `classify` is the same arithmetic over an array of
points at once (numpy rounds every elementwise f32 operation to f32, so the words are the same; tests/test_terrain_exclusion_cpu.py
holds the two against each other) and keeps what each pass said: `boundary` (the first pass returned true) and `ray` (what the ray
cast says, evaluated for every point, also where the reference never gets there)."""
import numpy as np

from tests.terrain_gen_ref import F, Generator, dot2, magnitude2, rclamp01, triangulate  # noqa: F401  (Generator: re-exported for the tests)

EPSILON = F(0.01)


class Exclusions:
    """the map's sectors of terrain_mode == 1, flattened as rxr_set_terrain_exclusions takes them.  `polygons`: per sector its
    linedefs' start vertices in order; `boxes`: per sector (min.x, min.y, max.x, max.y), by default the polygon's own bounds"""

    def __init__(self, polygons=(), boxes=None):
        self.polygons = [np.ascontiguousarray(p, F).reshape(-1, 2) for p in polygons]
        if boxes is None:
            boxes = [(p[:, 0].min(), p[:, 1].min(), p[:, 0].max(), p[:, 1].max()) for p in self.polygons]
        self.sector_boxes = np.ascontiguousarray(boxes, F).reshape(-1, 4)
        assert len(self.sector_boxes) == len(self.polygons)
        self.vertex_offsets = np.concatenate([[0], np.cumsum([len(p) for p in self.polygons])]).astype(np.uint32)
        self.vertices = np.concatenate(self.polygons + [np.zeros((0, 2), F)]).astype(F)

    def args(self):
        """keyword arguments of the product's TerrainGenerator.set_exclusions"""
        return dict(sector_boxes=self.sector_boxes, vertex_offsets=self.vertex_offsets, vertices=self.vertices)

    def active(self, box):
        """collect_excluded_sectors (:438-457): the sectors whose box intersects `box` as given, in list order"""
        b = np.asarray(box, F)
        return [s for s, sb in enumerate(self.sector_boxes) if sb[0] <= b[2] and sb[2] >= b[0] and sb[1] <= b[3] and sb[3] >= b[1]]


def point_in_sector(px, py, verts):
    """:891-950 for one point: (inside, decided by the boundary pass)"""
    px, py = F(px), F(py)
    n = len(verts)
    if n < 3:
        return False, False
    with np.errstate(all="ignore"):
        j = n - 1
        for i in range(n):
            vix, viy, vjx, vjy = verts[i][0], verts[i][1], verts[j][0], verts[j][1]
            ex, ey = F(vjx - vix), F(vjy - viy)
            edge_length_sq = dot2(ex, ey, ex, ey)
            if edge_length_sq > F(0.0):
                t = rclamp01(F(dot2(F(px - vix), F(py - viy), ex, ey) / edge_length_sq))
                qx, qy = F(vix + F(ex * t)), F(viy + F(ey * t))
                if magnitude2(F(px - qx), F(py - qy)) < EPSILON:
                    return True, True
            j = i
        inside = False
        j = n - 1
        for i in range(n):
            vix, viy, vjx, vjy = verts[i][0], verts[i][1], verts[j][0], verts[j][1]
            if (viy > py) != (vjy > py) and px < F(F(F(F(vjx - vix) * F(py - viy)) / F(vjy - viy)) + vix):
                inside = not inside
            j = i
    return inside, False


def classify(points, verts):
    """the same for points [P][2] at once: (boundary [P] bool, ray [P] bool); inside = boundary | ray"""
    pts = np.asarray(points, F).reshape(-1, 2)
    px, py = pts[:, 0], pts[:, 1]
    boundary, ray = np.zeros(len(pts), bool), np.zeros(len(pts), bool)
    n = len(verts)
    if n < 3:
        return boundary, ray
    with np.errstate(all="ignore"):
        j = n - 1
        for i in range(n):
            vix, viy, vjx, vjy = verts[i][0], verts[i][1], verts[j][0], verts[j][1]
            ex, ey = F(vjx - vix), F(vjy - viy)
            edge_length_sq = dot2(ex, ey, ex, ey)
            if edge_length_sq > F(0.0):
                t = (dot2(px - vix, py - viy, ex, ey) / edge_length_sq).astype(F)
                t = np.where(t < F(0.0), F(0.0), np.where(t > F(1.0), F(1.0), t)).astype(F)   # rclamp01: a NaN stays, -0.0 stays
                qx, qy = (vix + ex * t).astype(F), (viy + ey * t).astype(F)
                boundary |= magnitude2(px - qx, py - qy) < EPSILON
            cross_x = (F(vjx - vix) * (py - viy) / F(vjy - viy) + vix).astype(F)
            ray ^= ((viy > py) != (vjy > py)) & (px < cross_x)
            j = i
    return boundary, ray


def apply_exclusions(gen, excl, box):
    """:747-825 for one chunk box.  Returns a dict: counts = (steps_x, steps_y, active_sectors, n_vertices) with negative steps as 0;
    active (sector ids); points [P][2]; boundary / ray [P][A] per point and active sector; keep [T] per triangle of triangulate
    (None in the shared layout); vertex_points [n_vertices]: the grid point each vertex is"""
    (sx, sy), pts = gen.generate_grid(box)
    sx, sy = max(sx, 0), max(sy, 0)
    active = excl.active(box)
    out = dict(active=active, points=pts, keep=None)
    if not active:
        out.update(counts=(sx, sy, 0, sx * sy), vertex_points=np.arange(sx * sy, dtype=np.int64), boundary=np.zeros((len(pts), 0), bool), ray=np.zeros((len(pts), 0), bool))
        return out
    passes = [classify(pts, excl.polygons[s]) for s in active]
    boundary = np.stack([p[0] for p in passes], axis=1) if len(pts) else np.zeros((0, len(active)), bool)
    ray = np.stack([p[1] for p in passes], axis=1) if len(pts) else np.zeros((0, len(active)), bool)
    inside = boundary | ray
    tris = triangulate(sx, sy) if sx > 0 and sy > 0 else np.zeros((0, 3), np.uint32)
    # dropped iff ONE sector holds all three corners (the reference's `&&` and `break` change work, not results)
    keep = ~(inside[tris[:, 0]] & inside[tris[:, 1]] & inside[tris[:, 2]]).any(axis=1) if len(tris) else np.zeros(0, bool)
    vertex_points = tris[keep].reshape(-1).astype(np.int64)
    out.update(counts=(sx, sy, len(active), len(vertex_points)), keep=keep, vertex_points=vertex_points, boundary=boundary, ray=ray, triangles=tris)
    return out


def expected_vertices(res):
    """x and z of the vertices, [n_vertices][2] f32 (y is the height of grid point vertex_points[i]; w is 1.0)"""
    return res["points"][res["vertex_points"]] if len(res["vertex_points"]) else np.zeros((0, 2), F)


# ---- the scenes the CPU and the GPU tests share ----
def square(x0, y0, x1, y1, clockwise=False):
    p = [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]
    return p[::-1] if clockwise else p


def fuzz_scene(seed):
    """a 64 x 64 map (its generator is tests/terrain_gen_ref.scene(seed)) with excluded sectors of every kind: squares on grid lines
    (their right and top edges hold grid points the ray cast calls outside), two neighbours sharing the grid line x = 30 and a third
    one a cell away (triangles whose corners lie in different sectors), an L and a U (concave) with integer and fractional corners,
    random convex polygons in both windings.  Returns (Exclusions, boxes): the whole map and four chunk boxes"""
    rng = np.random.default_rng([0x7E44E7, seed])
    polys = [square(20, 8, 30, 18), square(30, 8, 38, 18, clockwise=True), square(39, 8, 44, 18)]
    ox, oy = int(rng.integers(4, 10)), int(rng.integers(24, 30))
    polys.append([(ox, oy), (ox + 12, oy), (ox + 12, oy + 5), (ox + 5, oy + 5), (ox + 5, oy + 14), (ox, oy + 14)])                       # an L
    ux, uy = float(rng.integers(28, 34)) + 0.5, float(rng.integers(26, 32)) + 0.25
    polys.append([(ux, uy), (ux, uy + 12), (ux + 4, uy + 12), (ux + 4, uy + 4), (ux + 9, uy + 4), (ux + 9, uy + 12), (ux + 13, uy + 12), (ux + 13, uy)])   # a U, clockwise
    for k in range(4):
        cx, cy, r, m = rng.uniform(10, 54), rng.uniform(44, 58), rng.uniform(3, 7), int(rng.integers(3, 9))
        ang = np.sort(rng.uniform(0, 2 * np.pi, m))
        p = [(cx + r * np.cos(a), cy + r * np.sin(a)) for a in ang]
        polys.append(p[::-1] if k % 2 else p)
    hx, hy = int(rng.integers(46, 52)), int(rng.integers(22, 30))
    polys.append(square(hx + 0.005, hy + 0.005, hx + 8 - 0.005, hy + 9 - 0.005))   # corners 0.005 inside the grid lines: the epsilon band
    boxes = [(0.0, 0.0, 64.0, 64.0), (16.0, 0.0, 32.0, 16.0), (32.0, 16.0, 48.0, 32.0), (0.0, 48.0, 16.0, 64.0), (48.0, 0.0, 64.0, 16.0)]
    return Exclusions(polys), boxes
