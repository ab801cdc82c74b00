"""A numpy-float32 transcription of the generated terrain's height field (reference src/chunkbuilder/terrain_generator.rs:
sample_height_at :57-163 = interpolate_height_at :650-714 with calculate_map_edge_falloff :718-743, calculate_ridge_height_at :513-550
over distance_point_to_segment :1037-1055, apply_linedef_smoothing :555-623; sample_normal_at :166-181; generate_grid :460-485;
triangulate :829-879), every operation rounded to f32, with vek's magnitude, dot and normalized as include/rusterix_vek.hpp restates
them.  Nothing is hoisted or reordered here: this is the text of the reference, one line per line.

powf is the one operation of the field that is not bit-defined (a libm call on either side).  `sample` therefore returns per point

    height   the f32 result with numpy's powf
    sites    how many powf sites were evaluated
    lo, hi   float64 bounds of the results any powf within POW_ULPS ulp32 of the true power can give: with zero sites lo == hi ==
             height; otherwise the arithmetic behind each site is repeated in interval form -- each powf result widened by POW_ULPS
             ulp32 (the bound tests/test_gpu_libm_ulp.py holds the Pow opcode to), each later f32 rounding widened by one ulp32 of
             the endpoint of larger magnitude (a rounding moves a value by half an ulp at most), and where a comparison on a
             pow-dependent value (influence > 0.0, total_influence > 1.0) is undecided both branches are united (the function is
             continuous there)
    exempt   a powf result below 2^-126 (ulps mean nothing there, and `influence > 0.0` may flip): the point is not compared
"""
import math

import numpy as np

F = np.float32
POW_ULPS = 16
TINY = 2.0 ** -126


def ulp32(x):
    """the spacing of f32 at |x| (float64 in, float64 out)"""
    x = abs(float(x))
    if math.isnan(x) or math.isinf(x):
        return x
    if x < TINY:
        return 2.0 ** -149
    return 2.0 ** (math.frexp(x)[1] - 1 - 23)


class Iv:
    """a closed float64 interval; every operation models ONE f32 operation on any operands inside the operand intervals"""

    __slots__ = ("lo", "hi")

    def __init__(self, lo, hi=None):
        self.lo, self.hi = float(lo), float(lo if hi is None else hi)

    @staticmethod
    def of(x):
        return x if isinstance(x, Iv) else Iv(float(x))

    def _rounded(self):
        if math.isnan(self.lo) or math.isnan(self.hi):
            return Iv(math.nan)
        w = ulp32(max(abs(self.lo), abs(self.hi)))
        return Iv(self.lo - w, self.hi + w)

    def __add__(self, o):
        o = Iv.of(o)
        return Iv(self.lo + o.lo, self.hi + o.hi)._rounded()

    __radd__ = __add__

    def __sub__(self, o):
        o = Iv.of(o)
        return Iv(self.lo - o.hi, self.hi - o.lo)._rounded()

    def __rsub__(self, o):
        return Iv.of(o) - self

    def __mul__(self, o):
        o = Iv.of(o)
        p = [self.lo * o.lo, self.lo * o.hi, self.hi * o.lo, self.hi * o.hi]
        if any(math.isnan(v) for v in p):
            return Iv(math.nan)
        return Iv(min(p), max(p))._rounded()

    __rmul__ = __mul__

    def union(self, o):
        o = Iv.of(o)
        if math.isnan(self.lo) or math.isnan(o.lo):
            return Iv(math.nan)
        return Iv(min(self.lo, o.lo), max(self.hi, o.hi))


def _pow_iv(p):
    """the interval of a powf site whose numpy result is p"""
    w = POW_ULPS * ulp32(p)
    return Iv(float(p) - w, float(p) + w)


# ---- vek, as include/rusterix_vek.hpp restates it ----
def dot2(ax, ay, bx, by):
    return F(F(ax * bx) + F(ay * by))


def magnitude2(x, y):
    return F(np.sqrt(dot2(x, y, x, y)))


def rclamp01(t):
    """f32::clamp(0.0, 1.0): a NaN stays, -0.0 stays"""
    return F(0.0) if t < F(0.0) else (F(1.0) if t > F(1.0) else t)


def fmin(a, b):
    """f32::min: a NaN is skipped"""
    if a != a:
        return b
    if b != b:
        return a
    return a if a < b else b


def normal_from_heights(h_center, h_right, h_up):
    """the tail of sample_normal_at (:174-180): tangents, cross, normalized"""
    with np.errstate(all="ignore"):
        delta = F(0.1)
        ax, ay, az = delta, F(F(h_right) - F(h_center)), F(0.0)
        bx, by, bz = F(0.0), F(F(h_up) - F(h_center)), delta
        cx = F(F(ay * bz) - F(az * by))
        cy = F(F(az * bx) - F(ax * bz))
        cz = F(F(ax * by) - F(ay * bx))
        m = F(np.sqrt(F(F(F(cx * cx) + F(cy * cy)) + F(cz * cz))))
        return np.array([F(cx / m), F(cy / m), F(cz / m)], F)


class Generator:
    """the lists TerrainGenerator::generate collects (:255-294), flattened as rxr_set_terrain_generator takes them"""

    def __init__(self, control_points=(), ridges=(), ridge_edge_offsets=None, ridge_edges=(), linedefs=(), map_box=(-100.0, -100.0, 100.0, 100.0),
                 subdivisions=1):
        def rec(a, k):
            a = np.ascontiguousarray(a, F)
            return a.reshape(a.size // k, k)

        self.control_points, self.ridges, self.ridge_edges, self.linedefs = rec(control_points, 4), rec(ridges, 4), rec(ridge_edges, 4), rec(linedefs, 9)
        self.ridge_edge_offsets = np.zeros(1, np.uint32) if ridge_edge_offsets is None else np.asarray(ridge_edge_offsets, np.uint32).reshape(-1)
        assert len(self.ridge_edge_offsets) == len(self.ridges) + 1
        self.map_box = np.ascontiguousarray(map_box, F).reshape(4)
        self.subdivisions = int(subdivisions)

    def args(self):
        """keyword arguments of the product's TerrainGenerator"""
        return dict(control_points=self.control_points, ridges=self.ridges, ridge_edge_offsets=self.ridge_edge_offsets, ridge_edges=self.ridge_edges,
                    linedefs=self.linedefs, map_box=self.map_box, subdivisions=self.subdivisions)

    # calculate_map_edge_falloff (:718-743)
    def edge_falloff(self, px, py):
        b = self.map_box
        m = fmin(fmin(fmin(F(px - b[0]), F(b[2] - px)), F(py - b[1])), F(b[3] - py))
        if m <= F(0.0):
            return F(0.0)
        if m >= F(10.0):
            return F(1.0)
        t = F(m / F(10.0))
        return F(F(t * t) * F(F(3.0) - F(F(2.0) * t)))

    # interpolate_height_at (:650-714)
    def base_height(self, px, py):
        if len(self.control_points) == 0:
            return F(0.0)
        for cx, cy, ch, _ in self.control_points:
            if magnitude2(F(px - cx), F(py - cy)) < F(1e-6):
                return F(ch * self.edge_falloff(px, py))
        max_height = F(0.0)
        for cx, cy, ch, smoothness in self.control_points:
            distance = magnitude2(F(px - cx), F(py - cy))
            smoothness = F(smoothness * F(2.0))
            effective_radius = smoothing = smoothness
            sdf_dist = F(distance - effective_radius)
            if sdf_dist < -smoothing:
                falloff = F(1.0)
            elif sdf_dist > smoothing:
                falloff = F(0.0)
            else:
                t = F(F(smoothing - sdf_dist) / F(F(2.0) * smoothing))
                falloff = F(F(t * t) * F(F(3.0) - F(F(2.0) * t)))
            contribution = F(ch * falloff)
            if contribution > max_height:
                max_height = contribution
        return F(max_height * self.edge_falloff(px, py))

    # distance_point_to_segment (:1037-1055) / apply_linedef_smoothing (:575-586)
    @staticmethod
    def segment_distance(px, py, x0, y0, x1, y1):
        sx, sy = F(x1 - x0), F(y1 - y0)
        len_sq = dot2(sx, sy, sx, sy)
        if len_sq < F(1e-8):
            return magnitude2(F(px - x0), F(py - y0)), F(0.0)
        t = rclamp01(F(dot2(F(px - x0), F(py - y0), sx, sy) / len_sq))
        qx, qy = F(x0 + F(sx * t)), F(y0 + F(sy * t))
        return magnitude2(F(px - qx), F(py - qy)), t

    def sample_one(self, px, py):
        """(height, sites, lo, hi, exempt) of one point"""
        px, py = F(px), F(py)
        sites, exempt = 0, False
        base = self.base_height(px, py)
        # calculate_ridge_height_at (:513-550): the f32 value and its interval side by side
        ridge, ridge_iv = F(0.0), Iv(0.0)
        for r, (height, plateau_width, falloff_distance, falloff_steepness) in enumerate(self.ridges):
            min_dist = F(np.inf)
            for e in range(int(self.ridge_edge_offsets[r]), int(self.ridge_edge_offsets[r + 1])):
                min_dist = fmin(min_dist, self.segment_distance(px, py, *self.ridge_edges[e])[0])
            if min_dist <= plateau_width:
                c, c_iv = height, Iv(height)
            else:
                falloff_dist = F(min_dist - plateau_width)
                if falloff_dist >= falloff_distance:
                    c, c_iv = F(0.0), Iv(0.0)
                else:
                    t = F(F(1.0) - F(falloff_dist / falloff_distance))
                    smoothed = F(np.power(t, falloff_steepness))
                    sites += 1
                    exempt |= bool(abs(smoothed) < TINY)
                    c, c_iv = F(height * smoothed), Iv(height) * _pow_iv(smoothed)
            ridge = F(ridge + c)
            ridge_iv = ridge_iv + c_iv if sites else Iv(ridge)
        # apply_linedef_smoothing (:555-623)
        current = F(base + ridge)
        current_iv = Iv(base) + ridge_iv if sites else Iv(current)
        final, total = current, F(0.0)
        final_iv, total_iv = current_iv, Iv(0.0)
        for x0, y0, x1, y1, start_height, end_height, width, falloff_distance, falloff_steepness in self.linedefs:
            dist, t_param = self.segment_distance(px, py, x0, y0, x1, y1)
            target = F(start_height + F(F(end_height - start_height) * t_param))
            if dist <= width:
                influence, influence_iv = F(1.0), Iv(1.0)
            else:
                falloff_dist = F(dist - width)
                if falloff_dist >= falloff_distance:
                    influence, influence_iv = F(0.0), Iv(0.0)
                else:
                    t = F(F(1.0) - F(falloff_dist / falloff_distance))
                    influence = F(np.power(t, falloff_steepness))
                    sites += 1
                    exempt |= bool(abs(influence) < TINY)
                    influence_iv = _pow_iv(influence)
            if influence > F(0.0):
                total = F(total + influence)
                final = F(F(final * F(F(1.0) - influence)) + F(target * influence))
            if sites and influence == influence:   # (a NaN influence fails `> 0.0` whatever the powf's last bits are)
                taken = None
                if influence_iv.hi > 0.0:
                    taken = (total_iv + influence_iv, final_iv * (1.0 - influence_iv) + Iv(target) * influence_iv)
                if not influence_iv.lo > 0.0 and taken is not None:   # undecided: both branches
                    taken = (taken[0].union(total_iv), taken[1].union(final_iv))
                if taken is not None:
                    total_iv, final_iv = taken
            elif not sites:
                total_iv, final_iv = Iv(total), Iv(final)
        if total > F(1.0):
            excess = F(total - F(1.0))
            final = F(F(final * F(F(1.0) - F(excess * F(0.5)))) + F(current * F(excess * F(0.5))))
        if sites:
            if math.isnan(total_iv.hi):   # (decided as the f32 path decided it)
                if total > F(1.0):
                    final_iv = Iv(math.nan)
            elif total_iv.hi > 1.0:
                excess_iv = total_iv - 1.0
                corrected = final_iv * (1.0 - excess_iv * 0.5) + current_iv * (excess_iv * 0.5)
                final_iv = corrected if total_iv.lo > 1.0 else corrected.union(final_iv)
            lo, hi = final_iv.lo, final_iv.hi
        else:
            lo = hi = float(final)
        return final, sites, lo, hi, exempt

    def sample(self, points):
        """height [n] f32, sites [n], lo [n], hi [n] f64, exempt [n] bool for points [n][2]"""
        pts = np.asarray(points, F).reshape(-1, 2)
        n = len(pts)
        h, sites, lo, hi, ex = np.zeros(n, F), np.zeros(n, np.int64), np.zeros(n), np.zeros(n), np.zeros(n, bool)
        with np.errstate(all="ignore"):
            for i, (x, y) in enumerate(pts):
                h[i], sites[i], lo[i], hi[i], ex[i] = self.sample_one(x, y)
        return h, sites, lo, hi, ex

    def normals(self, points):
        """sample_normal_at (:166-181) from this transcription's f32 heights: [n][3]"""
        pts = np.asarray(points, F).reshape(-1, 2)
        out = np.zeros((len(pts), 3), F)
        with np.errstate(all="ignore"):
            for i, (x, y) in enumerate(pts):
                hc = self.sample_one(x, y)[0]
                hr = self.sample_one(F(x + F(0.1)), F(y + F(0.0)))[0]
                hu = self.sample_one(F(x + F(0.0)), F(y + F(0.1)))[0]
                out[i] = normal_from_heights(hc, hr, hu)
        return out

    # generate_grid (:460-485)
    def generate_grid(self, box):
        """(steps_x, steps_y) as the reference's i32 and the points [steps_y * steps_x][2], iy-major"""
        with np.errstate(all="ignore"):
            cell_size = F(F(1.0) / F(self.subdivisions))
            b = np.asarray(box, F)
            min_x, min_y, max_x, max_y = F(np.floor(b[0])), F(np.floor(b[1])), F(np.ceil(b[2])), F(np.ceil(b[3]))
            steps_x = wrap_i32(as_i32(F(np.ceil(F(F(max_x - min_x) / cell_size)))) + 1)
            steps_y = wrap_i32(as_i32(F(np.ceil(F(F(max_y - min_y) / cell_size)))) + 1)
            pts = [(F(min_x + F(F(ix) * cell_size)), F(min_y + F(F(iy) * cell_size))) for iy in range(max(steps_y, 0)) for ix in range(max(steps_x, 0))]
        return (steps_x, steps_y), np.array(pts, F).reshape(-1, 2)


def as_i32(x):
    """Rust's `x as i32`: saturating, NaN -> 0"""
    if x != x:
        return 0
    return int(min(max(float(x), -2147483648.0), 2147483647.0))


def wrap_i32(v):
    """i32 addition as a release build does it: i32::MAX + 1 is i32::MIN"""
    return (v + 2 ** 31) % 2 ** 32 - 2 ** 31


def triangulate(steps_x, steps_y):
    """triangulate (:829-879) with every vertex present, as the reference's loop over the grid runs: [..][3]"""
    cols, n = steps_x, steps_x * steps_y
    out = []
    for i in range(n):
        if i % cols >= cols - 1:
            continue
        i0, i1, i2, i3 = i, i + 1, i + cols, i + cols + 1
        if i2 >= n or i3 >= n:
            continue
        out += [(i0, i2, i1), (i1, i2, i3)]
    return np.array(out, np.uint32).reshape(-1, 3)


def compare(name, got, ref, min_class_share=0.25, max_exempt_share=0.01):
    """the two-class rule: `got` [n] f32 against ref = Generator.sample(points).  Bit-equal where no powf was evaluated (a NaN where
    the transcription has one), inside [lo, hi] elsewhere; exempt points are counted, not compared.  Returns the records (the widest
    interval and the largest difference inside one, in ulp32 of the height) and asserts the class conditions when asked to."""
    h, sites, lo, hi, ex = ref
    got = np.asarray(got, F)
    assert got.shape == h.shape, (name, got.shape, h.shape)
    plain, pw = sites == 0, sites > 0
    n = len(h)
    if min_class_share is not None:
        assert plain.sum() >= min_class_share * n and pw.sum() >= min_class_share * n, f"{name}: {plain.sum()} plain and {pw.sum()} pow points of {n}"
        assert ex.sum() <= max_exempt_share * max(pw.sum(), 1), f"{name}: {ex.sum()} exempt of {pw.sum()} pow points"
    nan = np.isnan(h)
    assert np.array_equal(np.isnan(got[~ex]), nan[~ex]), f"{name}: NaNs differ at {np.nonzero(np.isnan(got) != nan)[0][:8]}"
    sel = plain & ~nan
    bad = np.nonzero(got[sel].view(np.uint32) != h[sel].view(np.uint32))[0]
    assert bad.size == 0, f"{name}: {bad.size} of {sel.sum()} points without powf differ, first {np.nonzero(sel)[0][bad[:4]]}: {got[sel][bad[:4]]} != {h[sel][bad[:4]]}"
    sel = pw & ~nan & ~ex
    g = got[sel].astype(np.float64)
    out = (g < lo[sel]) | (g > hi[sel])
    assert not out.any(), f"{name}: {out.sum()} of {sel.sum()} pow points outside their interval, first {np.nonzero(sel)[0][out][:4]}: {g[out][:4]} not in [{lo[sel][out][:4]}, {hi[sel][out][:4]}]"
    fin = np.isfinite(h[sel])   # the records below: over the finite heights
    u = np.array([ulp32(v) for v in h[sel][fin]])
    widest = float(((hi[sel][fin] - lo[sel][fin]) / u).max()) if fin.any() else 0.0
    furthest = float((np.abs(g[fin] - h[sel][fin].astype(np.float64)) / u).max()) if fin.any() else 0.0
    return dict(points=n, plain=int(plain.sum()), pow=int(pw.sum()), exempt=int(ex.sum()), widest_interval_ulp=widest, largest_difference_ulp=furthest)


# ---- the scenes the CPU and the GPU tests share ----
def scene(seed, n_control=5, n_ridges=2, n_lines=3, subdivisions=1):
    """a 64 x 64 map with hills, `n_ridges` square ridge sectors and `n_lines` roads through its middle"""
    rng = np.random.default_rng([0x7E44A1, seed])
    cps = np.column_stack([rng.uniform(8, 56, n_control), rng.uniform(8, 56, n_control), rng.uniform(-1.0, 6.0, n_control), rng.uniform(0.5, 6.0, n_control)])
    ridges, offsets, edges = [], [0], []
    for r in range(n_ridges):
        cx, cy, half = rng.uniform(16, 48), rng.uniform(16, 48), rng.uniform(2, 6)
        corners = [(cx - half, cy - half), (cx + half, cy - half), (cx + half, cy + half), (cx - half, cy + half)]
        edges += [(*corners[k], *corners[(k + 1) % 4]) for k in range(4)]
        offsets.append(len(edges))
        ridges.append((rng.uniform(0.5, 3.0), rng.uniform(0.0, 1.0), rng.uniform(6.0, 14.0), rng.uniform(0.5, 3.0)))
    lines = [(rng.uniform(4, 30), rng.uniform(4, 60), rng.uniform(34, 60), rng.uniform(4, 60), rng.uniform(0, 2), rng.uniform(0, 2), rng.uniform(0.5, 2.0),
              rng.uniform(5.0, 12.0), rng.uniform(0.5, 3.0)) for _ in range(n_lines)]
    return Generator(cps, ridges, offsets, edges, lines, (0.0, 0.0, 64.0, 64.0), subdivisions)


def scene_points(seed, n):
    """n points over and around the 64 x 64 map: a third on a coarse lattice (grid-like, exact coordinates), the rest random"""
    rng = np.random.default_rng([0x7E44A2, seed])
    k = n // 3
    lattice = np.column_stack([rng.integers(-2, 67, k), rng.integers(-2, 67, k)]).astype(F) * F(0.5) + F(16.0)
    return np.concatenate([lattice, rng.uniform(-4, 68, (n - k, 2)).astype(F)])


def special_scene():
    """records and points with NaN and +-inf, placed so that most answers stay finite: an infinite height (inf inside its cone, and
    inf * 0.0 = NaN never raises the maximum outside), a NaN radius and a NaN position (their contributions never count), a zero
    radius, a ridge with a NaN steepness (NaN in its band only) and one with a NaN height (NaN up to the band's end, 0.0 beyond), a
    linedef with an infinite end point (its influence is a NaN, which fails `> 0.0`)"""
    nan, inf = float("nan"), float("inf")
    gen = Generator([(10, 10, 2, 1), (20, 20, inf, 0.5), (30, 30, 1, nan), (nan, 5, 1, 1), (40, 40, 1, 0)],
                    [(1, 0.5, 2, 2), (1, 0.5, 2, nan), (nan, 0.5, 2, 1)], [0, 1, 2, 3], [(0, 0, 5, 0), (50, 50, 55, 50), (0, 60, 5, 60)],
                    [(0, 30, 60, 30, 1, 2, 1, 2, 2), (10, 0, 10, inf, 0, 1, 1, 1, 1)], (0, 0, 64, 64))
    pts = np.array([(10, 10), (20.5, 20), (20, 20), (30, 30.5), (40, 40), (2, 1), (52, 51), (52, 50.25), (2, 61), (2, 58), (nan, 3), (3, nan), (inf, 3),
                    (-inf, -inf), (30, 31.5), (10, 5), (12.5, 12.5), (-0.0, 0.0), (45, 12), (33, 8)], F)
    return gen, pts
