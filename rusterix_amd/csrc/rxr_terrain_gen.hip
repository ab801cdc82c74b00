// rxr_terrain_gen.hip -- the generated terrain's height field: TerrainGenerator::sample_height_at (src/chunkbuilder/terrain_generator.rs:57-163),
// which is interpolate_height_at (:650-714) with calculate_map_edge_falloff (:718-743), calculate_ridge_height_at (:513-550) over
// distance_point_to_segment (:1037-1055) and apply_linedef_smoothing (:555-623); sample_normal_at (:166-181); the grids of
// generate_grid (:460-485).  include/rxr.h: rxr_check_terrain_generator, rxr_set_terrain_generator, rxr_generated_heights(_to),
// rxr_generated_grids(_to).
//
// Semantics, per point, all f32, one operation per reference operation in its order, nothing fused (the build's -ffp-contract=off),
// divisions and square roots correctly rounded (rxr_exact_math.h):
//   * base: with no control points 0.0, WITHOUT the edge factor.  Else the exact-match scan (magnitude(point - cp) < 1e-6) runs over
//     ALL control points before the cones: the FIRST control point in list order that matches wins and the base is its
//     height * edge_factor, the cones are not looked at (ridges and linedefs still apply).  Else the maximum over the cones
//     height * falloff, which starts at +0.0 and takes a contribution only under `>`: negative and NaN contributions never count.
//     (One loop here: the magnitude of the scan and the cone's distance are the same operations on the same operands.)
//   * edge factor: f32::min skips a NaN; <= 0.0 gives 0.0, >= 10.0 gives 1.0, else the smoothstep of min / 10.0.
//   * ridges: the distance to a ridge's edges starts at +inf and is lowered by f32::min (a NaN distance is skipped); a ridge without
//     edges keeps +inf and contributes 0.0 (or its height where the plateau width is +inf).  Contributions are added in list order
//     to a sum that starts at 0.0.
//   * clamp(0.0, 1.0) keeps a NaN and keeps -0.0.
//   * linedefs are folded in list order, only when influence > 0.0; the over-influence correction (total_influence > 1.0) comes
//     at the end and blends back towards the height before the first linedef.
//   * TerrainConfig's idw_power and max_influence_distance are read by nothing in the reference: they do not cross this boundary.
//   * powf is the device libm call the Pow opcode of rxr_vm.h makes: the only operation here that is not bit-defined.
// Hoisted into the set-up pass (rxr_set_terrain_generator, on the host, in the same f32 operations -- the same operation on the same
// operands gives the same bits): a segment's seg = end - start, len_sq = seg.x * seg.x + seg.y * seg.y and its degenerate test
// len_sq < 1e-8; a control point's radius smoothness * 2.0 and 2.0 * radius; a linedef's end_height - start_height.  Nothing else
// is reassociated.
//
// Layout: one point per lane, wave64, workgroups of 256.  The record loops run on a wave-uniform index over read-only arrays, so the
// records arrive in scalar registers (s_load_dwordx4 / x8: no vector memory traffic, no LDS) and every lane's arithmetic is VALU on
// one scalar operand set.  A normal's three height samples (p, p + (0.1, 0.0), p + (0.0, 0.1)) run in the same loops as three
// points of the lane: the records are walked once.  A call is cut into launches of bounded work, points x records
// (RXR_TERRAIN_GEN_LAUNCH_POINTS overrides the points a launch).  Nothing a queued launch reads can change under it except the
// resident records, which rxr_set_terrain_generator replaces only after rxr_quiesce.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "rxr_debug.h"
#include "rxr_terrain_gen.h"

#define GEN_LAUNCH_BOXES 128u   // boxes a grid launch carries in its arguments (16 bytes each)

struct GenPointArgs {
    GenRecords G;
    const float *points;   // [n][2]
    uint32_t first, end;   // the points of this launch
    float *heights;        // [n]
    float *normals;        // [n][3], k_terrain_gen_normals only
};
struct GenGridArgs {
    GenRecords G;
    GenBox box[GEN_LAUNCH_BOXES];
    float cell_size;
    uint32_t stride;        // heights of box b of this launch start at heights + b * stride
    float *heights;
    uint32_t *counts;       // [boxes of this launch][2]
};

using namespace rxgen;   // rxr_terrain_gen.h: the records, sample_height_at (gen_eval), generate_grid's bounds

extern "C" __global__ __launch_bounds__(GEN_WG) void k_terrain_gen_heights(GenPointArgs A) {
    const uint32_t j = blockIdx.x * GEN_WG + threadIdx.x;   // (at most 2^30 + 255: the sum below cannot wrap for a live lane)
    const bool live = j < A.end - A.first;
    const uint32_t i = A.first + j;
    const float *p = A.points + 2 * (size_t)(live ? i : A.first);   // (a lane past the end repeats a point and stores nothing)
    const float px[1] = {p[0]}, py[1] = {p[1]};
    float h[1];
    gen_eval<1>(A.G, px, py, h);
    if (live) A.heights[i] = h[0];
}

// ... with sample_normal_at (:166-181)
extern "C" __global__ __launch_bounds__(GEN_WG) void k_terrain_gen_normals(GenPointArgs A) {
    const uint32_t j = blockIdx.x * GEN_WG + threadIdx.x;   // (at most 2^30 + 255: the sum below cannot wrap for a live lane)
    const bool live = j < A.end - A.first;
    const uint32_t i = A.first + j;
    const float *p = A.points + 2 * (size_t)(live ? i : A.first);
    const float delta = 0.1f;
    const float px[3] = {p[0], p[0] + delta, p[0] + 0.0f}, py[3] = {p[1], p[1] + 0.0f, p[1] + delta};
    float h[3];
    gen_eval<3>(A.G, px, py, h);
    // tangent_x = (delta, h_right - h_center, 0.0), tangent_z = (0.0, h_up - h_center, delta); cross, normalized
    const float ax = delta, ay = h[1] - h[0], az = 0.0f, bx = 0.0f, by = h[2] - h[0], bz = delta;
    const float cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
    float nx, ny, nz, mag;
    rxm::normalize3(cx, cy, cz, nx, ny, nz, mag);
    if (!live) return;
    A.heights[i] = h[0];
    float *o = A.normals + 3 * (size_t)i;
    o[0] = nx, o[1] = ny, o[2] = nz;
}

// grid (blockIdx.y = the box of this launch, blockIdx.x * GEN_WG + threadIdx.x = iy * steps_x + ix): generate_grid (:460-485)
extern "C" __global__ __launch_bounds__(GEN_WG) void k_terrain_gen_grid(GenGridArgs A) {
    const GenBox b = A.box[blockIdx.y];
    const uint32_t count = (uint32_t)b.sx * (uint32_t)b.sy;   // (<= stride: checked on the host)
    // (the box's counts are stored behind the record loops, as every store is: a store ahead of them would turn the records' scalar
    // loads into vector loads)
    const bool writes_counts = blockIdx.x == 0u && threadIdx.x == 0u;
    if (blockIdx.x * GEN_WG >= count) {   // (the whole workgroup: an empty grid, or a shorter one than the launch's longest)
        if (writes_counts) A.counts[2u * blockIdx.y] = (uint32_t)b.sx, A.counts[2u * blockIdx.y + 1u] = (uint32_t)b.sy;
        return;
    }
    const uint32_t j = blockIdx.x * GEN_WG + threadIdx.x;
    const bool live = j < count;
    const uint32_t jj = live ? j : 0u;
    const uint32_t iy = jj / (uint32_t)b.sx, ix = jj - iy * (uint32_t)b.sx;
    const float px[1] = {b.min_x + (float)(int32_t)ix * A.cell_size}, py[1] = {b.min_y + (float)(int32_t)iy * A.cell_size};
    float h[1];
    gen_eval<1>(A.G, px, py, h);
    if (live) A.heights[(size_t)blockIdx.y * A.stride + j] = h[0];
    if (writes_counts) A.counts[2u * blockIdx.y] = (uint32_t)b.sx, A.counts[2u * blockIdx.y + 1u] = (uint32_t)b.sy;
}

namespace {

struct GenCounts {
    uint32_t C, R, E, L;
};

int check_generator(const float *cps, uint32_t C, const float *ridges, uint32_t R, const uint32_t *off, const float *edges, uint32_t E, const float *lines,
                    uint32_t L, const float *map_box, std::string &err) {
    auto bad = [&](int code, const std::string &m) {
        err = m;
        return code;
    };
    if (C > RXR_TERRAIN_GEN_MAX_CONTROL_POINTS) return bad(RXR_ERR_UNSUPPORTED, std::to_string(C) + " control points exceed RXR_TERRAIN_GEN_MAX_CONTROL_POINTS");
    if (R > RXR_TERRAIN_GEN_MAX_RIDGES) return bad(RXR_ERR_UNSUPPORTED, std::to_string(R) + " ridges exceed RXR_TERRAIN_GEN_MAX_RIDGES");
    if (E > RXR_TERRAIN_GEN_MAX_RIDGE_EDGES) return bad(RXR_ERR_UNSUPPORTED, std::to_string(E) + " ridge edges exceed RXR_TERRAIN_GEN_MAX_RIDGE_EDGES");
    if (L > RXR_TERRAIN_GEN_MAX_LINEDEFS) return bad(RXR_ERR_UNSUPPORTED, std::to_string(L) + " linedefs exceed RXR_TERRAIN_GEN_MAX_LINEDEFS");
    if (!map_box) return bad(RXR_ERR_INVALID, "NULL map_box");
    if (C && !cps) return bad(RXR_ERR_INVALID, "NULL control_points");
    if (R && !ridges) return bad(RXR_ERR_INVALID, "NULL ridges");
    if (R && !off) return bad(RXR_ERR_INVALID, "NULL ridge_edge_offsets");
    if (E && !edges) return bad(RXR_ERR_INVALID, "NULL ridge_edges");
    if (L && !lines) return bad(RXR_ERR_INVALID, "NULL linedefs");
    if (!R && E) return bad(RXR_ERR_INVALID, "ridge edges without a ridge");
    if (R) {
        if (off[0] != 0u) return bad(RXR_ERR_INVALID, "ridge_edge_offsets[0] must be 0");
        for (uint32_t r = 0; r < R; ++r)
            if (off[r + 1] < off[r]) return bad(RXR_ERR_INVALID, "ridge_edge_offsets[" + std::to_string(r + 1) + "] is below its predecessor");
        if (off[R] != E) return bad(RXR_ERR_INVALID, "ridge_edge_offsets[n_ridges] = " + std::to_string(off[R]) + " is not n_ridge_edges = " + std::to_string(E));
    }
    return RXR_OK;
}

// the set-up pass of a segment: seg, len_sq and the degenerate test (:1042-1045, :575-578)
void segment_record(const float *s, float *o) {
    const float sx = s[2] - s[0], sy = s[3] - s[1];
    const float len_sq = sx * sx + sy * sy;
    o[0] = s[0], o[1] = s[1], o[2] = sx, o[3] = sy, o[4] = len_sq, o[5] = len_sq < 1e-8f ? 1.0f : 0.0f;
}

// the points a launch takes: the bound on points x records, or the environment's
uint32_t launch_points(const rxr_ctx *ctx, uint32_t samples) {
    if (const char *e = getenv("RXR_TERRAIN_GEN_LAUNCH_POINTS")) {
        const unsigned long long v = strtoull(e, nullptr, 10);
        if (v) return (uint32_t)std::min<unsigned long long>(v, 1u << 30);   // (the bound below holds for the override as well)
    }
    const unsigned long long records = std::max<unsigned long long>(1, ((unsigned long long)ctx->gen_n[0] + ctx->gen_n[2] + ctx->gen_n[3]) * samples);
    return (uint32_t)std::min<unsigned long long>(std::max<unsigned long long>(GEN_LAUNCH_WORK / records, GEN_WG), 1u << 30);
}

// every point of a call on device arrays, queued on `s`
int points_run(rxr_ctx *ctx, const float *points, uint32_t n, float *heights, float *normals, hipStream_t s) {
    const uint32_t bound = launch_points(ctx, normals ? 3u : 1u);
    GenPointArgs A{};
    A.G = records_of(ctx);
    A.points = points;
    A.heights = heights;
    A.normals = normals;
    const int rc = rxr_query_begin(ctx, ctx->lane[Q_GEN], s);
    if (rc != RXR_OK) return rc;
    ctx->gen_launches = 0;
    for (uint32_t first = 0; first < n;) {
        const uint32_t count = std::min(n - first, bound);
        A.first = first;
        A.end = first + count;
        const dim3 grid((count + GEN_WG - 1u) / GEN_WG);
        if (normals) hipLaunchKernelGGL(k_terrain_gen_normals, grid, dim3(GEN_WG), 0, s, A);
        else hipLaunchKernelGGL(k_terrain_gen_heights, grid, dim3(GEN_WG), 0, s, A);
        HIPCHK(ctx, hipGetLastError());
        ++ctx->gen_launches;
        first += count;
    }
    return rxr_query_end(ctx, ctx->lane[Q_GEN], s);
}

// generate_grid's bounds of every box (:464-474); refuses what the call cannot hold
int grid_boxes(rxr_ctx *ctx, const char *who, const float *boxes, uint32_t n, uint32_t subdivisions, uint32_t stride, std::vector<GenBox> &out, float &cell_size) {
    const std::string w = who;
    if (!ctx->gen_set) return rxr_fail(ctx, RXR_ERR_INVALID, w + ": no terrain generator is resident (rxr_set_terrain_generator)");
    if (!subdivisions) return rxr_fail(ctx, RXR_ERR_INVALID, w + ": subdivisions must be at least 1 (the reference divides by it)");
    if (n && !boxes) return rxr_fail(ctx, RXR_ERR_INVALID, w + ": NULL boxes");
    size_t total;
    if (__builtin_mul_overflow((size_t)n, (size_t)stride * 4u, &total)) return rxr_fail(ctx, RXR_ERR_INVALID, w + ": the height array's size overflows");
    cell_size = 1.0f / (float)subdivisions;
    out.resize(n);
    for (uint32_t i = 0; i < n; ++i) {
        const float *b = boxes + 4 * (size_t)i;
        const float min_x = std::floor(b[0]), min_y = std::floor(b[1]), max_x = std::ceil(b[2]), max_y = std::ceil(b[3]);
        // (`as i32 + 1` on a saturated cast wraps, as in a release build of the reference: a negative step, an empty grid)
        const int32_t sx = (int32_t)((uint32_t)as_i32(std::ceil((max_x - min_x) / cell_size)) + 1u);
        const int32_t sy = (int32_t)((uint32_t)as_i32(std::ceil((max_y - min_y) / cell_size)) + 1u);
        const int64_t cx = std::max<int64_t>(sx, 0), cy = std::max<int64_t>(sy, 0);
        if (cx * cy > (int64_t)stride)
            return rxr_fail(ctx, RXR_ERR_INVALID, w + ": box " + std::to_string(i) + " has a grid of " + std::to_string(cx) + " x " + std::to_string(cy) + " points, more than the stride " + std::to_string(stride));
        out[i] = GenBox{min_x, min_y, (int32_t)cx, (int32_t)cy};
    }
    return RXR_OK;
}

// every box of a call into device arrays, queued on `s`
int grids_run(rxr_ctx *ctx, const std::vector<GenBox> &boxes, float cell_size, uint32_t stride, uint32_t *counts, float *heights, hipStream_t s) {
    const uint32_t n = (uint32_t)boxes.size();
    const uint32_t bound = launch_points(ctx, 1u);
    const int rc = rxr_query_begin(ctx, ctx->lane[Q_GEN], s);
    if (rc != RXR_OK) return rc;
    ctx->gen_launches = 0;
    GenGridArgs A{};
    A.G = records_of(ctx);
    A.cell_size = cell_size;
    A.stride = stride;
    for (uint32_t b0 = 0; b0 < n;) {
        // boxes of this launch: up to GEN_LAUNCH_BOXES, and up to `bound` points (at least one box)
        uint32_t nb = 0, most = 0;
        unsigned long long points = 0;
        while (b0 + nb < n && nb < GEN_LAUNCH_BOXES) {
            const uint32_t c = (uint32_t)boxes[b0 + nb].sx * (uint32_t)boxes[b0 + nb].sy;
            if (nb && points + c > bound) break;
            A.box[nb] = boxes[b0 + nb];
            points += c;
            most = std::max(most, c);
            ++nb;
        }
        A.heights = heights + (size_t)b0 * stride;
        A.counts = counts + 2 * (size_t)b0;
        // (a launch of empty grids still writes their counts)
        hipLaunchKernelGGL(k_terrain_gen_grid, dim3(std::max((most + GEN_WG - 1u) / GEN_WG, 1u), nb), dim3(GEN_WG), 0, s, A);
        HIPCHK(ctx, hipGetLastError());
        ++ctx->gen_launches;
        b0 += nb;
    }
    return rxr_query_end(ctx, ctx->lane[Q_GEN], s);
}

}  // namespace

extern "C" {

int rxr_check_terrain_generator(const float *control_points, uint32_t n_control_points, const float *ridges, uint32_t n_ridges, const uint32_t *ridge_edge_offsets,
                                const float *ridge_edges, uint32_t n_ridge_edges, const float *linedefs, uint32_t n_linedefs, const float map_box[4],
                                char *message, uint32_t message_capacity) {
    std::string err;
    const int rc = check_generator(control_points, n_control_points, ridges, n_ridges, ridge_edge_offsets, ridge_edges, n_ridge_edges, linedefs, n_linedefs, map_box, err);
    rxr_copy_message(err, message, message_capacity);
    return rc;
}

int rxr_set_terrain_generator(rxr_ctx *ctx, const float *control_points, uint32_t n_control_points, const float *ridges, uint32_t n_ridges,
                              const uint32_t *ridge_edge_offsets, const float *ridge_edges, uint32_t n_ridge_edges, const float *linedefs, uint32_t n_linedefs,
                              const float map_box[4]) {
    if (!ctx) return RXR_ERR_INVALID;
    if (ctx->group)
        return rxr_as_member0(ctx, [&](rxr_ctx *m) {
            return rxr_set_terrain_generator(m, control_points, n_control_points, ridges, n_ridges, ridge_edge_offsets, ridge_edges, n_ridge_edges, linedefs, n_linedefs, map_box);
        });
    const uint32_t C = n_control_points, R = n_ridges, E = n_ridge_edges, L = n_linedefs;
    std::string err;
    int rc = check_generator(control_points, C, ridges, R, ridge_edge_offsets, ridge_edges, E, linedefs, L, map_box, err);
    if (rc != RXR_OK) return rxr_fail(ctx, rc, "rxr_set_terrain_generator: " + err);
    // the device records, with what does not depend on the point computed here (the header comment: same operations, same bits)
    BlobCursor take;
    const size_t off[5] = {take((size_t)C * GEN_CP_FLOATS * 4), take((size_t)R * 16), take(((size_t)R + 1) * 4), take((size_t)E * GEN_EDGE_FLOATS * 4),
                           take((size_t)L * GEN_LINE_FLOATS * 4)};
    std::vector<uint8_t> blob(take.o, 0);
    float *cp = (float *)(blob.data() + off[0]);
    for (uint32_t i = 0; i < C; ++i) {
        const float *s = control_points + RXR_TERRAIN_GEN_CONTROL_POINT_FLOATS * (size_t)i;
        float *o = cp + GEN_CP_FLOATS * (size_t)i;
        const float radius = s[3] * 2.0f;
        o[0] = s[0], o[1] = s[1], o[2] = s[2], o[3] = radius, o[4] = 2.0f * radius;
    }
    if (R) memcpy(blob.data() + off[1], ridges, (size_t)R * 16);
    uint32_t *ro = (uint32_t *)(blob.data() + off[2]);
    for (uint32_t r = 0; r <= R; ++r) ro[r] = R ? ridge_edge_offsets[r] : 0u;
    float *ed = (float *)(blob.data() + off[3]);
    for (uint32_t e = 0; e < E; ++e) segment_record(ridge_edges + RXR_TERRAIN_GEN_RIDGE_EDGE_FLOATS * (size_t)e, ed + GEN_EDGE_FLOATS * (size_t)e);
    float *ln = (float *)(blob.data() + off[4]);
    for (uint32_t l = 0; l < L; ++l) {
        const float *s = linedefs + RXR_TERRAIN_GEN_LINEDEF_FLOATS * (size_t)l;
        float *o = ln + GEN_LINE_FLOATS * (size_t)l;
        segment_record(s, o);
        o[6] = s[4], o[7] = s[5] - s[4], o[8] = s[6], o[9] = s[7], o[10] = s[8];
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if ((rc = rxr_quiesce(ctx)) != RXR_OK) return rc;   // queued evaluations read what is replaced here
    ctx->gen_set = false;
    if ((rc = rxr_ensure(ctx, ctx->d_gen, std::max<size_t>(blob.size(), 256))) != RXR_OK) return rc;
    HIPCHK(ctx, hipMemcpyAsync(ctx->d_gen.p, blob.data(), blob.size(), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // (the blob is read until here)
    for (int i = 0; i < 5; ++i) ctx->gen_off[i] = off[i];
    ctx->gen_n[0] = C, ctx->gen_n[1] = R, ctx->gen_n[2] = E, ctx->gen_n[3] = L;
    memcpy(ctx->gen_box, map_box, sizeof ctx->gen_box);
    ctx->gen_set = true;
    return RXR_OK;
}

int rxr_generated_heights(rxr_ctx *ctx, const float *points, uint32_t n, float *heights, float *normals) {
    if (!ctx) return RXR_ERR_INVALID;
    if (ctx->group) return rxr_as_member0(ctx, [&](rxr_ctx *m) { return rxr_generated_heights(m, points, n, heights, normals); });
    if (!ctx->gen_set) return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_generated_heights: no terrain generator is resident (rxr_set_terrain_generator)");
    if (!n) return RXR_OK;
    if (!points || !heights) return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_generated_heights: NULL point or height array");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    QueryIO io{ctx, ctx->lane[Q_GEN]};
    const unsigned i_p = io.in(points, (size_t)n * 8), i_h = io.out(heights, (size_t)n * 4), i_n = io.out(normals, (size_t)n * 12);
    int rc = io.upload();
    if (rc != RXR_OK) return rc;
    if ((rc = points_run(ctx, io.dev<float>(i_p), n, io.dev<float>(i_h), io.dev<float>(i_n), ctx->stream)) != RXR_OK) return rc;
    return io.download();
}

int rxr_generated_heights_to(rxr_ctx *ctx, const float *dev_points, uint32_t n, float *dev_heights, float *dev_normals, void *hip_stream) {
    if (!ctx) return RXR_ERR_INVALID;
    if (ctx->group) return rxr_fail(ctx, RXR_ERR_UNSUPPORTED, "rxr_generated_heights_to on a multi-device context: device pointers and streams belong to ONE device (use rxr_member)");
    if (!ctx->gen_set) return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_generated_heights_to: no terrain generator is resident (rxr_set_terrain_generator)");
    if (!n) return RXR_OK;
    if (!dev_points || !dev_heights) return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_generated_heights_to: NULL point or height array");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const void *const p[3] = {dev_points, dev_heights, dev_normals};
    const size_t bytes[3] = {(size_t)n * 8, (size_t)n * 4, (size_t)n * 12};
    const char *const names[3] = {"dev_points", "dev_heights", "dev_normals"};
    const int rc = device_arrays(ctx, "rxr_generated_heights_to", p, bytes, names, 3);
    if (rc != RXR_OK) return rc;
    return points_run(ctx, dev_points, n, dev_heights, dev_normals, hip_stream ? (hipStream_t)hip_stream : ctx->stream);
}

int rxr_generated_grids(rxr_ctx *ctx, const float *boxes, uint32_t n, uint32_t subdivisions, uint32_t stride, uint32_t *counts, float *heights) {
    if (!ctx) return RXR_ERR_INVALID;
    if (ctx->group) return rxr_as_member0(ctx, [&](rxr_ctx *m) { return rxr_generated_grids(m, boxes, n, subdivisions, stride, counts, heights); });
    std::vector<GenBox> gb;
    float cell_size;
    int rc = grid_boxes(ctx, "rxr_generated_grids", boxes, n, subdivisions, stride, gb, cell_size);
    if (rc != RXR_OK) return rc;
    if (!n) return RXR_OK;
    if (!counts || (!heights && stride)) return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_generated_grids: NULL output array");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // the heights go up as well as down: the slots past a box's count come back as the caller left them
    QueryIO io{ctx, ctx->lane[Q_GEN]};
    const unsigned i_c = io.out(counts, (size_t)n * 8), i_h = io.inout(heights, (size_t)n * stride * 4);
    if ((rc = io.upload()) != RXR_OK) return rc;
    if ((rc = grids_run(ctx, gb, cell_size, stride, io.dev<uint32_t>(i_c), io.dev<float>(i_h), ctx->stream)) != RXR_OK) return rc;
    return io.download();
}

int rxr_generated_grids_to(rxr_ctx *ctx, const float *boxes, uint32_t n, uint32_t subdivisions, uint32_t stride, uint32_t *dev_counts, float *dev_heights,
                           void *hip_stream) {
    if (!ctx) return RXR_ERR_INVALID;
    if (ctx->group) return rxr_fail(ctx, RXR_ERR_UNSUPPORTED, "rxr_generated_grids_to on a multi-device context: device pointers and streams belong to ONE device (use rxr_member)");
    std::vector<GenBox> gb;
    float cell_size;
    int rc = grid_boxes(ctx, "rxr_generated_grids_to", boxes, n, subdivisions, stride, gb, cell_size);
    if (rc != RXR_OK) return rc;
    if (!n) return RXR_OK;
    if (!dev_counts || (!dev_heights && stride)) return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_generated_grids_to: NULL output array");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const void *const p[2] = {dev_counts, stride ? dev_heights : nullptr};
    const size_t bytes[2] = {(size_t)n * 8, (size_t)n * stride * 4};
    const char *const names[2] = {"dev_counts", "dev_heights"};
    if ((rc = device_arrays(ctx, "rxr_generated_grids_to", p, bytes, names, 2)) != RXR_OK) return rc;
    return grids_run(ctx, gb, cell_size, stride, dev_counts, dev_heights, hip_stream ? (hipStream_t)hip_stream : ctx->stream);
}

// test-only: the launches of the last evaluation call
uint32_t rxr_debug_terrain_gen_launches(rxr_ctx *ctx) {
    if (!ctx) return 0;
    if (ctx->group) return rxr_debug_terrain_gen_launches(rxr_member(ctx, 0));
    return ctx->gen_launches;
}

}  // extern "C"
