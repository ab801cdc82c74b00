// rxr_terrain_excl.hip -- the generated terrain's chunk meshes with their excluded sectors cut out: TerrainGenerator::apply_exclusions
// (src/chunkbuilder/terrain_generator.rs:747-825) over collect_excluded_sectors' box test (:438-457, src/map/bbox.rs:43-48) and
// point_in_sector (:891-950), behind generate_grid and interpolate_heights (rxr_terrain_gen.h).  include/rxr.h:
// rxr_check_terrain_exclusions, rxr_set_terrain_exclusions, rxr_generated_meshes(_to).
//
// Semantics, all f32, one operation per reference operation in its order, nothing fused (the build's -ffp-contract=off), divisions and
// square roots correctly rounded (rxr_exact_math.h):
//   * a sector is ACTIVE for a chunk box iff sector.min.x <= box.max.x && sector.max.x >= box.min.x && sector.min.y <= box.max.y &&
//     sector.max.y >= box.min.y on the box as the caller gave it (touching counts, a NaN makes it inactive).  A sector with fewer than
//     three vertices is active like any other and holds no point.
//   * no active sector: the SHARED layout, the grid points (x, h, y, 1) in grid order.  Else the UNSHARED one: the triangles of
//     triangulate in its order -- per cell, row by row, (i0, i2, i1) then (i1, i2, i3) -- but for those whose three corners lie inside
//     ONE active sector; a kept triangle is its three vertices, one after the other.
//   * point_in_sector: the boundary pass (distance to an edge's nearest point < 0.01, over the edges of squared length > 0.0, t
//     clamped as f32::clamp does: a NaN stays) or else the ray cast's parity.  Both passes are pure, so they run in one loop here; a
//     point is inside iff either says so.  The ray cast's crossing abscissa is multiplied, divided, added, as written; where the
//     reference's `&&` skips that division its value is not looked at here either.
// Hoisted into the set-up pass (rxr_set_terrain_exclusions, on the host, in the same f32 operations): an edge's vj - vi, its squared
// length and the `> 0.0` test.  vj.x - vi.x and vj.y - vi.y of the ray cast are that edge's components: the same bits.
//
// Two kernels a round of boxes, and a call scratch between them (heights, then inside-bits):
//   k_terrain_excl_classify   one grid point per lane, blockIdx.y = the box, blockIdx.z = a word of 32 active sectors.  The sector
//       loop runs over ALL resident sectors on a wave-uniform index and repeats the reference's box test -- which sectors are active is
//       decided on the device from the registration, nothing is uploaded per call --; an active sector's rank among the active ones
//       is its bit.  Boxes, offsets and edge records arrive through scalar loads; the lane's arithmetic is VALU on one scalar operand
//       set.  Word 0's workgroups also evaluate the point's height (gen_eval: the word rxr_generated_grids gives).  A lane stores its
//       height and its word BEHIND the loops: a store ahead of them would turn the records' scalar loads into vector loads.  Each
//       point is tested once per active sector; every exit is wave-uniform; nothing is culled beyond the box test.
//   k_terrain_excl_emit       one workgroup per box.  Shared layout: copies the grid.  Unshared: per cell the keep flags of its two
//       triangles (OR over the words of the AND of the three corners' words), an exclusive scan of the kept count in row-major cell
//       order -- DPP inside the wave, the four waves' totals through LDS, a running carry over rounds of 256 cells --, then the kept
//       triangles' vertices.  No atomics; slots past n_vertices are not written.
// A call is cut into rounds of at most EXCL_LAUNCH_BOXES boxes and GEN_LAUNCH_WORK point-records, a box's records being the
// generator's and the vertices of its active sectors (RXR_TERRAIN_EXCL_LAUNCH_POINTS bounds a round's points instead); the rounds of
// a call share the scratch in stream order, calls are ordered by the lane (rxr_query.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "rxr_terrain_gen.h"

#define EXCL_LAUNCH_BOXES 64u     // boxes a round carries in its kernels' arguments (48 bytes each)
#define EXCL_EDGE_FLOATS 8u       // vi.x, vi.y, edge.x, edge.y | edge_length_sq, edge_length_sq > 0.0 (1.0 / 0.0), vj.y, 0

struct ExclRecords {
    const float4 *box;        // [S]: min.x, min.y, max.x, max.y
    const uint32_t *voff;     // [S + 1]
    const float4 *edge;       // [V][2]: the edge that ENDS at vertex i's predecessor (i, j = i - 1 cyclic)
    uint32_t S;
};
struct ExclBox {
    GenBox g;
    float raw[4];             // the chunk box as given: what the sectors' boxes are tested against
    uint32_t active;          // sectors active for this box (the host's count; the device ranks the same sectors)
    uint32_t np;              // grid points this box needs: steps_x * steps_y, 0 in the unshared layout without a cell
    uint32_t point0, mask0;   // where its heights and its mask words start in the round's scratch (words)
};
struct ExclClassifyArgs {
    GenRecords G;
    ExclRecords E;
    ExclBox box[EXCL_LAUNCH_BOXES];
    float cell_size;
    float *heights;
    uint32_t *masks;          // box b, word w, point j at mask0 + w * np + j
};
struct ExclEmitArgs {
    ExclBox box[EXCL_LAUNCH_BOXES];
    float cell_size;
    uint32_t stride;
    const float *heights;
    const uint32_t *masks;
    uint32_t *counts;         // [boxes of this round][4]
    float *vertices;          // [boxes of this round][stride][4]
};

using namespace rxgen;

namespace {

// point_in_sector (:891-950) over the edge records [e0, e1), at least three
__device__ __forceinline__ bool point_in_sector(const float4 *edge, uint32_t e0, uint32_t e1, float px, float py) {
    bool on_boundary = false, inside = false;
    for (uint32_t e = e0; e < e1; ++e) {
        const float4 a = edge[2u * e], b = edge[2u * e + 1u];
        if (b.y != 0.0f) {   // (wave-uniform) edge_length_sq > 0.0
            const float t = clamp01(fdiv((px - a.x) * a.z + (py - a.y) * a.w, b.x));
            const float qx = a.x + a.z * t, qy = a.y + a.w * t;
            const bool near = magnitude2(px - qx, py - qy) < 0.01f;   // (every lane, every edge: no lane leaves the loop early)
            on_boundary |= near;
        }
        const bool straddles = (a.y > py) != (b.z > py);
        const float cross_x = fdiv(a.z * (py - a.y), a.w) + a.x;
        if (straddles && px < cross_x) inside = !inside;
    }
    return on_boundary || inside;
}

}  // namespace

extern "C" __global__ __launch_bounds__(GEN_WG) void k_terrain_excl_classify(ExclClassifyArgs A) {
    const ExclBox b = A.box[blockIdx.y];
    const uint32_t words = (b.active + 31u) >> 5, z = blockIdx.z;
    if (z >= (words > 1u ? words : 1u) || blockIdx.x * GEN_WG >= b.np) return;   // (the whole workgroup)
    const uint32_t j = blockIdx.x * GEN_WG + threadIdx.x;
    const bool live = j < b.np;
    const uint32_t jj = live ? j : 0u;   // (a lane past the end repeats a point and stores nothing)
    const uint32_t iy = jj / (uint32_t)b.g.sx, ix = jj - iy * (uint32_t)b.g.sx;
    const float px[1] = {b.g.min_x + (float)(int32_t)ix * A.cell_size}, py[1] = {b.g.min_y + (float)(int32_t)iy * A.cell_size};
    float h[1] = {0.0f};
    if (z == 0u) gen_eval<1>(A.G, px, py, h);
    uint32_t bits = 0u;
    if (words) {
        uint32_t rank = 0u;   // active sectors before sector s
        for (uint32_t s = 0; s < A.E.S; ++s) {
            const float4 sb = A.E.box[s];
            if (!(sb.x <= b.raw[2] && sb.z >= b.raw[0] && sb.y <= b.raw[3] && sb.w >= b.raw[1])) continue;
            const uint32_t r = rank++;
            if ((r >> 5) < z) continue;
            if ((r >> 5) > z) break;   // (wave-uniform: the word is complete)
            const uint32_t e0 = A.E.voff[s], e1 = A.E.voff[s + 1u];
            if (e1 - e0 < 3u) continue;
            if (point_in_sector(A.E.edge, e0, e1, px[0], py[0])) bits |= 1u << (r & 31u);
        }
    }
    if (!live) return;
    if (z == 0u) A.heights[b.point0 + j] = h[0];
    if (words) A.masks[(size_t)b.mask0 + (size_t)z * b.np + j] = bits;
}

extern "C" __global__ __launch_bounds__(GEN_WG) void k_terrain_excl_emit(ExclEmitArgs A) {
    __shared__ uint32_t wave_total[GEN_WG / 64u];
    const ExclBox b = A.box[blockIdx.x];
    const uint32_t tid = threadIdx.x, sx = (uint32_t)b.g.sx, sy = (uint32_t)b.g.sy;
    float *vtx = A.vertices + (size_t)blockIdx.x * A.stride * 4;
    const float *hts = A.heights + b.point0;
    uint32_t *counts = A.counts + 4 * (size_t)blockIdx.x;
    auto put = [&](size_t slot, uint32_t i) {   // grid point i as vertex `slot`
        const uint32_t iy = i / sx, ix = i - iy * sx;
        float *o = vtx + 4 * slot;
        o[0] = b.g.min_x + (float)(int32_t)ix * A.cell_size, o[1] = hts[i], o[2] = b.g.min_y + (float)(int32_t)iy * A.cell_size, o[3] = 1.0f;
    };
    if (b.active == 0u) {   // the shared layout (np <= stride: checked on the host)
        for (uint32_t i = tid; i < b.np; i += GEN_WG) put(i, i);
        if (tid == 0u) counts[0] = sx, counts[1] = sy, counts[2] = 0u, counts[3] = b.np;
        return;
    }
    const uint32_t words = (b.active + 31u) >> 5;
    const uint32_t cw = sx - 1u, n_cells = b.np ? cw * (sy - 1u) : 0u;   // (6 * n_cells <= stride: checked on the host)
    const uint32_t *masks = A.masks + b.mask0;
    uint32_t carry = 0u;   // kept triangles of the rounds before; the same in every thread
    for (uint32_t c0 = 0; c0 < n_cells; c0 += GEN_WG) {
        const uint32_t cell = c0 + tid;
        const bool valid = cell < n_cells;
        const uint32_t cy = valid ? cell / cw : 0u, cx = valid ? cell - cy * cw : 0u;
        const uint32_t i0 = cy * sx + cx, i1 = i0 + 1u, i2 = i0 + sx, i3 = i2 + 1u;
        uint32_t drop0 = 0u, drop1 = 0u;
        for (uint32_t w = 0; w < words; ++w) {
            const uint32_t *m = masks + (size_t)w * b.np;
            const uint32_t m12 = m[i1] & m[i2];
            drop0 |= m[i0] & m12;
            drop1 |= m12 & m[i3];
        }
        const uint32_t keep0 = valid && !drop0, keep1 = valid && !drop1, v = keep0 + keep1;
        const uint32_t inclusive = rxm::wave_inclusive_add(v);
        if ((tid & 63u) == 63u) wave_total[tid >> 6] = inclusive;
        __syncthreads();
        uint32_t before = carry, round = 0u;
        for (uint32_t w = 0; w < GEN_WG / 64u; ++w) {
            const uint32_t t = wave_total[w];
            if (w < (tid >> 6)) before += t;
            round += t;
        }
        const size_t slot = 3 * (size_t)(before + inclusive - v);
        if (keep0) put(slot, i0), put(slot + 1, i2), put(slot + 2, i1);
        if (keep1) put(slot + 3 * keep0, i1), put(slot + 3 * keep0 + 1, i2), put(slot + 3 * keep0 + 2, i3);
        carry += round;
        __syncthreads();   // (the totals are rewritten by the next round)
    }
    if (tid == 0u) counts[0] = sx, counts[1] = sy, counts[2] = b.active, counts[3] = 3u * carry;
}

namespace {

int check_exclusions(const float *boxes, const uint32_t *off, const float *verts, uint32_t S, uint32_t V, std::string &err) {
    auto bad = [&](int code, const std::string &m) {
        err = m;
        return code;
    };
    if (S > RXR_TERRAIN_GEN_MAX_EXCLUDED_SECTORS) return bad(RXR_ERR_UNSUPPORTED, std::to_string(S) + " sectors exceed RXR_TERRAIN_GEN_MAX_EXCLUDED_SECTORS");
    if (V > RXR_TERRAIN_GEN_MAX_EXCLUSION_VERTICES) return bad(RXR_ERR_UNSUPPORTED, std::to_string(V) + " vertices exceed RXR_TERRAIN_GEN_MAX_EXCLUSION_VERTICES");
    if (S && !boxes) return bad(RXR_ERR_INVALID, "NULL sector_boxes");
    if (S && !off) return bad(RXR_ERR_INVALID, "NULL vertex_offsets");
    if (V && !verts) return bad(RXR_ERR_INVALID, "NULL vertices");
    if (!S && V) return bad(RXR_ERR_INVALID, "vertices without a sector");
    if (S) {
        if (off[0] != 0u) return bad(RXR_ERR_INVALID, "vertex_offsets[0] must be 0");
        for (uint32_t s = 0; s < S; ++s)
            if (off[s + 1] < off[s]) return bad(RXR_ERR_INVALID, "vertex_offsets[" + std::to_string(s + 1) + "] is below its predecessor");
        if (off[S] != V) return bad(RXR_ERR_INVALID, "vertex_offsets[n_sectors] = " + std::to_string(off[S]) + " is not n_vertices = " + std::to_string(V));
    }
    return RXR_OK;
}

ExclRecords excl_records_of(const rxr_ctx *ctx) {
    ExclRecords E{};
    const uint8_t *base = (const uint8_t *)ctx->d_excl.p;
    E.S = ctx->excl_S;
    if (!E.S) return E;   // (nothing is read)
    E.box = (const float4 *)(base + ctx->excl_off[0]);
    E.voff = (const uint32_t *)(base + ctx->excl_off[1]);
    E.edge = (const float4 *)(base + ctx->excl_off[2]);
    return E;
}

// the points a round takes at most: 2^30, or the environment's (the round's work is bounded next to it: meshes_run)
uint32_t launch_points() {
    if (const char *e = getenv("RXR_TERRAIN_EXCL_LAUNCH_POINTS")) {
        const unsigned long long v = strtoull(e, nullptr, 10);
        if (v) return (uint32_t)std::min<unsigned long long>(v, 1u << 30);
    }
    return 1u << 30;
}

// generate_grid's bounds, the active sectors and the layout of every box; refuses what the call cannot hold
// (work[i]: box i's points x records -- the generator's, the vertices of its ACTIVE sectors, and an eighth of a record per resident
// sector for the box scan)
int mesh_boxes(rxr_ctx *ctx, const char *who, const float *boxes, uint32_t n, uint32_t subdivisions, uint32_t stride, std::vector<ExclBox> &out,
               std::vector<uint64_t> &work, float &cell_size) {
    const std::string w = who;
    if (!ctx->gen_set) return rxr_fail(ctx, RXR_ERR_INVALID, w + ": no terrain generator is resident (rxr_set_terrain_generator)");
    if (!subdivisions) return rxr_fail(ctx, RXR_ERR_INVALID, w + ": subdivisions must be at least 1 (the reference divides by it)");
    if (n && !boxes) return rxr_fail(ctx, RXR_ERR_INVALID, w + ": NULL boxes");
    size_t total;
    if (__builtin_mul_overflow((size_t)n, (size_t)stride * 16u, &total)) return rxr_fail(ctx, RXR_ERR_INVALID, w + ": the vertex array's size overflows");
    cell_size = 1.0f / (float)subdivisions;
    out.resize(n);
    work.resize(n);
    const float *sb = ctx->excl_boxes.data();
    const uint64_t base_records = (uint64_t)ctx->gen_n[0] + ctx->gen_n[2] + ctx->gen_n[3] + ctx->excl_S / 8u;
    for (uint32_t i = 0; i < n; ++i) {
        const float *b = boxes + 4 * (size_t)i;
        ExclBox e{};
        e.g = grid_box(b, cell_size);
        memcpy(e.raw, b, sizeof e.raw);
        uint64_t active_vertices = 0;
        for (uint32_t s = 0; s < ctx->excl_S; ++s)   // BBox::intersects (src/map/bbox.rs:43-48), the sector's box first
            if (sb[4 * s] <= b[2] && sb[4 * s + 2] >= b[0] && sb[4 * s + 1] <= b[3] && sb[4 * s + 3] >= b[1]) {
                ++e.active;
                active_vertices += ctx->excl_voff[s + 1] - ctx->excl_voff[s];
            }
        const uint64_t points = (uint64_t)e.g.sx * (uint64_t)e.g.sy;
        const uint64_t cells = (e.g.sx > 1 && e.g.sy > 1) ? (uint64_t)(e.g.sx - 1) * (uint64_t)(e.g.sy - 1) : 0;
        const uint64_t layout = e.active ? 6 * cells : points;
        if (layout > stride)
            return rxr_fail(ctx, RXR_ERR_INVALID, w + ": box " + std::to_string(i) + " has a grid of " + std::to_string(e.g.sx) + " x " + std::to_string(e.g.sy) + " points and " +
                                                      std::to_string(e.active) + " active sectors: up to " + std::to_string(layout) + " vertices, more than the stride " + std::to_string(stride));
        e.np = (uint32_t)(e.active ? (cells ? points : 0) : points);   // (points <= 4 * cells where there is a cell: below the stride)
        if ((uint64_t)e.np * ((e.active + 31u) >> 5) >> 32)
            return rxr_fail(ctx, RXR_ERR_OOM, w + ": box " + std::to_string(i) + " needs 2^32 or more mask words of scratch");
        out[i] = e;
        work[i] = (uint64_t)e.np * std::max<uint64_t>(base_records + active_vertices, 1);
    }
    return RXR_OK;
}

// every box of a call into device arrays, queued on `s`
int meshes_run(rxr_ctx *ctx, std::vector<ExclBox> &boxes, const std::vector<uint64_t> &work, float cell_size, uint32_t stride, uint32_t *counts, float *vertices,
               hipStream_t s) {
    const uint32_t n = (uint32_t)boxes.size();
    const uint32_t bound = launch_points();
    // the rounds: up to EXCL_LAUNCH_BOXES boxes, up to `bound` points, up to GEN_LAUNCH_WORK point-records (rxr_terrain_gen.h: what a
    // launch of the height field takes) and fewer than 2^32 mask words (at least one box); every box's place in its round's scratch
    std::vector<uint32_t> round_boxes;
    size_t scratch_words = 0;
    for (uint32_t b0 = 0; b0 < n;) {
        uint32_t nb = 0;
        unsigned long long points = 0, mask_words = 0, records = 0;
        while (b0 + nb < n && nb < EXCL_LAUNCH_BOXES) {
            ExclBox &b = boxes[b0 + nb];
            const unsigned long long mw = (unsigned long long)b.np * ((b.active + 31u) >> 5);
            if (nb && (points + b.np > bound || records + work[b0 + nb] > GEN_LAUNCH_WORK || (mask_words + mw) >> 32)) break;
            records += work[b0 + nb];
            b.point0 = (uint32_t)points;
            b.mask0 = (uint32_t)mask_words;
            points += b.np;
            mask_words += mw;
            ++nb;
        }
        round_boxes.push_back(nb);
        scratch_words = std::max<size_t>(scratch_words, points + mask_words);
        b0 += nb;
    }
    int rc = rxr_query_begin(ctx, ctx->lane[Q_EXCL], s);
    if (rc != RXR_OK) return rc;
    if ((rc = rxr_ensure(ctx, ctx->d_excl_scratch, std::max<size_t>(scratch_words * 4, 256))) != RXR_OK) return rc;
    ctx->excl_launches = 0;
    ExclClassifyArgs C{};
    C.G = records_of(ctx);
    C.E = excl_records_of(ctx);
    C.cell_size = cell_size;
    ExclEmitArgs M{};
    M.cell_size = cell_size;
    M.stride = stride;
    uint32_t b0 = 0;
    for (const uint32_t nb : round_boxes) {
        uint32_t most = 0, most_words = 1;
        unsigned long long points = 0;
        for (uint32_t k = 0; k < nb; ++k) {
            const ExclBox &b = boxes[b0 + k];
            C.box[k] = M.box[k] = b;
            points += b.np;
            most = std::max(most, b.np);
            most_words = std::max(most_words, (b.active + 31u) >> 5);
        }
        C.heights = (float *)ctx->d_excl_scratch.p;
        C.masks = (uint32_t *)ctx->d_excl_scratch.p + points;   // (the round's heights, then its mask words)
        M.heights = C.heights;
        M.masks = C.masks;
        M.counts = counts + 4 * (size_t)b0;
        M.vertices = vertices + (size_t)b0 * stride * 4;
        if (most) {
            hipLaunchKernelGGL(k_terrain_excl_classify, dim3((most + GEN_WG - 1u) / GEN_WG, nb, most_words), dim3(GEN_WG), 0, s, C);
            HIPCHK(ctx, hipGetLastError());
        }
        // (a round of empty grids still writes their counts)
        hipLaunchKernelGGL(k_terrain_excl_emit, dim3(nb), dim3(GEN_WG), 0, s, M);
        HIPCHK(ctx, hipGetLastError());
        ++ctx->excl_launches;
        b0 += nb;
    }
    return rxr_query_end(ctx, ctx->lane[Q_EXCL], s);
}

}  // namespace

extern "C" {

int rxr_check_terrain_exclusions(const float *sector_boxes, const uint32_t *vertex_offsets, const float *vertices, uint32_t n_sectors, uint32_t n_vertices,
                                 char *message, uint32_t message_capacity) {
    std::string err;
    const int rc = check_exclusions(sector_boxes, vertex_offsets, vertices, n_sectors, n_vertices, err);
    rxr_copy_message(err, message, message_capacity);
    return rc;
}

int rxr_set_terrain_exclusions(rxr_ctx *ctx, const float *sector_boxes, const uint32_t *vertex_offsets, const float *vertices, uint32_t n_sectors, uint32_t n_vertices) {
    if (!ctx) return RXR_ERR_INVALID;
    if (ctx->group)
        return rxr_as_member0(ctx, [&](rxr_ctx *m) { return rxr_set_terrain_exclusions(m, sector_boxes, vertex_offsets, vertices, n_sectors, n_vertices); });
    const uint32_t S = n_sectors, V = n_vertices;
    std::string err;
    int rc = check_exclusions(sector_boxes, vertex_offsets, vertices, S, V, err);
    if (rc != RXR_OK) return rxr_fail(ctx, rc, "rxr_set_terrain_exclusions: " + err);
    // the device records, with what does not depend on the point computed here (the header comment: same operations, same bits)
    BlobCursor take;
    const size_t off[3] = {take((size_t)S * 16), take(((size_t)S + 1) * 4), take((size_t)V * EXCL_EDGE_FLOATS * 4)};
    std::vector<uint8_t> blob(take.o, 0);
    if (S) memcpy(blob.data() + off[0], sector_boxes, (size_t)S * 16);
    uint32_t *vo = (uint32_t *)(blob.data() + off[1]);
    for (uint32_t s = 0; s <= S; ++s) vo[s] = S ? vertex_offsets[s] : 0u;
    float *ed = (float *)(blob.data() + off[2]);
    for (uint32_t s = 0; s < S; ++s) {
        const uint32_t v0 = vertex_offsets[s], nv = vertex_offsets[s + 1] - v0;
        for (uint32_t i = 0; i < nv; ++i) {
            const float *vi = vertices + 2 * (size_t)(v0 + i), *vj = vertices + 2 * (size_t)(v0 + (i ? i - 1 : nv - 1));
            float *o = ed + EXCL_EDGE_FLOATS * (size_t)(v0 + i);
            const float ex = vj[0] - vi[0], ey = vj[1] - vi[1];
            const float len_sq = ex * ex + ey * ey;
            o[0] = vi[0], o[1] = vi[1], o[2] = ex, o[3] = ey, o[4] = len_sq, o[5] = len_sq > 0.0f ? 1.0f : 0.0f, o[6] = vj[1];
        }
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if ((rc = rxr_quiesce(ctx)) != RXR_OK) return rc;   // queued mesh calls read what is replaced here
    if ((rc = rxr_ensure(ctx, ctx->d_excl, std::max<size_t>(blob.size(), 256))) != RXR_OK) return rc;
    ctx->excl_S = ctx->excl_V = 0;   // (until the records below have arrived)
    ctx->excl_boxes.clear();
    ctx->excl_voff.assign(1, 0u);
    HIPCHK(ctx, hipMemcpyAsync(ctx->d_excl.p, blob.data(), blob.size(), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // (the blob is read until here)
    for (int i = 0; i < 3; ++i) ctx->excl_off[i] = off[i];
    if (S) ctx->excl_boxes.assign(sector_boxes, sector_boxes + 4 * (size_t)S);
    if (S) ctx->excl_voff.assign(vertex_offsets, vertex_offsets + S + 1);
    ctx->excl_S = S, ctx->excl_V = V;
    return RXR_OK;
}

int rxr_generated_meshes(rxr_ctx *ctx, const float *boxes, uint32_t n, uint32_t subdivisions, uint32_t stride, uint32_t *counts, float *vertices) {
    if (!ctx) return RXR_ERR_INVALID;
    if (ctx->group) return rxr_as_member0(ctx, [&](rxr_ctx *m) { return rxr_generated_meshes(m, boxes, n, subdivisions, stride, counts, vertices); });
    std::vector<ExclBox> eb;
    std::vector<uint64_t> work;
    float cell_size;
    int rc = mesh_boxes(ctx, "rxr_generated_meshes", boxes, n, subdivisions, stride, eb, work, cell_size);
    if (rc != RXR_OK) return rc;
    if (!n) return RXR_OK;
    if (!counts || (!vertices && stride)) return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_generated_meshes: NULL output array");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // the vertices go up as well as down: the slots past a box's count come back as the caller left them
    QueryIO io{ctx, ctx->lane[Q_EXCL]};
    const unsigned i_c = io.out(counts, (size_t)n * 16), i_v = io.inout(stride ? vertices : nullptr, (size_t)n * stride * 16);
    if ((rc = io.upload()) != RXR_OK) return rc;
    if ((rc = meshes_run(ctx, eb, work, cell_size, stride, io.dev<uint32_t>(i_c), io.dev<float>(i_v), ctx->stream)) != RXR_OK) return rc;
    return io.download();
}

int rxr_generated_meshes_to(rxr_ctx *ctx, const float *boxes, uint32_t n, uint32_t subdivisions, uint32_t stride, uint32_t *dev_counts, float *dev_vertices,
                            void *hip_stream) {
    if (!ctx) return RXR_ERR_INVALID;
    if (ctx->group) return rxr_fail(ctx, RXR_ERR_UNSUPPORTED, "rxr_generated_meshes_to on a multi-device context: device pointers and streams belong to ONE device (use rxr_member)");
    std::vector<ExclBox> eb;
    std::vector<uint64_t> work;
    float cell_size;
    int rc = mesh_boxes(ctx, "rxr_generated_meshes_to", boxes, n, subdivisions, stride, eb, work, cell_size);
    if (rc != RXR_OK) return rc;
    if (!n) return RXR_OK;
    if (!dev_counts || (!dev_vertices && stride)) return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_generated_meshes_to: NULL output array");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const void *const p[2] = {dev_counts, stride ? dev_vertices : nullptr};
    const size_t bytes[2] = {(size_t)n * 16, (size_t)n * stride * 16};
    const char *const names[2] = {"dev_counts", "dev_vertices"};
    if ((rc = device_arrays(ctx, "rxr_generated_meshes_to", p, bytes, names, 2)) != RXR_OK) return rc;
    return meshes_run(ctx, eb, work, cell_size, stride, dev_counts, dev_vertices, hip_stream ? (hipStream_t)hip_stream : ctx->stream);
}

// test-only: the rounds (one classification and one emission launch each) of the last mesh call
uint32_t rxr_debug_terrain_excl_launches(rxr_ctx *ctx) {
    if (!ctx) return 0;
    if (ctx->group) return rxr_debug_terrain_excl_launches(rxr_member(ctx, 0));
    return ctx->excl_launches;
}

}  // extern "C"
