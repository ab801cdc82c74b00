// rxr_terrain_flatten.hip -- processed_heights on the device: the Height pass of TerrainChunk::process_batch_modifiers
// (src/terrain/chunk.rs:144-208) over ShapeFX::sector_modify_heightmap (src/shapestack/shapefx.rs:414-478) and linedef_modify_heightmap
// (:682-820).  include/rxr.h: rxr_check_terrain_flatten, rxr_set_terrain_flatten, rxr_flatten_terrain, rxr_flatten_terrain_to,
// rxr_set_terrain_height_source; DESIGN.md section 25.
//
// Semantics: the header states them.  All f32, one operation per reference operation in its order, nothing fused (the build's
// -ffp-contract=off); divisions and square roots through rxr_exact_math.h.  The reference loops over an op's integer range and inserts
// into a dictionary; no op reads another's result, so a cell's value is a function of the cell alone -- the last op in list order whose
// loop reaches the cell and whose tests pass -- and this file computes it per cell (tests/test_terrain_flatten_cpu.py holds the
// per-cell form to the loop form).
//
// One workgroup of 256 threads per chunk, so everything per op is wave-uniform: op, edge and segment records are read through uniform
// addresses (scalar loads), the chunk's lists through LDS.
//   1. the chunk's ORDERED list of active ops: 256 candidates a round, four ballots and prefix counts, the waves' totals through LDS.
//      A sector op is active iff its box.expanded(2.0) intersects the chunk's bounds; a linedef op is listed always and
//   2. gets its active segments the same way (box.expanded(2.0) against the bounds), in list order, as indices into its range
//   3. one thread per cell walks the list (FLATTEN_WALK_BACKWARD: from the end, leaving at the first op that writes -- the same value,
//      because the last writer wins; profiles/terrain_flatten/README.md has both forms' times) and writes the caller's arrays and the
//      processed grid
// A call is cut into launches of at most FLATTEN_LAUNCH_CHUNKS chunks, whose coordinates travel as kernel arguments.  The processed
// grid is the one thing written here that other queries read: rxr_flatten_run waits for the picks' and the mesh builds' lanes, and
// they wait for this one when they read the processed grid (rxr_terrain_hit.hip, rxr_terrain_mesh.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "rxr_debug.h"
#include "rxr_query.h"
#include "rxr_exact_math.h"
#include "rxr_terrain_flatten_records.h"

#ifndef FLATTEN_WALK_BACKWARD
#define FLATTEN_WALK_BACKWARD 0
#endif
#define FLATTEN_WG 256u
#define FLATTEN_LAUNCH_CHUNKS 256u   // chunk coordinates per launch (2 KiB of kernel arguments)

struct FlattenArgs {
    const float *heights;    // the REGISTERED grid [gh][gw], row-major
    const uint8_t *mask;     // ... and its presence
    float *pheights;         // the PROCESSED grid, same rectangle
    uint8_t *pmask;
    int32_t x0, y0;
    uint32_t gw, gh;
    float sx, sy;
    uint32_t cs;             // chunk_size, 1 .. RXR_TERRAIN_MESH_MAX_CHUNK_SIZE
    const float4 *ops;       // [n_ops][FLATTEN_OP_WORDS]
    const float4 *records;   // [slots][FLATTEN_RECORD_WORDS]
    uint32_t n_ops;
    uint32_t seg_slots;      // the linedef ops' range lengths, summed: the segment list's room in LDS
    float *out_heights;      // [n][cs * cs] from this launch's first chunk on, or NULL; so out_present
    uint8_t *out_present;
    int32_t coords[FLATTEN_LAUNCH_CHUNKS][2];
};

namespace {

// LDS of a workgroup: act[n_ops], seg_at[n_ops], seg_n[n_ops] words, 4 words of wave totals, seg[seg_slots] halfwords
__host__ __device__ inline uint32_t flatten_lds_bytes(uint32_t n_ops, uint32_t seg_slots) { return n_ops * 12u + 16u + (seg_slots * 2u + 3u) / 4u * 4u; }

__device__ __forceinline__ float fdiv(float n, float d) { return rxm::div1_known(n, d, rxm::in_window(n) && rxm::in_window(d)); }
// Rust's f32::clamp(0.0, 1.0): a NaN stays, -0.0 stays
__device__ __forceinline__ float clamp01(float t) { return t < 0.0f ? 0.0f : (t > 1.0f ? 1.0f : t); }
__device__ __forceinline__ float magnitude2(float x, float y) { return rxm::sqrt_exact(x * x + y * y); }
// ShapeFX::smoothstep (:2258-2261)
__device__ __forceinline__ float smoothstep(float edge0, float edge1, float x) {
    const float t = clamp01(fdiv(x - edge0, edge1 - edge0));
    return t * t * (3.0f - 2.0f * t);
}
// Rust's `x as i32`: saturating, NaN -> 0
__device__ __forceinline__ int32_t as_i32(float x) {
    if (x != x) return 0;
    if (x >= 2147483648.0f) return INT32_MAX;
    if (x <= -2147483648.0f) return INT32_MIN;
    return (int32_t)x;
}
__device__ __forceinline__ uint32_t uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
// 16 bytes of a record table at a wave-uniform index, through the constant address space: a scalar load (s_load_dwordx4) into scalar
// registers.  A plain global load behind the kernel's stores is issued as a vector load.  The tables are written by
// rxr_set_terrain_flatten and never by a kernel.
__device__ __forceinline__ float4 uniform_word(const float4 *table, uint32_t i) {
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    typedef const u32x4 __attribute__((address_space(4))) *vec_ptr;
    const u32x4 v = *(vec_ptr)(table + i);
    return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
}
// BBox::intersects (src/map/bbox.rs:43-48), the chunk's bounds first
__device__ __forceinline__ bool intersects(float bx0, float by0, float bx1, float by1, float4 o) { return bx0 <= o.z && bx1 >= o.x && by0 <= o.w && by1 >= o.y; }

// One round of an order-preserving compaction over the workgroup: thread `tid` offers a candidate (`take`); returns the round's
// total, and in `slot` this thread's place among the round's taken ones.  Two barriers: every thread of the workgroup calls it.
__device__ __forceinline__ uint32_t compact_round(bool take, uint32_t *wave_total, uint32_t tid, uint32_t &slot) {
    const unsigned long long votes = __builtin_amdgcn_ballot_w64(take);
    const uint32_t before = __builtin_amdgcn_mbcnt_hi((uint32_t)(votes >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)votes, 0u));
    if ((tid & 63u) == 0u) wave_total[tid >> 6] = (uint32_t)__builtin_popcountll(votes);
    __syncthreads();
    uint32_t earlier = 0, total = 0;
    for (uint32_t w = 0; w < FLATTEN_WG / 64u; ++w) {
        const uint32_t t = wave_total[w];
        if (w < (tid >> 6)) earlier += t;
        total += t;
    }
    __syncthreads();   // (the totals are rewritten by the next round)
    slot = earlier + before;
    return total;
}

}  // namespace

extern "C" __global__ __launch_bounds__(FLATTEN_WG) void k_terrain_flatten(FlattenArgs A) {
    extern __shared__ uint32_t lds[];
    const uint32_t cs = A.cs, n_cells = cs * cs, tid = threadIdx.x, chunk = blockIdx.x;
    uint32_t *act = lds, *seg_at = lds + A.n_ops, *seg_n = lds + 2u * A.n_ops, *wave_total = lds + 3u * A.n_ops;
    uint16_t *seg = (uint16_t *)(wave_total + 4);
    // (the host checked that every cell of the chunk lies within +-2^30)
    const int32_t wx0 = A.coords[chunk][0] * (int32_t)cs, wy0 = A.coords[chunk][1] * (int32_t)cs;
    // TerrainChunk::bounds (:130-134): from_pos_size(origin as f32, size as f32 - 1.0)
    const float size_f = (float)(int32_t)cs - 1.0f;
    const float bx0 = (float)wx0, by0 = (float)wy0, bx1 = bx0 + size_f, by1 = by0 + size_f;

    // 1. the active ops, in list order
    uint32_t n_act = 0;   // the same in every thread
    for (uint32_t i0 = 0; i0 < A.n_ops; i0 += FLATTEN_WG) {
        const uint32_t i = i0 + tid;
        bool take = false;
        if (i < A.n_ops) {
            const uint32_t kind = __float_as_uint(A.ops[FLATTEN_OP_WORDS * i + 3u].z);
            take = kind == RXR_TERRAIN_FLATTEN_LINEDEFS || intersects(bx0, by0, bx1, by1, A.ops[FLATTEN_OP_WORDS * i + 1u]);
        }
        uint32_t slot;
        const uint32_t total = compact_round(take, wave_total, tid, slot);
        if (take) act[n_act + slot] = i;
        n_act += total;
    }
    __syncthreads();
    // 2. the linedef ops' active segments, in list order
    uint32_t seg_used = 0;
    for (uint32_t k = 0; k < n_act; ++k) {
        const uint32_t op = uniform(act[k]);
        const float4 d = uniform_word(A.ops, FLATTEN_OP_WORDS * op + 3u);
        if (__float_as_uint(d.z) != RXR_TERRAIN_FLATTEN_LINEDEFS) continue;
        const uint32_t first = __float_as_uint(d.x), count = __float_as_uint(d.y);
        uint32_t n_seg = 0;
        for (uint32_t r0 = 0; r0 < count; r0 += FLATTEN_WG) {
            const uint32_t r = r0 + tid;
            const bool take = r < count && intersects(bx0, by0, bx1, by1, A.records[FLATTEN_RECORD_WORDS * (first + r) + 2u]);
            uint32_t slot;
            const uint32_t total = compact_round(take, wave_total, tid, slot);
            if (take) seg[seg_used + n_seg + slot] = (uint16_t)r;   // (r < RXR_TERRAIN_FLATTEN_MAX_SEGMENTS = 2^14)
            n_seg += total;
        }
        if (tid == 0) seg_at[k] = seg_used, seg_n[k] = n_seg;
        seg_used += n_seg;
    }
    __syncthreads();

    // 3. a thread per cell
    for (uint32_t cell = tid; cell < n_cells; cell += FLATTEN_WG) {
        const int32_t x = wx0 + (int32_t)(cell % cs), y = wy0 + (int32_t)(cell / cs);
        const uint32_t gx = (uint32_t)x - (uint32_t)A.x0, gy = (uint32_t)y - (uint32_t)A.y0;
        const bool in_grid = gx < A.gw && gy < A.gh;
        const size_t at = (size_t)gy * A.gw + gx;
        const bool was = in_grid && A.mask[at] != 0;          // get_height_unprocessed is Some
        const float unprocessed = was ? A.heights[at] : 0.0f;
        const float px = (float)x, py = (float)y;
        const bool in_chunk_box = px >= bx0 && px <= bx1 && py >= by0 && py <= by1;   // chunk_bbox.contains
        bool written = false;
        float value = unprocessed;
#if FLATTEN_WALK_BACKWARD
        for (uint32_t k = n_act; k-- > 0u && !written;) {
#else
        for (uint32_t k = 0; k < n_act; ++k) {
#endif
            const uint32_t op = uniform(act[k]);
            const float4 a = uniform_word(A.ops, FLATTEN_OP_WORDS * op), d = uniform_word(A.ops, FLATTEN_OP_WORDS * op + 3u);
            const float bevel = a.x;
            const uint32_t first = __float_as_uint(d.x), count = __float_as_uint(d.y);
            if (__float_as_uint(d.z) == RXR_TERRAIN_FLATTEN_SECTOR) {
                const float4 rg = uniform_word(A.ops, FLATTEN_OP_WORDS * op + 2u);
                const int32_t min_x = (int32_t)__float_as_uint(rg.x), max_x = (int32_t)__float_as_uint(rg.y), min_y = (int32_t)__float_as_uint(rg.z), max_y = (int32_t)__float_as_uint(rg.w);
                // expanded_bbox = *bbox after expand(bevel): each side moves by bevel * 0.5
                const float ex0 = bx0 - a.w, ey0 = by0 - a.w, ex1 = bx1 + a.w, ey1 = by1 + a.w;
                const bool reached = x >= min_x && x <= max_x && y >= min_y && y <= max_y && px >= ex0 && px <= ex1 && py >= ey0 && py <= ey1;
                if (!(reached && in_chunk_box)) continue;
                // Sector::signed_distance (src/map/sector.rs:308-333)
                float min_dist = 3.40282347e+38f;
                bool inside = false;
                for (uint32_t e = 0; e < count; ++e) {
                    const float4 r0 = uniform_word(A.records, FLATTEN_RECORD_WORDS * (first + e)), r1 = uniform_word(A.records, FLATTEN_RECORD_WORDS * (first + e) + 1u);
                    const float tx = px - r0.x, ty = py - r0.y;
                    const float t = clamp01(fdiv(tx * r0.z + ty * r0.w, r1.x));
                    const float qx = r0.x + r0.z * t, qy = r0.y + r0.w * t;
                    min_dist = fminf(min_dist, magnitude2(px - qx, py - qy));   // (f32::min drops a NaN, as fminf does)
                    // is_inside (:272-305): polygon[i] = (r0.x, r0.y), polygon[j].y = r1.w, polygon[j] - polygon[i] = (r1.y, r1.z)
                    if (count >= 3u && (r0.y > py) != (r1.w > py) && px < fdiv(r1.y * (py - r0.y), r1.z) + r0.x) inside = !inside;
                }
                const float sd = inside ? -min_dist : min_dist;
                if (sd < a.z) {
                    const float s = smoothstep(0.0f, bevel, bevel - sd);
                    const float original = was ? unprocessed : a.y;
                    value = original * (1.0f - s) + a.y * s;
                    written = true;
                }
            } else {
                const uint32_t s0 = uniform(seg_at[k]), ns = uniform(seg_n[k]);
                if (!ns) continue;   // closest_segment is None
                // tile_min .. tile_max (:782-785), wave-uniform
                const float bsx = bevel * A.sx, bsy = bevel * A.sy;
                const int32_t tx0 = as_i32(floorf(fdiv(bx0 - bsx, A.sx))), ty0 = as_i32(floorf(fdiv(by0 - bsy, A.sy)));
                const int32_t tx1 = as_i32(ceilf(fdiv(bx1 + bsx, A.sx))), ty1 = as_i32(ceilf(fdiv(by1 + bsy, A.sy)));
                if (!(x >= tx0 && x < tx1 && y >= ty0 && y < ty1 && in_chunk_box)) continue;
                const float cx = (px + 0.5f) * A.sx, cy = (py + 0.5f) * A.sy;   // tile_center
                float best = 0.0f, best_t = 0.0f, h0 = 0.0f, h1 = 0.0f;
                for (uint32_t j = 0; j < ns; ++j) {
                    const uint32_t r = first + uniform((uint32_t)seg[s0 + j]);
                    const float4 r0 = uniform_word(A.records, FLATTEN_RECORD_WORDS * r), r1 = uniform_word(A.records, FLATTEN_RECORD_WORDS * r + 1u);
                    // point_to_line_segment (:711-719)
                    const float ax = cx - r0.x, ay = cy - r0.y;
                    const float t = clamp01(fdiv(ax * r0.z + ay * r0.w, r1.x));
                    const float qx = r0.x + r0.z * t, qy = r0.y + r0.w * t;
                    const float dist = magnitude2(cx - qx, cy - qy);
                    if (j == 0u || dist < best) best = dist, best_t = t, h0 = r1.y, h1 = r1.z;
                }
                if (best > bevel) continue;   // (a NaN distance goes on, as in the reference)
                const float height = h0 * (1.0f - best_t) + h1 * best_t;
                const float blend = smoothstep(0.0f, bevel, bevel - best);
                const float original = was ? unprocessed : height;
                value = original * (1.0f - blend) + height * blend;
                written = true;
            }
        }
        const bool present = was || written;
        if (in_grid) {
            A.pheights[at] = value;
            A.pmask[at] = present ? 1 : 0;
        }
        const size_t o = (size_t)chunk * n_cells + cell;
        if (A.out_heights) A.out_heights[o] = value;
        if (A.out_present) A.out_present[o] = present ? 1 : 0;
    }
}

namespace {

// what both entry points refuse, but for their pointers
int flatten_check(rxr_ctx *ctx, const char *who, const int32_t *coords, uint32_t n, int32_t cs) {
    const std::string w = who;
    if (!ctx->heights_set) return rxr_fail(ctx, RXR_ERR_INVALID, w + ": no terrain heights are resident (rxr_set_terrain_heights)");
    if (cs < 1) return rxr_fail(ctx, RXR_ERR_INVALID, w + ": chunk_size must be at least 1");
    if (cs > RXR_TERRAIN_MESH_MAX_CHUNK_SIZE)
        return rxr_fail(ctx, RXR_ERR_UNSUPPORTED, w + ": chunk_size " + std::to_string(cs) + " exceeds RXR_TERRAIN_MESH_MAX_CHUNK_SIZE");
    if (n && !coords) return rxr_fail(ctx, RXR_ERR_INVALID, w + ": NULL chunk_coords");
    auto name = [&](uint32_t i) { return "chunk " + std::to_string(i) + " (" + std::to_string(coords[2 * (size_t)i]) + ", " + std::to_string(coords[2 * (size_t)i + 1]) + ")"; };
    for (uint32_t i = 0; i < n; ++i)
        for (int a = 0; a < 2; ++a) {
            const int64_t lo = (int64_t)coords[2 * (size_t)i + a] * cs;
            if (lo < -(1ll << 30) || lo + cs - 1 > (1ll << 30)) return rxr_fail(ctx, RXR_ERR_INVALID, w + ": " + name(i) + ": its cells leave +-2^30");
        }
    // two workgroups would write the same cells of the processed grid
    std::vector<uint32_t> order(n);
    for (uint32_t i = 0; i < n; ++i) order[i] = i;
    auto key = [&](uint32_t i) { return ((uint64_t)(uint32_t)coords[2 * (size_t)i] << 32) | (uint32_t)coords[2 * (size_t)i + 1]; };
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return key(a) < key(b); });
    for (uint32_t i = 1; i < n; ++i)
        if (key(order[i]) == key(order[i - 1])) return rxr_fail(ctx, RXR_ERR_INVALID, w + ": " + name(std::max(order[i], order[i - 1])) + " is named twice");
    return RXR_OK;
}

// every chunk of a call into device arrays (either may be null), queued on `s`
int flatten_run(rxr_ctx *ctx, const int32_t *coords, uint32_t n, int32_t cs, float *heights, uint8_t *present, hipStream_t s) {
    uint32_t bound = FLATTEN_LAUNCH_CHUNKS;
    if (const char *e = getenv("RXR_TERRAIN_FLATTEN_LAUNCH_CHUNKS")) {
        const unsigned long long v = strtoull(e, nullptr, 10);
        if (v) bound = (uint32_t)std::min<unsigned long long>(v, FLATTEN_LAUNCH_CHUNKS);
    }
    FlattenArgs A{};
    A.heights = (const float *)ctx->d_heights.p;
    A.mask = (const uint8_t *)ctx->d_heights_mask.p;
    A.pheights = (float *)ctx->d_pheights.p;
    A.pmask = (uint8_t *)ctx->d_pheights_mask.p;
    A.x0 = ctx->heights_x0;
    A.y0 = ctx->heights_y0;
    A.gw = ctx->heights_gw;
    A.gh = ctx->heights_gh;
    A.sx = ctx->heights_scale[0];
    A.sy = ctx->heights_scale[1];
    A.cs = (uint32_t)cs;
    A.ops = (const float4 *)((const uint8_t *)ctx->d_flatten.p + ctx->flatten_off[0]);
    A.records = (const float4 *)((const uint8_t *)ctx->d_flatten.p + ctx->flatten_off[1]);
    A.n_ops = ctx->flatten_ops;
    A.seg_slots = ctx->flatten_seg_slots;
    // behind this lane's last call, and behind the queued picks and mesh builds, which may read the processed grid
    int rc = rxr_query_begin(ctx, ctx->lane[Q_FLATTEN], s);
    if (rc != RXR_OK || (rc = rxr_query_begin(ctx, ctx->lane[Q_HEIGHTS], s)) != RXR_OK || (rc = rxr_query_begin(ctx, ctx->lane[Q_MESH], s)) != RXR_OK) return rc;
    ctx->flatten_launches = 0;
    const size_t per = (size_t)cs * (size_t)cs;
    for (uint32_t c0 = 0; c0 < n; c0 += bound) {
        const uint32_t nc = std::min(n - c0, bound);
        memcpy(A.coords, coords + 2 * (size_t)c0, (size_t)nc * 2 * sizeof(int32_t));
        A.out_heights = heights ? heights + (size_t)c0 * per : nullptr;
        A.out_present = present ? present + (size_t)c0 * per : nullptr;
        hipLaunchKernelGGL(k_terrain_flatten, dim3(nc), dim3(FLATTEN_WG), flatten_lds_bytes(A.n_ops, A.seg_slots), s, A);
        HIPCHK(ctx, hipGetLastError());
        ++ctx->flatten_launches;
    }
    return rxr_query_end(ctx, ctx->lane[Q_FLATTEN], s);
}

}  // namespace

extern "C" {

int rxr_check_terrain_flatten(const uint32_t *op_kinds, const float *op_params, const uint32_t *op_ranges, uint32_t n_ops, const float *records,
                              uint32_t n_records, char *message, uint32_t message_capacity) {
    std::string err;
    const int rc = rxflat::check(op_kinds, op_params, op_ranges, n_ops, records, n_records, nullptr, nullptr, err);
    rxr_copy_message(err, message, message_capacity);
    return rc;
}

int rxr_set_terrain_flatten(rxr_ctx *ctx, const uint32_t *op_kinds, const float *op_params, const uint32_t *op_ranges, uint32_t n_ops, const float *records,
                            uint32_t n_records) {
    if (!ctx) return RXR_ERR_INVALID;
    if (ctx->group) return rxr_as_member0(ctx, [&](rxr_ctx *m) { return rxr_set_terrain_flatten(m, op_kinds, op_params, op_ranges, n_ops, records, n_records); });
    std::string err;
    uint32_t slots = 0, seg_slots = 0;
    int rc = rxflat::check(op_kinds, op_params, op_ranges, n_ops, records, n_records, &slots, &seg_slots, err);
    if (rc != RXR_OK) return rxr_fail(ctx, rc, "rxr_set_terrain_flatten: " + err);
    size_t records_at = 0;
    const std::vector<float> blob = rxflat::build(op_kinds, op_params, op_ranges, n_ops, records, slots, &records_at);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if ((rc = rxr_quiesce(ctx)) != RXR_OK) return rc;   // queued flattens read what is replaced here
    if ((rc = rxr_ensure(ctx, ctx->d_flatten, std::max<size_t>(blob.size() * sizeof(float), 256))) != RXR_OK) return rc;
    ctx->flatten_ops = ctx->flatten_seg_slots = 0;   // (until the records below have arrived)
    if (!blob.empty()) HIPCHK(ctx, hipMemcpyAsync(ctx->d_flatten.p, blob.data(), blob.size() * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // (the blob is read until here)
    ctx->flatten_off[0] = 0, ctx->flatten_off[1] = records_at;
    ctx->flatten_ops = n_ops, ctx->flatten_seg_slots = seg_slots;
    return RXR_OK;
}

int rxr_flatten_terrain(rxr_ctx *ctx, const int32_t *chunk_coords, uint32_t n, int32_t chunk_size, float *heights, uint8_t *present) {
    if (!ctx) return RXR_ERR_INVALID;
    if (ctx->group) return rxr_as_member0(ctx, [&](rxr_ctx *m) { return rxr_flatten_terrain(m, chunk_coords, n, chunk_size, heights, present); });
    int rc = flatten_check(ctx, "rxr_flatten_terrain", chunk_coords, n, chunk_size);
    if (rc != RXR_OK) return rc;
    if (!n) return RXR_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t cells = (size_t)n * (size_t)chunk_size * (size_t)chunk_size;   // (at most 2^32 * 2^12)
    QueryIO io{ctx, ctx->lane[Q_FLATTEN]};
    const unsigned i_h = io.out(heights, cells * sizeof(float)), i_p = io.out(present, cells);
    if ((rc = io.upload()) != RXR_OK) return rc;
    if ((rc = flatten_run(ctx, chunk_coords, n, chunk_size, io.dev<float>(i_h), io.dev<uint8_t>(i_p), ctx->stream)) != RXR_OK) return rc;
    return io.download();
}

int rxr_flatten_terrain_to(rxr_ctx *ctx, const int32_t *chunk_coords, uint32_t n, int32_t chunk_size, float *dev_heights, uint8_t *dev_present, void *hip_stream) {
    if (!ctx) return RXR_ERR_INVALID;
    if (ctx->group) return rxr_fail(ctx, RXR_ERR_UNSUPPORTED, "rxr_flatten_terrain_to on a multi-device context: device pointers and streams belong to ONE device (use rxr_member)");
    const int rc = flatten_check(ctx, "rxr_flatten_terrain_to", chunk_coords, n, chunk_size);
    if (rc != RXR_OK) return rc;
    if (!n) return RXR_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t cells = (size_t)n * (size_t)chunk_size * (size_t)chunk_size;
    if (dev_heights && ((uintptr_t)dev_heights & 3u)) return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_flatten_terrain_to: dev_heights must be 4-byte aligned device memory");
    if (dev_heights && !rxr_on_device(ctx, dev_heights, cells * sizeof(float)))
        return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_flatten_terrain_to: dev_heights is not device memory of the context's device (or is too small)");
    if (dev_present && !rxr_on_device(ctx, dev_present, cells))
        return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_flatten_terrain_to: dev_present is not device memory of the context's device (or is too small)");
    return flatten_run(ctx, chunk_coords, n, chunk_size, dev_heights, dev_present, hip_stream ? (hipStream_t)hip_stream : ctx->stream);
}

int rxr_set_terrain_height_source(rxr_ctx *ctx, uint32_t source) {
    if (!ctx) return RXR_ERR_INVALID;
    if (ctx->group) return rxr_as_member0(ctx, [&](rxr_ctx *m) { return rxr_set_terrain_height_source(m, source); });
    if (source != RXR_TERRAIN_HEIGHTS_REGISTERED && source != RXR_TERRAIN_HEIGHTS_PROCESSED)
        return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_set_terrain_height_source: " + std::to_string(source) + " is neither RXR_TERRAIN_HEIGHTS_REGISTERED nor RXR_TERRAIN_HEIGHTS_PROCESSED");
    ctx->height_source = source;
    return RXR_OK;
}

// test-only: the k_terrain_flatten launches of the last flatten call
uint32_t rxr_debug_terrain_flatten_launches(rxr_ctx *ctx) {
    if (!ctx) return 0;
    if (ctx->group) return rxr_debug_terrain_flatten_launches(rxr_member(ctx, 0));
    return ctx->flatten_launches;
}

}  // extern "C"
