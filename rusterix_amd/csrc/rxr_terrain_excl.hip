// rxr_terrain_excl.hip -- the generated terrain's chunk meshes with their excluded sectors cut out: TerrainGenerator::apply_exclusions
// (src/chunkbuilder/terrain_generator.rs:747-825) over collect_excluded_sectors' box test (:438-457, src/map/bbox.rs:43-48) and
// point_in_sector (:891-950), behind generate_grid and interpolate_heights (rxr_terrain_gen.h).  include/rxr.h:
// rxr_check_terrain_exclusions, rxr_set_terrain_exclusions, rxr_generated_meshes(_to).
// Behind them, in the same rounds and on the same scratch: partition_by_tiles (:954-1034), k_terrain_tiles_emit, rxr_check_terrain_tiles,
// rxr_set_terrain_tiles, rxr_generated_tile_meshes(_to); its comment stands in front of that kernel.
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

#include "rxr_debug.h"
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
#define TILE_BITMAP_WORDS (RXR_TERRAIN_TILES_MAX_TILES / 32u)
#define TILE_RECORD_WORDS 4u      // per triangle in the call scratch: tile slot, vertex base, position in its group, first-use corners
struct TileTable {
    const uint64_t *keys;     // [n] ascending: tile_key of the override cells
    const uint32_t *slots;    // [n]
    uint32_t n;
};
struct TileEmitArgs {
    ExclBox box[EXCL_LAUNCH_BOXES];
    uint32_t tri0[EXCL_LAUNCH_BOXES];   // where a box's triangle records start in `tris` (words)
    TileTable T;
    float cell_size;
    uint32_t max_groups, vstride, tstride;
    const float *heights;
    const uint32_t *masks;
    uint32_t *tris;
    uint32_t *box_counts;     // [boxes of this round][4]
    uint32_t *counts;         // [boxes of this round][max_groups][2]
    uint32_t *group_tiles;    // [boxes of this round][max_groups]
    float *vertices, *uvs;    // [boxes of this round][max_groups][vstride][4], ..[2]
    uint32_t *indices;        // [boxes of this round][max_groups][tstride][3]
};
// a tile cell as one sortable word: x, then z, each with its sign bit flipped
__host__ __device__ inline uint64_t tile_key(int32_t x, int32_t z) { return (uint64_t)((uint32_t)x ^ 0x80000000u) << 32 | ((uint32_t)z ^ 0x80000000u); }

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

// ---- partition_by_tiles (:954-1034): the same boxes as per-tile meshes with uvs and indices (the header comment of the section
// "generated terrain tile meshes" in include/rxr.h) ----
namespace {

// `x.floor() as i32`: saturating, a NaN is 0
__device__ __forceinline__ int32_t floor_as_i32(float x) {
    const float f = floorf(x);
    if (!(f == f)) return 0;
    if (f <= -2147483648.0f) return INT32_MIN;
    if (f >= 2147483648.0f) return INT32_MAX;
    return (int32_t)f;
}

// the tile slot of the triangle whose corners have the uvs (u0, v0), (u1, v1), (u2, v2), in that order: the centre added left to
// right, then divided by 3.0 (a division, correctly rounded), floored, looked up among the overrides; slot 0 without one
__device__ __forceinline__ uint32_t tile_slot(const TileTable &T, float u0, float u1, float u2, float v0, float v1, float v2) {
    const float center_u = fdiv((u0 + u1) + u2, 3.0f), center_v = fdiv((v0 + v1) + v2, 3.0f);
    const uint64_t key = tile_key(floor_as_i32(center_u), floor_as_i32(center_v));
    uint32_t lo = 0u, hi = T.n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (T.keys[mid] < key) lo = mid + 1u;
        else hi = mid;
    }
    return (lo < T.n && T.keys[lo] == key) ? T.slots[lo] : 0u;
}

}  // namespace

// One workgroup per box, three passes over its cells in rounds of GEN_WG, two triangles a lane (triangle t = 2 * cell + k):
//   A  keep flag and tile slot of every triangle into the call scratch, the slots present into an LDS bitmap (integer OR: no order);
//      a popcount prefix over the bitmap ranks the slots: group = slots present below this one.
//   B  an ORDERED segmented scan in triangle order of (triangles, first-use vertices) per group: inside a wave one DPP prefix sum per
//      distinct group present (ballot, the first pending lane's group), across the waves their totals per group in LDS, across the
//      rounds running counters per group in LDS.  No atomic decides a position.  First-use vertices and uvs are written here, and in the
//      unshared layout (every triangle owns its corners) the indices as well.
//   C  shared layout only: a corner's index is vertex_base(first triangle of its group that names the grid point) + the first uses
//      ahead of that corner inside it; both were written to the scratch in pass B, a workgroup barrier lies between.
// A grid point (vx, vy) is named by at most six triangles, in ascending order: cell (vx-1, vy-1) triangle 1 (as its corner 2), cell
// (vx, vy-1) triangles 0 and 1 (corner 1 of both), cell (vx-1, vy) triangle 0 (corner 2) and triangle 1 (corner 0), cell (vx, vy)
// triangle 0 (corner 0).  In the shared layout every triangle is kept, so "same group" is "same slot".
extern "C" __global__ __launch_bounds__(GEN_WG) void k_terrain_tiles_emit(TileEmitArgs A) {
    __shared__ uint32_t bitmap[TILE_BITMAP_WORDS];    // tile slots present in this box
    __shared__ uint32_t rank0[TILE_BITMAP_WORDS];     // slots present in the words before
    __shared__ uint32_t wave_total[GEN_WG / 64u][RXR_TERRAIN_TILES_MAX_GROUPS];   // a round's triangles | first uses << 16, per wave and group
    __shared__ uint32_t run_tri[RXR_TERRAIN_TILES_MAX_GROUPS], run_vtx[RXR_TERRAIN_TILES_MAX_GROUPS];
    constexpr uint32_t NONE = 0xFFFFFFFFu;
    const ExclBox b = A.box[blockIdx.x];
    const uint32_t tid = threadIdx.x, sx = (uint32_t)b.g.sx, sy = (uint32_t)b.g.sy, G = A.max_groups;
    const bool unshared = b.active != 0u;
    const uint32_t cw = sx > 1u ? sx - 1u : 0u, ch = sy > 1u ? sy - 1u : 0u;
    const uint32_t n_cells = b.np ? cw * ch : 0u, nt = 2u * n_cells;   // (2 * n_cells <= triangle_stride: checked on the host)
    const float *hts = A.heights + b.point0;
    const uint32_t *masks = A.masks + b.mask0;
    uint32_t *rec_slot = A.tris + A.tri0[blockIdx.x], *rec_base = rec_slot + nt, *rec_pos = rec_base + nt, *rec_first = rec_pos + nt;
    uint32_t *counts = A.counts + 2 * (size_t)blockIdx.x * G, *group_tiles = A.group_tiles + (size_t)blockIdx.x * G;
    auto grid_x = [&](uint32_t ix) { return b.g.min_x + (float)(int32_t)ix * A.cell_size; };
    auto grid_z = [&](uint32_t iy) { return b.g.min_y + (float)(int32_t)iy * A.cell_size; };

    for (uint32_t i = tid; i < TILE_BITMAP_WORDS; i += GEN_WG) bitmap[i] = 0u;
    if (tid < RXR_TERRAIN_TILES_MAX_GROUPS) {
        run_tri[tid] = run_vtx[tid] = 0u;
        for (uint32_t w = 0; w < GEN_WG / 64u; ++w) wave_total[w][tid] = 0u;
    }
    __syncthreads();
    // ---- A
    const uint32_t words = (b.active + 31u) >> 5;
    for (uint32_t cell = tid; cell < n_cells; cell += GEN_WG) {
        const uint32_t cy = cell / cw, cx = cell - cy * cw;
        const uint32_t i0 = cy * sx + cx, i1 = i0 + 1u, i2 = i0 + sx, i3 = i2 + 1u;
        uint32_t drop0 = 0u, drop1 = 0u;
        for (uint32_t w = 0; w < words; ++w) {
            const uint32_t *m = masks + (size_t)w * b.np;
            const uint32_t m12 = m[i1] & m[i2];
            drop0 |= m[i0] & m12;
            drop1 |= m12 & m[i3];
        }
        const float x0 = grid_x(cx), x1 = grid_x(cx + 1u), z0 = grid_z(cy), z1 = grid_z(cy + 1u);
        const uint32_t s0 = drop0 ? NONE : tile_slot(A.T, x0, x0, x1, z0, z1, z0);   // (i0, i2, i1)
        const uint32_t s1 = drop1 ? NONE : tile_slot(A.T, x1, x0, x1, z0, z1, z1);   // (i1, i2, i3)
        rec_slot[2u * cell] = s0, rec_slot[2u * cell + 1u] = s1;
        if (s0 != NONE) atomicOr(&bitmap[s0 >> 5], 1u << (s0 & 31u));   // (slots are below n_tiles <= 32 * TILE_BITMAP_WORDS: checked at registration)
        if (s1 != NONE) atomicOr(&bitmap[s1 >> 5], 1u << (s1 & 31u));
    }
    __syncthreads();
    if (tid < TILE_BITMAP_WORDS) {
        uint32_t r = 0u;
        for (uint32_t w = 0; w < tid; ++w) r += __popc(bitmap[w]);
        rank0[tid] = r;
    }
    __syncthreads();
    const uint32_t n_groups = rank0[TILE_BITMAP_WORDS - 1u] + __popc(bitmap[TILE_BITMAP_WORDS - 1u]);   // (<= max_groups: bounded on the host)
    auto group_of = [&](uint32_t slot) { return rank0[slot >> 5] + __popc(bitmap[slot >> 5] & ((1u << (slot & 31u)) - 1u)); };
    if (tid < TILE_BITMAP_WORDS) {
        uint32_t word = bitmap[tid], r = rank0[tid];
        for (; word; word &= word - 1u, ++r)
            if (r < G) group_tiles[r] = 32u * tid + (uint32_t)__builtin_ctz(word);
    }
    for (uint32_t g = tid; g < G; g += GEN_WG)
        if (g >= n_groups) group_tiles[g] = NONE, counts[2u * g] = 0u, counts[2u * g + 1u] = 0u;
    // the first triangle of slot `s` that names grid point (vx, vy), and which of its corners that is
    auto first_user = [&](uint32_t vx, uint32_t vy, uint32_t s, uint32_t &corner) -> uint32_t {
        if (vy >= 1u) {
            const uint32_t row = (vy - 1u) * cw;
            if (vx >= 1u && rec_slot[2u * (row + vx - 1u) + 1u] == s) return corner = 2u, 2u * (row + vx - 1u) + 1u;
            if (vx < cw) {
                const uint32_t t = 2u * (row + vx);
                if (rec_slot[t] == s) return corner = 1u, t;
                if (rec_slot[t + 1u] == s) return corner = 1u, t + 1u;
            }
        }
        if (vy < ch) {
            const uint32_t row = vy * cw;
            if (vx >= 1u) {
                const uint32_t t = 2u * (row + vx - 1u);
                if (rec_slot[t] == s) return corner = 2u, t;
                if (rec_slot[t + 1u] == s) return corner = 0u, t + 1u;
            }
            if (vx < cw && rec_slot[2u * (row + vx)] == s) return corner = 0u, 2u * (row + vx);
        }
        return corner = 0u, NONE;   // (not reached for a corner of a triangle of slot s)
    };
    // ---- B
    for (uint32_t c0 = 0; c0 < n_cells; c0 += GEN_WG) {
        const uint32_t cell = c0 + tid;
        const bool valid = cell < n_cells;
        const uint32_t cy = valid ? cell / cw : 0u, cx = valid ? cell - cy * cw : 0u;
        const uint32_t s0 = valid ? rec_slot[2u * cell] : NONE, s1 = valid ? rec_slot[2u * cell + 1u] : NONE;
        uint32_t g0 = s0 != NONE ? group_of(s0) : NONE, g1 = s1 != NONE ? group_of(s1) : NONE;
        if (g0 >= G) g0 = NONE;   // (never: the host refuses a box that can have more groups)
        if (g1 >= G) g1 = NONE;
        // the corners as grid coordinates: triangle 0 = (i0, i2, i1), triangle 1 = (i1, i2, i3)
        const uint32_t px[2][3] = {{cx, cx, cx + 1u}, {cx + 1u, cx, cx + 1u}}, py[2][3] = {{cy, cy + 1u, cy}, {cy, cy + 1u, cy + 1u}};
        uint32_t f0 = 7u, f1 = 7u;   // first-use corners, bit j = corner j
        if (!unshared) {
            f0 = f1 = 0u;
            uint32_t corner;
#pragma unroll
            for (uint32_t j = 0; j < 3u; ++j) {
                if (g0 != NONE && first_user(px[0][j], py[0][j], s0, corner) == 2u * cell) f0 |= 1u << j;
                if (g1 != NONE && first_user(px[1][j], py[1][j], s1, corner) == 2u * cell + 1u) f1 |= 1u << j;
            }
        }
        const uint32_t n0 = __popc(f0), n1 = __popc(f1);
        uint32_t pos0 = 0u, base0 = 0u, pos1 = 0u, base1 = 0u;
        bool todo0 = g0 != NONE, todo1 = g1 != NONE;
        for (;;) {   // (wave-uniform: one turn per distinct group of this wave's triangles)
            const unsigned long long pending = __builtin_amdgcn_ballot_w64(todo0 || todo1);
            if (!pending) break;
            const uint32_t g = (uint32_t)__builtin_amdgcn_readlane((int)(todo0 ? g0 : g1), (int)__builtin_ctzll(pending));
            const bool a0 = todo0 && g0 == g, a1 = todo1 && g1 == g;
            const uint32_t v = (a0 ? 1u + (n0 << 16) : 0u) + (a1 ? 1u + (n1 << 16) : 0u);   // (a wave has at most 128 triangles, 384 corners)
            const uint32_t inclusive = rxm::wave_inclusive_add(v), before = inclusive - v;
            if (a0) pos0 = before & 0xFFFFu, base0 = before >> 16;
            if (a1) pos1 = (before & 0xFFFFu) + (a0 ? 1u : 0u), base1 = (before >> 16) + (a0 ? n0 : 0u);
            if ((tid & 63u) == 63u) wave_total[tid >> 6][g] = inclusive;
            todo0 = todo0 && !a0, todo1 = todo1 && !a1;
        }
        __syncthreads();
#pragma unroll
        for (uint32_t k = 0; k < 2u; ++k) {
            const uint32_t g = k ? g1 : g0;
            if (g == NONE) continue;
            uint32_t pos = (k ? pos1 : pos0) + run_tri[g], base = (k ? base1 : base0) + run_vtx[g];
            for (uint32_t w = 0; w < (tid >> 6); ++w) {
                const uint32_t t = wave_total[w][g];
                pos += t & 0xFFFFu, base += t >> 16;
            }
            const uint32_t first = k ? f1 : f0, t = 2u * cell + k;
            const size_t mesh = (size_t)blockIdx.x * G + g;
            float *vtx = A.vertices + mesh * A.vstride * 4, *uv = A.uvs + mesh * A.vstride * 2;
            uint32_t slot = base;
#pragma unroll
            for (uint32_t j = 0; j < 3u; ++j) {
                if (!(first >> j & 1u) || slot >= A.vstride) continue;   // (the stride holds every first use: checked on the host)
                const float x = grid_x(px[k][j]), z = grid_z(py[k][j]);
                float *o = vtx + 4 * (size_t)slot;
                o[0] = x, o[1] = hts[py[k][j] * sx + px[k][j]], o[2] = z, o[3] = 1.0f;
                uv[2 * (size_t)slot] = x, uv[2 * (size_t)slot + 1] = z;
                ++slot;
            }
            if (pos >= A.tstride) continue;
            if (unshared) {
                uint32_t *idx = A.indices + (mesh * A.tstride + pos) * 3;
                idx[0] = base, idx[1] = base + 1u, idx[2] = base + 2u;
            } else {
                rec_base[t] = base, rec_pos[t] = pos, rec_first[t] = first;
            }
        }
        __syncthreads();
        if (tid < RXR_TERRAIN_TILES_MAX_GROUPS) {
            uint32_t tri = 0u, vtx = 0u;
            for (uint32_t w = 0; w < GEN_WG / 64u; ++w) {
                const uint32_t t = wave_total[w][tid];
                tri += t & 0xFFFFu, vtx += t >> 16;
                wave_total[w][tid] = 0u;
            }
            run_tri[tid] += tri, run_vtx[tid] += vtx;
        }
        __syncthreads();   // (the totals are rewritten by the next round; the scratch of this one is read in pass C)
    }
    // ---- C
    if (!unshared) {
        for (uint32_t t = tid; t < nt; t += GEN_WG) {
            const uint32_t s = rec_slot[t], g = group_of(s);
            if (g >= G || rec_pos[t] >= A.tstride) continue;
            const uint32_t cell = t >> 1, k = t & 1u, cy = cell / cw, cx = cell - cy * cw;
            const uint32_t px[3] = {k ? cx + 1u : cx, cx, cx + 1u}, py[3] = {cy, cy + 1u, k ? cy + 1u : cy};
            uint32_t *idx = A.indices + (((size_t)blockIdx.x * G + g) * A.tstride + rec_pos[t]) * 3;
#pragma unroll
            for (uint32_t j = 0; j < 3u; ++j) {
                uint32_t corner;
                const uint32_t f = first_user(px[j], py[j], s, corner);
                idx[j] = f != NONE ? rec_base[f] + __popc(rec_first[f] & ((1u << corner) - 1u)) : 0u;
            }
        }
    }
    if (tid < n_groups && tid < G) counts[2u * tid] = run_vtx[tid], counts[2u * tid + 1u] = run_tri[tid];
    if (tid == 0u) {
        uint32_t *bc = A.box_counts + 4 * (size_t)blockIdx.x;
        bc[0] = sx, bc[1] = sy, bc[2] = b.active, bc[3] = n_groups;
    }
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

// the rounds of a call: up to EXCL_LAUNCH_BOXES boxes, up to `bound` points, up to GEN_LAUNCH_WORK point-records (rxr_terrain_gen.h: what
// a launch of the height field takes) and fewer than 2^32 scratch words (at least one box); every box's place in its round's scratch.
// extra: words a box needs behind the round's heights and mask words (the tile meshes' triangle records), extra0: where they start
// behind those; both may be NULL
struct Rounds {
    std::vector<uint32_t> boxes;   // boxes per round
    size_t scratch_words = 0;      // the largest round's
};
Rounds cut_rounds(std::vector<ExclBox> &boxes, const std::vector<uint64_t> &work, const std::vector<uint64_t> *extra = nullptr, std::vector<uint32_t> *extra0 = nullptr) {
    const uint32_t n = (uint32_t)boxes.size();
    const uint32_t bound = launch_points();
    Rounds R;
    for (uint32_t b0 = 0; b0 < n;) {
        uint32_t nb = 0;
        unsigned long long points = 0, mask_words = 0, records = 0, extra_words = 0;
        while (b0 + nb < n && nb < EXCL_LAUNCH_BOXES) {
            ExclBox &b = boxes[b0 + nb];
            const unsigned long long mw = (unsigned long long)b.np * ((b.active + 31u) >> 5), xw = extra ? (*extra)[b0 + nb] : 0;
            if (nb && (points + b.np > bound || records + work[b0 + nb] > GEN_LAUNCH_WORK || (mask_words + mw) >> 32 || (extra_words + xw) >> 32)) break;
            records += work[b0 + nb];
            b.point0 = (uint32_t)points;
            b.mask0 = (uint32_t)mask_words;
            if (extra0) (*extra0)[b0 + nb] = (uint32_t)extra_words;
            points += b.np;
            mask_words += mw;
            extra_words += xw;
            ++nb;
        }
        R.boxes.push_back(nb);
        R.scratch_words = std::max<size_t>(R.scratch_words, points + mask_words + extra_words);
        b0 += nb;
    }
    return R;
}

// every box of a call into device arrays, queued on `s`
int meshes_run(rxr_ctx *ctx, std::vector<ExclBox> &boxes, const std::vector<uint64_t> &work, float cell_size, uint32_t stride, uint32_t *counts, float *vertices,
               hipStream_t s) {
    const Rounds R = cut_rounds(boxes, work);
    const std::vector<uint32_t> &round_boxes = R.boxes;
    const size_t scratch_words = R.scratch_words;
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

// ---- the tile meshes' host ----
// the sorted keys of the cells, or the refusal; `order`: cell order[i] has the i-th smallest key
int check_tiles(const int32_t *cells, const uint32_t *slots, uint32_t n, uint32_t n_tiles, std::vector<uint32_t> &order, std::string &err) {
    auto bad = [&](int code, const std::string &m) {
        err = m;
        return code;
    };
    if (n > RXR_TERRAIN_TILES_MAX_CELLS) return bad(RXR_ERR_UNSUPPORTED, std::to_string(n) + " cells exceed RXR_TERRAIN_TILES_MAX_CELLS");
    if (n_tiles > RXR_TERRAIN_TILES_MAX_TILES) return bad(RXR_ERR_UNSUPPORTED, std::to_string(n_tiles) + " tiles exceed RXR_TERRAIN_TILES_MAX_TILES");
    if (!n_tiles) return bad(RXR_ERR_INVALID, "n_tiles must be at least 1 (slot 0 is the default tile)");
    if (n && !cells) return bad(RXR_ERR_INVALID, "NULL cells");
    if (n && !slots) return bad(RXR_ERR_INVALID, "NULL slots");
    for (uint32_t i = 0; i < n; ++i)
        if (slots[i] >= n_tiles) return bad(RXR_ERR_INVALID, "slots[" + std::to_string(i) + "] = " + std::to_string(slots[i]) + " is not below n_tiles = " + std::to_string(n_tiles));
    order.resize(n);
    for (uint32_t i = 0; i < n; ++i) order[i] = i;
    auto key = [&](uint32_t i) { return tile_key(cells[2 * (size_t)i], cells[2 * (size_t)i + 1]); };
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return key(a) < key(b); });
    for (uint32_t i = 1; i < n; ++i)
        if (key(order[i]) == key(order[i - 1]))
            return bad(RXR_ERR_INVALID, "cell (" + std::to_string(cells[2 * (size_t)order[i]]) + ", " + std::to_string(cells[2 * (size_t)order[i] + 1]) + ") is listed twice (entries " +
                                            std::to_string(std::min(order[i], order[i - 1])) + " and " + std::to_string(std::max(order[i], order[i - 1])) + ")");
    return RXR_OK;
}

// an upper bound of the groups box `e` can have: slot 0 and the distinct other slots among the override cells its triangles' centres
// can fall into.  A centre lies strictly between the grid's first and last coordinate of an axis as long as the rounding of three
// f32 operations is small against a third of a cell; where that cannot be relied on (huge or non-finite coordinates) every
// registered slot counts.
uint32_t groups_bound(const rxr_ctx *ctx, const ExclBox &e, float cell_size, std::vector<uint64_t> &seen) {
    const uint32_t n = ctx->tile_cells;
    std::fill(seen.begin(), seen.end(), 0ull);
    uint32_t distinct = 0;
    auto take = [&](uint32_t slot) {
        if (slot && !(seen[slot >> 6] >> (slot & 63u) & 1ull)) seen[slot >> 6] |= 1ull << (slot & 63u), ++distinct;
    };
    const float lo_x = e.g.min_x, lo_z = e.g.min_y, hi_x = e.g.min_x + (float)(e.g.sx - 1) * cell_size, hi_z = e.g.min_y + (float)(e.g.sy - 1) * cell_size;
    const float big = std::max(std::max(std::fabs(lo_x), std::fabs(hi_x)), std::max(std::fabs(lo_z), std::fabs(hi_z)));
    const bool tight = big == big && big < 0x1p20f && 16.0f * (big * 0x1p-23f) < cell_size / 3.0f;
    if (!tight) {
        for (uint32_t i = 0; i < n; ++i) take(ctx->tile_slots[i]);
        return distinct + 1u;
    }
    const int32_t x0 = as_i32(std::floor(lo_x)), x1 = as_i32(std::ceil(hi_x)) - 1, z0 = as_i32(std::floor(lo_z)), z1 = as_i32(std::ceil(hi_z)) - 1;
    if ((uint64_t)((int64_t)x1 - x0 + 1) > n) {   // fewer overrides than columns: look at each override
        for (uint32_t i = 0; i < n; ++i) {
            const int32_t x = (int32_t)((uint32_t)(ctx->tile_keys[i] >> 32) ^ 0x80000000u), z = (int32_t)((uint32_t)ctx->tile_keys[i] ^ 0x80000000u);
            if (x >= x0 && x <= x1 && z >= z0 && z <= z1) take(ctx->tile_slots[i]);
        }
    } else {
        for (int32_t x = x0; x <= x1; ++x) {   // a column's cells lie side by side in the sorted keys
            const uint64_t first = tile_key(x, z0), last = tile_key(x, z1);
            for (size_t i = std::lower_bound(ctx->tile_keys.begin(), ctx->tile_keys.end(), first) - ctx->tile_keys.begin(); i < n && ctx->tile_keys[i] <= last; ++i) take(ctx->tile_slots[i]);
        }
    }
    return distinct + 1u;
}

struct TileCall {
    std::vector<ExclBox> boxes;
    std::vector<uint64_t> work, records;   // records[i]: words of box i's triangle records
    float cell_size;
    uint32_t max_groups, vstride, tstride;
    size_t meshes;                         // n * max_groups
};

// the boxes of a tile-mesh call and everything it refuses before anything is queued
int tile_boxes(rxr_ctx *ctx, const char *who, const float *boxes, uint32_t n, uint32_t subdivisions, uint32_t max_groups, uint32_t vstride, uint32_t tstride, TileCall &c) {
    const std::string w = who;
    if (!ctx->gen_set) return rxr_fail(ctx, RXR_ERR_INVALID, w + ": no terrain generator is resident (rxr_set_terrain_generator)");
    if (!subdivisions) return rxr_fail(ctx, RXR_ERR_INVALID, w + ": subdivisions must be at least 1 (the reference divides by it)");
    if (!max_groups) return rxr_fail(ctx, RXR_ERR_INVALID, w + ": max_groups must be at least 1");
    if (max_groups > RXR_TERRAIN_TILES_MAX_GROUPS) return rxr_fail(ctx, RXR_ERR_UNSUPPORTED, w + ": max_groups = " + std::to_string(max_groups) + " exceeds RXR_TERRAIN_TILES_MAX_GROUPS");
    if (n && !boxes) return rxr_fail(ctx, RXR_ERR_INVALID, w + ": NULL boxes");
    size_t total;
    if (__builtin_mul_overflow((size_t)n, (size_t)max_groups, &c.meshes) || __builtin_mul_overflow(c.meshes, (size_t)vstride * 16u, &total) ||
        __builtin_mul_overflow(c.meshes, (size_t)tstride * 12u, &total))
        return rxr_fail(ctx, RXR_ERR_INVALID, w + ": an output array's size overflows");
    c.cell_size = 1.0f / (float)subdivisions;
    c.max_groups = max_groups, c.vstride = vstride, c.tstride = tstride;
    c.boxes.resize(n), c.work.resize(n), c.records.resize(n);
    const float *sb = ctx->excl_boxes.data();
    const uint64_t base_records = (uint64_t)ctx->gen_n[0] + ctx->gen_n[2] + ctx->gen_n[3] + ctx->excl_S / 8u;
    std::vector<uint64_t> seen((ctx->tile_count + 63u) / 64u);
    for (uint32_t i = 0; i < n; ++i) {
        const float *b = boxes + 4 * (size_t)i;
        const std::string bi = w + ": box " + std::to_string(i);
        ExclBox e{};
        e.g = grid_box(b, c.cell_size);
        memcpy(e.raw, b, sizeof e.raw);
        uint64_t active_vertices = 0;
        for (uint32_t s = 0; s < ctx->excl_S; ++s)   // BBox::intersects (src/map/bbox.rs:43-48), the sector's box first
            if (sb[4 * s] <= b[2] && sb[4 * s + 2] >= b[0] && sb[4 * s + 1] <= b[3] && sb[4 * s + 3] >= b[1]) {
                ++e.active;
                active_vertices += ctx->excl_voff[s + 1] - ctx->excl_voff[s];
            }
        const uint64_t points = (uint64_t)e.g.sx * (uint64_t)e.g.sy;
        const uint64_t cells = (e.g.sx > 1 && e.g.sy > 1) ? (uint64_t)(e.g.sx - 1) * (uint64_t)(e.g.sy - 1) : 0;
        const uint64_t most_vertices = e.active ? 6 * cells : (cells ? points : 0);   // one group can own the whole box
        const std::string grid = " has a grid of " + std::to_string(e.g.sx) + " x " + std::to_string(e.g.sy) + " points and " + std::to_string(e.active) + " active sectors: up to ";
        if (most_vertices > vstride) return rxr_fail(ctx, RXR_ERR_INVALID, bi + grid + std::to_string(most_vertices) + " vertices in a group, more than vertex_stride = " + std::to_string(vstride));
        if (2 * cells > tstride) return rxr_fail(ctx, RXR_ERR_INVALID, bi + grid + std::to_string(2 * cells) + " triangles in a group, more than triangle_stride = " + std::to_string(tstride));
        e.np = (uint32_t)(cells ? points : 0);   // (a grid without a cell has no triangle, so no group: none of its points is needed)
        if ((uint64_t)e.np * ((e.active + 31u) >> 5) >> 32) return rxr_fail(ctx, RXR_ERR_OOM, bi + " needs 2^32 or more mask words of scratch");
        if (cells) {
            const uint32_t bound = groups_bound(ctx, e, c.cell_size, seen);
            if (bound > max_groups)
                return rxr_fail(ctx, RXR_ERR_INVALID, bi + " can have " + std::to_string(bound) + " tile groups (the default tile and the distinct slots of the override cells in its range), more than max_groups = " +
                                                          std::to_string(max_groups));
        }
        c.boxes[i] = e;
        c.work[i] = (uint64_t)e.np * std::max<uint64_t>(base_records + active_vertices, 1);
        c.records[i] = 2 * cells * TILE_RECORD_WORDS;   // (2 * cells <= triangle_stride < 2^32)
    }
    return RXR_OK;
}

struct TileOut {
    uint32_t *box_counts, *counts, *group_tiles;
    float *vertices, *uvs;
    uint32_t *indices;
};

// every box of a tile-mesh call into device arrays, queued on `s`: per round the classification as in meshes_run, then the tile emission
int tiles_run(rxr_ctx *ctx, TileCall &c, const TileOut &o, hipStream_t s) {
    const uint32_t n = (uint32_t)c.boxes.size();
    std::vector<uint32_t> tri0(n);
    const Rounds R = cut_rounds(c.boxes, c.work, &c.records, &tri0);
    int rc = rxr_query_begin(ctx, ctx->lane[Q_EXCL], s);
    if (rc != RXR_OK) return rc;
    if ((rc = rxr_ensure(ctx, ctx->d_excl_scratch, std::max<size_t>(R.scratch_words * 4, 256))) != RXR_OK) return rc;
    ctx->tile_launches = 0;
    ExclClassifyArgs C{};
    C.G = records_of(ctx);
    C.E = excl_records_of(ctx);
    C.cell_size = c.cell_size;
    TileEmitArgs M{};
    M.cell_size = c.cell_size;
    M.max_groups = c.max_groups, M.vstride = c.vstride, M.tstride = c.tstride;
    M.T.n = ctx->tile_cells;
    M.T.keys = (const uint64_t *)ctx->d_tiles.p;
    M.T.slots = (const uint32_t *)((const uint8_t *)ctx->d_tiles.p + 8 * (size_t)ctx->tile_cells);
    uint32_t b0 = 0;
    for (const uint32_t nb : R.boxes) {
        uint32_t most = 0, most_words = 1;
        unsigned long long points = 0, mask_words = 0;
        for (uint32_t k = 0; k < nb; ++k) {
            const ExclBox &b = c.boxes[b0 + k];
            C.box[k] = M.box[k] = b;
            M.tri0[k] = tri0[b0 + k];
            points += b.np;
            mask_words += (unsigned long long)b.np * ((b.active + 31u) >> 5);
            most = std::max(most, b.np);
            most_words = std::max(most_words, (b.active + 31u) >> 5);
        }
        C.heights = (float *)ctx->d_excl_scratch.p;
        C.masks = (uint32_t *)ctx->d_excl_scratch.p + points;   // (the round's heights, its mask words, then its triangle records)
        M.heights = C.heights;
        M.masks = C.masks;
        M.tris = C.masks + mask_words;
        const size_t m0 = (size_t)b0 * c.max_groups;
        M.box_counts = o.box_counts + 4 * (size_t)b0;
        M.counts = o.counts + 2 * m0;
        M.group_tiles = o.group_tiles + m0;
        M.vertices = o.vertices + m0 * c.vstride * 4;
        M.uvs = o.uvs + m0 * c.vstride * 2;
        M.indices = o.indices + m0 * c.tstride * 3;
        if (most) {
            hipLaunchKernelGGL(k_terrain_excl_classify, dim3((most + GEN_WG - 1u) / GEN_WG, nb, most_words), dim3(GEN_WG), 0, s, C);
            HIPCHK(ctx, hipGetLastError());
        }
        // (a round of grids without a cell still writes their counts)
        hipLaunchKernelGGL(k_terrain_tiles_emit, dim3(nb), dim3(GEN_WG), 0, s, M);
        HIPCHK(ctx, hipGetLastError());
        ++ctx->tile_launches;
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

int rxr_check_terrain_tiles(const int32_t *cells, const uint32_t *slots, uint32_t n_cells, uint32_t n_tiles, char *message, uint32_t message_capacity) {
    std::string err;
    std::vector<uint32_t> order;
    const int rc = check_tiles(cells, slots, n_cells, n_tiles, order, err);
    rxr_copy_message(err, message, message_capacity);
    return rc;
}

int rxr_set_terrain_tiles(rxr_ctx *ctx, const int32_t *cells, const uint32_t *slots, uint32_t n_cells, uint32_t n_tiles) {
    if (!ctx) return RXR_ERR_INVALID;
    if (ctx->group) return rxr_as_member0(ctx, [&](rxr_ctx *m) { return rxr_set_terrain_tiles(m, cells, slots, n_cells, n_tiles); });
    std::string err;
    std::vector<uint32_t> order;
    int rc = check_tiles(cells, slots, n_cells, n_tiles, order, err);
    if (rc != RXR_OK) return rxr_fail(ctx, rc, "rxr_set_terrain_tiles: " + err);
    const uint32_t n = n_cells;
    std::vector<uint64_t> keys(n);
    std::vector<uint32_t> sorted_slots(n);
    for (uint32_t i = 0; i < n; ++i) {
        keys[i] = tile_key(cells[2 * (size_t)order[i]], cells[2 * (size_t)order[i] + 1]);
        sorted_slots[i] = slots[order[i]];
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if ((rc = rxr_quiesce(ctx)) != RXR_OK) return rc;   // queued tile-mesh calls read what is replaced here
    // the map goes into a buffer of its own, and the old one is let go only when the new one holds the map: a call that fails
    // here leaves the resident map as it was (once a map edit: the allocation does not matter)
    DevBuf fresh;
    if ((rc = rxr_ensure(ctx, fresh, std::max<size_t>(12 * (size_t)n, 256))) != RXR_OK) return rc;
    auto upload = [&]() -> int {
        if (!n) return RXR_OK;
        HIPCHK(ctx, hipMemcpyAsync(fresh.p, keys.data(), 8 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync((uint8_t *)fresh.p + 8 * (size_t)n, sorted_slots.data(), 4 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // (the vectors are read until here)
        return RXR_OK;
    };
    if ((rc = upload()) != RXR_OK) {
        (void)hipFree(fresh.p);
        return rc;
    }
    if (ctx->d_tiles.p) (void)hipFree(ctx->d_tiles.p);   // (nothing queued reads it: rxr_quiesce above)
    ctx->d_tiles = fresh;
    ctx->tile_keys.swap(keys);
    ctx->tile_slots.swap(sorted_slots);
    ctx->tile_cells = n, ctx->tile_count = n_tiles;
    return RXR_OK;
}

int rxr_generated_tile_meshes(rxr_ctx *ctx, const float *boxes, uint32_t n, uint32_t subdivisions, uint32_t max_groups, uint32_t vertex_stride, uint32_t triangle_stride,
                              uint32_t *box_counts, uint32_t *counts, uint32_t *group_tiles, float *vertices, float *uvs, uint32_t *indices) {
    if (!ctx) return RXR_ERR_INVALID;
    if (ctx->group)
        return rxr_as_member0(ctx, [&](rxr_ctx *m) {
            return rxr_generated_tile_meshes(m, boxes, n, subdivisions, max_groups, vertex_stride, triangle_stride, box_counts, counts, group_tiles, vertices, uvs, indices);
        });
    TileCall c;
    int rc = tile_boxes(ctx, "rxr_generated_tile_meshes", boxes, n, subdivisions, max_groups, vertex_stride, triangle_stride, c);
    if (rc != RXR_OK) return rc;
    if (!n) return RXR_OK;
    if (!box_counts || !counts || !group_tiles || ((!vertices || !uvs) && vertex_stride) || (!indices && triangle_stride))
        return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_generated_tile_meshes: NULL output array");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // vertices, uvs and indices go up as well as down: the slots past a mesh's counts come back as the caller left them
    QueryIO io{ctx, ctx->lane[Q_EXCL]};
    const unsigned i_b = io.out(box_counts, (size_t)n * 16), i_c = io.out(counts, c.meshes * 8), i_g = io.out(group_tiles, c.meshes * 4);
    const unsigned i_v = io.inout(vertex_stride ? vertices : nullptr, c.meshes * vertex_stride * 16), i_u = io.inout(vertex_stride ? uvs : nullptr, c.meshes * vertex_stride * 8);
    const unsigned i_i = io.inout(triangle_stride ? indices : nullptr, c.meshes * triangle_stride * 12);
    if ((rc = io.upload()) != RXR_OK) return rc;
    const TileOut o{io.dev<uint32_t>(i_b), io.dev<uint32_t>(i_c), io.dev<uint32_t>(i_g), io.dev<float>(i_v), io.dev<float>(i_u), io.dev<uint32_t>(i_i)};
    if ((rc = tiles_run(ctx, c, o, ctx->stream)) != RXR_OK) return rc;
    return io.download();
}

int rxr_generated_tile_meshes_to(rxr_ctx *ctx, const float *boxes, uint32_t n, uint32_t subdivisions, uint32_t max_groups, uint32_t vertex_stride, uint32_t triangle_stride,
                                 uint32_t *dev_box_counts, uint32_t *dev_counts, uint32_t *dev_group_tiles, float *dev_vertices, float *dev_uvs, uint32_t *dev_indices,
                                 void *hip_stream) {
    if (!ctx) return RXR_ERR_INVALID;
    if (ctx->group)
        return rxr_fail(ctx, RXR_ERR_UNSUPPORTED, "rxr_generated_tile_meshes_to on a multi-device context: device pointers and streams belong to ONE device (use rxr_member)");
    TileCall c;
    int rc = tile_boxes(ctx, "rxr_generated_tile_meshes_to", boxes, n, subdivisions, max_groups, vertex_stride, triangle_stride, c);
    if (rc != RXR_OK) return rc;
    if (!n) return RXR_OK;
    if (!dev_box_counts || !dev_counts || !dev_group_tiles || ((!dev_vertices || !dev_uvs) && vertex_stride) || (!dev_indices && triangle_stride))
        return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_generated_tile_meshes_to: NULL output array");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const void *const p[6] = {dev_box_counts, dev_counts, dev_group_tiles, vertex_stride ? dev_vertices : nullptr, vertex_stride ? dev_uvs : nullptr, triangle_stride ? dev_indices : nullptr};
    const size_t bytes[6] = {(size_t)n * 16, c.meshes * 8, c.meshes * 4, c.meshes * vertex_stride * 16, c.meshes * vertex_stride * 8, c.meshes * triangle_stride * 12};
    const char *const names[6] = {"dev_box_counts", "dev_counts", "dev_group_tiles", "dev_vertices", "dev_uvs", "dev_indices"};
    if ((rc = device_arrays(ctx, "rxr_generated_tile_meshes_to", p, bytes, names, 6)) != RXR_OK) return rc;
    const TileOut o{dev_box_counts, dev_counts, dev_group_tiles, dev_vertices, dev_uvs, dev_indices};
    return tiles_run(ctx, c, o, hip_stream ? (hipStream_t)hip_stream : ctx->stream);
}

// test-only: the rounds (one classification and one tile emission launch each) of the last tile-mesh call
uint32_t rxr_debug_terrain_tile_launches(rxr_ctx *ctx) {
    if (!ctx) return 0;
    if (ctx->group) return rxr_debug_terrain_tile_launches(rxr_member(ctx, 0));
    return ctx->tile_launches;
}

// test-only: the rounds (one classification and one emission launch each) of the last mesh call
uint32_t rxr_debug_terrain_excl_launches(rxr_ctx *ctx) {
    if (!ctx) return 0;
    if (ctx->group) return rxr_debug_terrain_excl_launches(rxr_member(ctx, 0));
    return ctx->excl_launches;
}

}  // extern "C"
