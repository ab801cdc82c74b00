// rxr_terrain_mesh.hip -- the geometry a terrain chunk's texture is drawn on: TerrainChunk::build_mesh (src/terrain/chunk.rs:253-297)
// with Batch3D::compute_vertex_normals (src/batch/batch3d.rs:771-809).  include/rxr.h: rxr_terrain_meshes, rxr_terrain_meshes_to.
//
// Semantics, all f32, one operation per reference operation in its order, nothing fused (the build's -ffp-contract=off).  The
// reference walks a hash map of the chunk's cells; this is the mesh it builds when the cells are visited in ascending (ly, lx), row
// by row.  For that order the dictionary has a closed form -- cells and corners in chunk-local coordinates, a
// cell PRESENT iff the caller listed it in rxr_set_terrain_heights:
//   owner     corner (px, py), 0 <= px, py <= cs, belongs to the first present cell among (px-1, py-1), (px, py-1), (px-1, py), (px, py);
//             a corner without an owner is not a vertex
//   vertex    index = corners owned by the cells before the owner in row-major order + the corner's rank among the owner's own corners
//             in the order (0,0), (1,0), (0,1), (1,1);  value = [X as f32 * scale.x, get_height(X, Y), Y as f32 * scale.y, 1] with
//             (X, Y) the corner in world cells -- the last row and column read the neighbouring chunks, or 0.0
//   triangle  2 rank(cell) = (i0, i2, i1) and 2 rank(cell) + 1 = (i1, i2, i3), rank = present cells before it, i0..i3 its corners
//   normal    the sum, from +0.0, of normalized(cross(p1 - p0, p2 - p0)) over the corner's incident triangles in ascending index:
//             cell (px-1, py-1) triangle 1; (px, py-1) triangles 0, 1; (px-1, py) triangles 0, 1; (px, py) triangle 0 (present cells
//             only); then / count as f32, then normalized again
//
// One workgroup of 256 threads per chunk:
//   1. the chunk's presence into LDS, with a rim of zeros (cells of other chunks own nothing here)
//   2. per cell its owned corners (a 4-bit mask) from the three or two neighbours before it
//   3. an exclusive scan over the cells in row-major order of (owned corners, present) packed into one word: DPP prefix sums inside a
//      wave, the four waves' totals through LDS, a running carry over the rounds of 256 cells (16 at the bound of 64 x 64)
//   4. one thread per cell writes its two triangles
//   5. one thread per corner writes its vertex and gathers its normal: the face normals of its up to six incident triangles are
//      computed again from the 3 x 3 corners around it and added in the order above -- no sum is split across lanes, no atomics
// A call is cut into launches of at most MESH_LAUNCH_CHUNKS chunks, whose coordinates travel as kernel arguments: nothing a queued
// launch reads can change under it except the resident heights and mask, which rxr_set_terrain_heights replaces only after rxr_quiesce.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>

#include "rxr_debug.h"
#include "rxr_query.h"
#include "rxr_exact_math.h"

#define MESH_WG 256u
#define MESH_LAUNCH_CHUNKS 256u   // chunk coordinates per launch (2 KiB of kernel arguments)

struct MeshArgs {
    const float *heights;    // [gh][gw], row-major
    const uint8_t *mask;     // the same grid: 1 = listed
    int32_t x0, y0;          // the grid's first cell
    uint32_t gw, gh;         // its size (0: nothing listed)
    float sx, sy;
    uint32_t cs;             // chunk_size, 1 .. RXR_TERRAIN_MESH_MAX_CHUNK_SIZE
    uint32_t *counts;        // [n][2], from this launch's first chunk on; so the three below
    float *vertices;         // [n][VS][4]
    uint32_t *indices;       // [n][TS][3]
    float *normals;          // [n][VS][3]
    int32_t coords[MESH_LAUNCH_CHUNKS][2];
};

namespace {

// LDS of a workgroup: info[cs * cs] words, own[cs * cs] bytes, pres[(cs + 2)^2] bytes, 4 words of wave totals
__host__ __device__ inline uint32_t mesh_lds_bytes(uint32_t cs) { return cs * cs * 4u + (cs * cs + (cs + 2u) * (cs + 2u) + 3u) / 4u * 4u + 16u; }

struct V3 {
    float x, y, z;
};
__device__ __forceinline__ V3 sub(V3 a, V3 b) { return V3{a.x - b.x, a.y - b.y, a.z - b.z}; }
// vek's cross, then `normalized` (dot left to right, sqrt, three divisions)
__device__ __forceinline__ V3 face_normal(V3 p0, V3 p1, V3 p2) {
    const V3 a = sub(p1, p0), b = sub(p2, p0);
    const float cx = a.y * b.z - a.z * b.y, cy = a.z * b.x - a.x * b.z, cz = a.x * b.y - a.y * b.x;
    V3 n;
    float mag;
    rxm::normalize3(cx, cy, cz, n.x, n.y, n.z, mag);
    return n;
}

struct MeshLds {
    uint32_t *info;   // per cell: vertices owned by the cells before it | present cells before it << 16
    uint8_t *own;     // per cell: bit k = it owns its corner k of (0,0), (1,0), (0,1), (1,1); 0 for an absent cell
    uint8_t *pres;    // [(cs + 2)][(cs + 2)]: cell (x, y) at (y + 1) * (cs + 2) + x + 1
    uint32_t *wave_total;
    uint32_t cs;
    __device__ __forceinline__ uint32_t present(int32_t x, int32_t y) const { return pres[(uint32_t)(y + 1) * (cs + 2u) + (uint32_t)(x + 1)]; }
    // the vertex index of corner (px, py), which has an owner
    __device__ __forceinline__ uint32_t vertex_of(int32_t px, int32_t py) const {
        int32_t ox = px, oy = py;
        uint32_t k = 0;   // the corner's number in its owner
        if (present(px - 1, py - 1)) ox = px - 1, oy = py - 1, k = 3;
        else if (present(px, py - 1)) oy = py - 1, k = 2;
        else if (present(px - 1, py)) ox = px - 1, k = 1;
        const uint32_t cell = (uint32_t)oy * cs + (uint32_t)ox;
        return (info[cell] & 0xFFFFu) + (uint32_t)__builtin_popcount(own[cell] & ((1u << k) - 1u));
    }
};

}  // namespace

extern "C" __global__ __launch_bounds__(MESH_WG) void k_terrain_mesh(MeshArgs A) {
    extern __shared__ uint32_t lds[];
    const uint32_t cs = A.cs, n_cells = cs * cs, side = cs + 2u, tid = threadIdx.x, chunk = blockIdx.x;
    MeshLds L;
    L.info = lds;
    L.own = (uint8_t *)(lds + n_cells);
    L.pres = L.own + n_cells;
    L.wave_total = lds + (mesh_lds_bytes(cs) - 16u) / 4u;
    L.cs = cs;
    // (the host checked that every cell of the chunk lies within +-2^30)
    const int32_t wx0 = A.coords[chunk][0] * (int32_t)cs, wy0 = A.coords[chunk][1] * (int32_t)cs;
    auto in_grid = [&](int32_t x, int32_t y, size_t &at) {
        const uint32_t gx = (uint32_t)x - (uint32_t)A.x0, gy = (uint32_t)y - (uint32_t)A.y0;
        at = (size_t)gy * A.gw + gx;
        return gx < A.gw && gy < A.gh;
    };

    // 1. presence
    for (uint32_t j = tid; j < side * side; j += MESH_WG) {
        const uint32_t lx = j % side - 1u, ly = j / side - 1u;   // (the rim wraps to 0xFFFFFFFF)
        size_t at;
        L.pres[j] = (lx < cs && ly < cs && in_grid(wx0 + (int32_t)lx, wy0 + (int32_t)ly, at)) ? A.mask[at] : 0;
    }
    __syncthreads();

    // 2. and 3.: owned corners per cell, scanned in row-major order
    uint32_t carry = 0;   // the same in every thread
    for (uint32_t c0 = 0; c0 < n_cells; c0 += MESH_WG) {
        const uint32_t cell = c0 + tid;
        const int32_t x = (int32_t)(cell % cs), y = (int32_t)(cell / cs);
        uint32_t own = 0;
        if (cell < n_cells && L.present(x, y)) {
            own = 8u;                                                                       // (1,1): no cell comes before this one
            if (!L.present(x - 1, y)) own |= 4u;                                            // (0,1)
            if (!L.present(x, y - 1) && !L.present(x + 1, y - 1)) own |= 2u;                // (1,0)
            if (!L.present(x - 1, y - 1) && !L.present(x, y - 1) && !L.present(x - 1, y)) own |= 1u;   // (0,0)
        }
        const uint32_t v = (uint32_t)__builtin_popcount(own) | (own ? 1u << 16 : 0u);       // (at most 4225 vertices: the halves never meet)
        const uint32_t inclusive = rxm::wave_inclusive_add(v);
        if ((tid & 63u) == 63u) L.wave_total[tid >> 6] = inclusive;
        __syncthreads();
        uint32_t before = carry, round = 0;
        for (uint32_t w = 0; w < MESH_WG / 64u; ++w) {
            const uint32_t t = L.wave_total[w];
            if (w < (tid >> 6)) before += t;
            round += t;
        }
        if (cell < n_cells) {
            L.info[cell] = before + inclusive - v;
            L.own[cell] = (uint8_t)own;
        }
        carry += round;
        __syncthreads();   // (the totals are rewritten by the next round; info and own are read below)
    }
    const uint32_t n_vertices = carry & 0xFFFFu, n_present = carry >> 16;
    const size_t VS = (size_t)(cs + 1u) * (cs + 1u), TS = 2u * (size_t)n_cells;
    if (tid == 0) {
        A.counts[2 * (size_t)chunk] = n_vertices;
        A.counts[2 * (size_t)chunk + 1] = 2u * n_present;
    }

    // 4. triangles
    uint32_t *idx = A.indices + (size_t)chunk * TS * 3;
    for (uint32_t cell = tid; cell < n_cells; cell += MESH_WG) {
        if (!L.own[cell]) continue;
        const int32_t x = (int32_t)(cell % cs), y = (int32_t)(cell / cs);
        const uint32_t i0 = L.vertex_of(x, y), i1 = L.vertex_of(x + 1, y), i2 = L.vertex_of(x, y + 1), i3 = L.vertex_of(x + 1, y + 1);
        uint32_t *t = idx + 6 * (size_t)(L.info[cell] >> 16);
        t[0] = i0, t[1] = i2, t[2] = i1;
        t[3] = i1, t[4] = i2, t[5] = i3;
    }

    // 5. vertices and normals
    float *vtx = A.vertices + (size_t)chunk * VS * 4, *nrm = A.normals + (size_t)chunk * VS * 3;
    for (uint32_t c = tid; c < (uint32_t)VS; c += MESH_WG) {
        const int32_t px = (int32_t)(c % (cs + 1u)), py = (int32_t)(c / (cs + 1u));
        const bool pa = L.present(px - 1, py - 1), pb = L.present(px, py - 1), pc = L.present(px - 1, py), pd = L.present(px, py);
        if (!(pa || pb || pc || pd)) continue;
        // the 3 x 3 corners around this one: P[j][i] is corner (px - 1 + i, py - 1 + j)
        V3 P[3][3];
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const int32_t X = wx0 + px - 1 + i, Y = wy0 + py - 1 + j;
                size_t at;
                const float h = in_grid(X, Y, at) ? A.heights[at] : 0.0f;   // Terrain::get_height
                P[j][i] = V3{(float)X * A.sx, h, (float)Y * A.sy};
            }
        V3 sum{0.0f, 0.0f, 0.0f};
        uint32_t count = 0;
        auto add = [&](V3 n) {
            sum.x = sum.x + n.x;
            sum.y = sum.y + n.y;
            sum.z = sum.z + n.z;
            ++count;
        };
        // a cell whose (0,0) corner is P[j][i]: triangle 0 = (i0, i2, i1), triangle 1 = (i1, i2, i3)
#define TRI0(j, i) face_normal(P[j][i], P[j + 1][i], P[j][i + 1])
#define TRI1(j, i) face_normal(P[j][i + 1], P[j + 1][i], P[j + 1][i + 1])
        if (pa) add(TRI1(0, 0));
        if (pb) {
            add(TRI0(0, 1));
            add(TRI1(0, 1));
        }
        if (pc) {
            add(TRI0(1, 0));
            add(TRI1(1, 0));
        }
        if (pd) add(TRI0(1, 1));
#undef TRI0
#undef TRI1
        V3 mean, n;
        float mag;
        rxm::div3(sum.x, sum.y, sum.z, (float)count, mean.x, mean.y, mean.z);
        rxm::normalize3(mean.x, mean.y, mean.z, n.x, n.y, n.z, mag);
        const uint32_t v = L.vertex_of(px, py);
        float *o = vtx + 4 * (size_t)v;
        o[0] = P[1][1].x, o[1] = P[1][1].y, o[2] = P[1][1].z, o[3] = 1.0f;
        float *q = nrm + 3 * (size_t)v;
        q[0] = n.x, q[1] = n.y, q[2] = n.z;
    }
}

namespace {

// what both entry points refuse, but for their pointers
int mesh_check(rxr_ctx *ctx, const char *who, const int32_t *coords, uint32_t n, int32_t cs) {
    const std::string w = who;
    if (!ctx->heights_set) return rxr_fail(ctx, RXR_ERR_INVALID, w + ": no terrain heights are resident (rxr_set_terrain_heights)");
    if (cs < 1) return rxr_fail(ctx, RXR_ERR_INVALID, w + ": chunk_size must be at least 1");
    if (cs > RXR_TERRAIN_MESH_MAX_CHUNK_SIZE)
        return rxr_fail(ctx, RXR_ERR_UNSUPPORTED, w + ": chunk_size " + std::to_string(cs) + " exceeds RXR_TERRAIN_MESH_MAX_CHUNK_SIZE");
    if (n && !coords) return rxr_fail(ctx, RXR_ERR_INVALID, w + ": NULL chunk_coords");
    for (uint32_t i = 0; i < n; ++i)
        for (int a = 0; a < 2; ++a) {
            const int64_t lo = (int64_t)coords[2 * (size_t)i + a] * cs;
            if (lo < -(1ll << 30) || lo + cs - 1 > (1ll << 30))
                return rxr_fail(ctx, RXR_ERR_INVALID, w + ": chunk " + std::to_string(i) + " (" + std::to_string(coords[2 * (size_t)i]) + ", " +
                                                          std::to_string(coords[2 * (size_t)i + 1]) + "): its cells leave +-2^30");
        }
    return RXR_OK;
}

// the four arrays' sizes in bytes; false if one does not fit a size_t
bool mesh_bytes(uint32_t n, int32_t cs, size_t bytes[4]) {
    const size_t VS = (size_t)(cs + 1) * (size_t)(cs + 1), TS = 2 * (size_t)cs * (size_t)cs;
    const size_t per[4] = {8, VS * 16, TS * 12, VS * 12};
    for (int i = 0; i < 4; ++i)
        if (__builtin_mul_overflow((size_t)n, per[i], &bytes[i])) return false;
    return true;
}

// every chunk of a call into device arrays, queued on `s`
int mesh_run(rxr_ctx *ctx, const int32_t *coords, uint32_t n, int32_t cs, uint32_t *counts, float *vertices, uint32_t *indices, float *normals, hipStream_t s) {
    MeshArgs A{};
    // (rxr_set_terrain_height_source: the processed grid and mask lie over the same rectangle; rxr_flatten_terrain_to writes them in stream order)
    const bool processed = ctx->height_source == RXR_TERRAIN_HEIGHTS_PROCESSED;
    A.heights = (const float *)(processed ? ctx->d_pheights.p : ctx->d_heights.p);
    A.mask = (const uint8_t *)(processed ? ctx->d_pheights_mask.p : ctx->d_heights_mask.p);
    A.x0 = ctx->heights_x0;
    A.y0 = ctx->heights_y0;
    A.gw = ctx->heights_gw;
    A.gh = ctx->heights_gh;
    A.sx = ctx->heights_scale[0];
    A.sy = ctx->heights_scale[1];
    A.cs = (uint32_t)cs;
    const size_t VS = (size_t)(cs + 1) * (size_t)(cs + 1), TS = 2 * (size_t)cs * (size_t)cs;
    int rc = rxr_query_begin(ctx, ctx->lane[Q_MESH], s);
    if (rc != RXR_OK || (processed && (rc = rxr_query_begin(ctx, ctx->lane[Q_FLATTEN], s)) != RXR_OK)) return rc;
    ctx->mesh_launches = 0;
    for (uint32_t c0 = 0; c0 < n; c0 += MESH_LAUNCH_CHUNKS) {
        const uint32_t nc = std::min(n - c0, MESH_LAUNCH_CHUNKS);
        memcpy(A.coords, coords + 2 * (size_t)c0, (size_t)nc * 2 * sizeof(int32_t));
        A.counts = counts + 2 * (size_t)c0;
        A.vertices = vertices + (size_t)c0 * VS * 4;
        A.indices = indices + (size_t)c0 * TS * 3;
        A.normals = normals + (size_t)c0 * VS * 3;
        hipLaunchKernelGGL(k_terrain_mesh, dim3(nc), dim3(MESH_WG), mesh_lds_bytes(A.cs), s, A);
        HIPCHK(ctx, hipGetLastError());
        ++ctx->mesh_launches;
    }
    return rxr_query_end(ctx, ctx->lane[Q_MESH], s);
}

}  // namespace

extern "C" {

int rxr_terrain_meshes(rxr_ctx *ctx, const int32_t *chunk_coords, uint32_t n, int32_t chunk_size, uint32_t *counts, float *vertices, uint32_t *indices,
                       float *normals) {
    if (!ctx) return RXR_ERR_INVALID;
    if (ctx->group) return rxr_as_member0(ctx, [&](rxr_ctx *m) { return rxr_terrain_meshes(m, chunk_coords, n, chunk_size, counts, vertices, indices, normals); });
    int rc = mesh_check(ctx, "rxr_terrain_meshes", chunk_coords, n, chunk_size);
    if (rc != RXR_OK) return rc;
    if (!n) return RXR_OK;
    if (!counts || !vertices || !indices || !normals) return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_terrain_meshes: NULL output array");
    size_t bytes[4];
    if (!mesh_bytes(n, chunk_size, bytes)) return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_terrain_meshes: the output arrays' sizes overflow");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // the three geometry arrays go up as well as down: the slots past a chunk's counts come back as the caller left them
    QueryIO io{ctx, ctx->lane[Q_MESH]};
    const unsigned i_c = io.out(counts, bytes[0]), i_v = io.inout(vertices, bytes[1]), i_i = io.inout(indices, bytes[2]), i_n = io.inout(normals, bytes[3]);
    if ((rc = io.upload()) != RXR_OK) return rc;
    if ((rc = mesh_run(ctx, chunk_coords, n, chunk_size, io.dev<uint32_t>(i_c), io.dev<float>(i_v), io.dev<uint32_t>(i_i), io.dev<float>(i_n), ctx->stream)) != RXR_OK)
        return rc;
    return io.download();
}

int rxr_terrain_meshes_to(rxr_ctx *ctx, const int32_t *chunk_coords, uint32_t n, int32_t chunk_size, uint32_t *dev_counts, float *dev_vertices,
                          uint32_t *dev_indices, float *dev_normals, void *hip_stream) {
    if (!ctx) return RXR_ERR_INVALID;
    if (ctx->group) return rxr_fail(ctx, RXR_ERR_UNSUPPORTED, "rxr_terrain_meshes_to on a multi-device context: device pointers and streams belong to ONE device (use rxr_member)");
    const int rc = mesh_check(ctx, "rxr_terrain_meshes_to", chunk_coords, n, chunk_size);
    if (rc != RXR_OK) return rc;
    if (!n) return RXR_OK;
    size_t bytes[4];
    if (!mesh_bytes(n, chunk_size, bytes)) return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_terrain_meshes_to: the output arrays' sizes overflow");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const struct {
        const void *p;
        const char *name;
    } arrays[4] = {{dev_counts, "dev_counts"}, {dev_vertices, "dev_vertices"}, {dev_indices, "dev_indices"}, {dev_normals, "dev_normals"}};
    for (int i = 0; i < 4; ++i) {
        if (!arrays[i].p || ((uintptr_t)arrays[i].p & 3u))
            return rxr_fail(ctx, RXR_ERR_INVALID, std::string("rxr_terrain_meshes_to: ") + arrays[i].name + " must be 4-byte aligned device memory");
        if (!rxr_on_device(ctx, arrays[i].p, bytes[i]))
            return rxr_fail(ctx, RXR_ERR_INVALID, std::string("rxr_terrain_meshes_to: ") + arrays[i].name + " is not device memory of the context's device (or is too small)");
    }
    return mesh_run(ctx, chunk_coords, n, chunk_size, dev_counts, dev_vertices, dev_indices, dev_normals, hip_stream ? (hipStream_t)hip_stream : ctx->stream);
}

// test-only: the k_terrain_mesh launches of the last mesh call
uint32_t rxr_debug_terrain_mesh_launches(rxr_ctx *ctx) {
    if (!ctx) return 0;
    if (ctx->group) return rxr_debug_terrain_mesh_launches(rxr_member(ctx, 0));
    return ctx->mesh_launches;
}

}  // extern "C"
