// rxr_normals.hip -- smooth vertex normals of meshes that live in device memory: Batch3D::compute_vertex_normals
// (src/batch/batch3d.rs:771-809).  include/rxr.h: rxr_check_vertex_normals, rxr_vertex_normals, rxr_vertex_normals_to; DESIGN.md
// section 20.
//
// Semantics, all f32, one operation per reference operation in its order, nothing fused (the build's -ffp-contract=off):
//   face      normalized(cross(p1 - p0, p2 - p0)) per triangle: vek's cross, then the dot product left to right, a square root and three
//             divisions, all correctly rounded (rxm::normalize3).  A degenerate triangle is 0 / 0 = NaN in all three components.
//   sum       per vertex from +0.0 (NOT from the first normal: +0.0 + -0.0 = +0.0), the face normals of the triangles that name it in
//             ASCENDING TRIANGLE INDEX, once per naming (a triangle (a, a, b) adds twice to a and counts twice)
//   finish    count > 0: sum / (count as f32), normalized again; count == 0: (+0.0, +0.0, +0.0)
// Float addition is not associative, so the order is the whole difficulty: no sum is split across lanes and nothing is added with
// atomics.  Two routes, chosen per call from the strides (which the host knows; the counts are device memory in the _to form):
//   small     triangle_stride <= the bound (NRM_SMALL_MAX, or RXR_VERTEX_NORMALS_SMALL_MAX in the environment): one workgroup per
//             mesh.  The mesh's indices and its face normals (computed once per triangle) go into LDS, 24 bytes a triangle; then one
//             thread per vertex walks the triangles in ascending index and adds on a match.  Every lane reads the same LDS word at the
//             same time: a broadcast.  No scratch, no sort.
//   general   k_nrm_faces: a thread per triangle slot writes the face normal to scratch and the slot's three corners as pairs
//             (key = mesh slot * vertex_stride + vertex, value = triangle slot); a refused triangle and a slot past its mesh's count
//             get the largest key.  One stable rocprim::radix_sort_pairs over the bits in use: the pairs go in triangle-major, so
//             within a key the triangles stay ascending.  k_nrm_gather: a thread per vertex finds its segment by binary search and
//             adds it sequentially.  A fan apex of a million triangles is one thread's million additions: slow, bounded, and
//             independent of scheduling.
// Both routes cut a call into launches of at most NRM_LAUNCH_SLOTS triangle (and vertex) slots, at least one mesh
// (RXR_VERTEX_NORMALS_LAUNCH_SLOTS overrides it).  What the device form cannot refuse it must not read: a mesh whose counts exceed the
// strides is skipped whole, a triangle with an index at or above its mesh's vertex count contributes to no vertex.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>
#include <cstring>
#include <string>

#include "rxr_debug.h"
#include "rxr_query.h"
#include "rxr_exact_math.h"

#define NRM_WG 256u
#define NRM_SMALL_WG 1024u   // the small route: sixteen waves share one mesh's LDS; two such workgroups fill a CU
// The small route's bound on triangle_stride.  It started at 3413 (24 bytes a triangle, two workgroups in a CU's 160 KiB); the
// crossover sweep of tools/vertex_normals_bench.py (profiles/vertex_normals/README.md, crossover_n64_*) put the two routes level
// at 1 024 triangles a mesh with 64 meshes in the call (89.2 against 88.9 us) and at 1 536, and the general route ahead from 2 048
// on; the 1 024 terrain chunks of 512 triangles win by 1.7x on this side of it.  A lone mesh is already faster through the general route from
// 256 triangles on (35.5 against 22.9 us): the bound is set by calls of many meshes, which are what the route is for.
#define NRM_SMALL_MAX 1024u
#define NRM_SMALL_CAP 6825u          // what one workgroup can hold at all: 160 KiB less the counter and its padding, / 24 (an override is cut to it)
#define NRM_LAUNCH_SLOTS (1u << 20)  // triangle slots (and vertex slots) per launch; a mesh larger than this is a launch of its own

struct NrmArgs {
    const uint32_t *counts;    // [n][2], from this launch's first mesh on; so the four below
    const float *vertices;     // [n][VS][4]
    const uint32_t *indices;   // [n][TS][3]
    float *normals;            // [n][VS][3]
    uint32_t *refused;         // [n] or null
    uint32_t n, VS, TS;
    // the general route's scratch
    float *face;               // [n * TS][3]
    unsigned long long *keys;  // [3 * n * TS], triangle-major (k_nrm_faces writes, k_nrm_gather reads the sorted ones)
    uint32_t *vals;            // [3 * n * TS]
};

namespace {

struct V3 {
    float x, y, z;
};
__device__ __forceinline__ V3 load_xyz(const float *vertices, size_t v) { return V3{vertices[4 * v], vertices[4 * v + 1], vertices[4 * v + 2]}; }
// vek's cross, then `normalized` (dot left to right, sqrt, three divisions): face_normal of rxr_terrain_mesh.hip
__device__ __forceinline__ V3 face_normal(V3 p0, V3 p1, V3 p2) {
    const V3 a{p1.x - p0.x, p1.y - p0.y, p1.z - p0.z}, b{p2.x - p0.x, p2.y - p0.y, p2.z - p0.z};
    const float cx = a.y * b.z - a.z * b.y, cy = a.z * b.x - a.x * b.z, cz = a.x * b.y - a.y * b.x;
    V3 n;
    float mag;
    rxm::normalize3(cx, cy, cz, n.x, n.y, n.z, mag);
    return n;
}
// sum / (count as f32), normalized again; (+0.0, +0.0, +0.0) for a vertex no triangle names
__device__ __forceinline__ V3 finish(V3 sum, uint32_t count) {
    if (!count) return V3{0.0f, 0.0f, 0.0f};
    V3 mean, n;
    float mag;
    rxm::div3(sum.x, sum.y, sum.z, (float)count, mean.x, mean.y, mean.z);
    rxm::normalize3(mean.x, mean.y, mean.z, n.x, n.y, n.z, mag);
    return n;
}

}  // namespace

// the small route: LDS = idx[3 * TS] words, then face[3 * TS] floats (only the mesh's first `nt` triangles are filled and read)
extern "C" __global__ __launch_bounds__(NRM_SMALL_WG) void k_nrm_small(NrmArgs A) {
    extern __shared__ __align__(16) uint32_t lds[];
    __shared__ uint32_t n_refused;
    const uint32_t tid = threadIdx.x;
    const size_t m = blockIdx.x;
    const uint32_t nv = A.counts[2 * m], nt = A.counts[2 * m + 1];
    if (nv > A.VS || nt > A.TS) {   // (the same in every thread)
        if (tid == 0 && A.refused) A.refused[m] = 0xFFFFFFFFu;
        return;
    }
    uint32_t *idx = lds;
    float *face = (float *)(lds + 3 * (size_t)A.TS);
    const float *vtx = A.vertices + m * A.VS * 4;
    const uint32_t *tri = A.indices + m * A.TS * 3;
    if (tid == 0) n_refused = 0;
    __syncthreads();
    for (uint32_t t = tid; t < nt; t += NRM_SMALL_WG) {
        uint32_t i0 = tri[3 * (size_t)t], i1 = tri[3 * (size_t)t + 1], i2 = tri[3 * (size_t)t + 2];
        if (i0 >= nv || i1 >= nv || i2 >= nv) {
            atomicAdd(&n_refused, 1u);           // (a count of integers: the order does not show)
            i0 = i1 = i2 = 0xFFFFFFFFu;          // no vertex: nv <= VS <= 0xFFFFFFFF, a vertex index is below it
        } else {
            const V3 n = face_normal(load_xyz(vtx, i0), load_xyz(vtx, i1), load_xyz(vtx, i2));
            face[3 * t] = n.x, face[3 * t + 1] = n.y, face[3 * t + 2] = n.z;
        }
        idx[3 * t] = i0, idx[3 * t + 1] = i1, idx[3 * t + 2] = i2;
    }
    __syncthreads();
    float *out = A.normals + m * A.VS * 3;
    for (uint32_t v = tid; v < nv; v += NRM_SMALL_WG) {
        V3 sum{0.0f, 0.0f, 0.0f};
        uint32_t count = 0;
        auto add = [&](uint32_t t, uint32_t hits) {   // triangle t names this vertex `hits` times
            const V3 n{face[3 * t], face[3 * t + 1], face[3 * t + 2]};
            for (uint32_t k = 0; k < hits; ++k) {
                sum.x = sum.x + n.x;
                sum.y = sum.y + n.y;
                sum.z = sum.z + n.z;
            }
            count += hits;
        };
        // eight triangles a round: their 24 index words in six 16-byte reads that do not wait for each other, one test for "none of
        // them names this vertex" (the usual case: a vertex has a handful of triangles), and only then the triangles one by one
        uint32_t t = 0;
        const uint4 *idx4 = (const uint4 *)idx;
        for (; t + 8 <= nt; t += 8) {
            uint4 q[6];
#pragma unroll
            for (int k = 0; k < 6; ++k) q[k] = idx4[3 * (t >> 2) + k];
            uint32_t mask = 0;   // bit j: word j of the 24 is this vertex
#pragma unroll
            for (int k = 0; k < 6; ++k)
                mask |= ((uint32_t)(q[k].x == v) | (uint32_t)(q[k].y == v) << 1 | (uint32_t)(q[k].z == v) << 2 | (uint32_t)(q[k].w == v) << 3) << (4 * k);
            if (!mask) continue;
            for (uint32_t j = 0; j < 8; ++j) {
                const uint32_t hits = (uint32_t)__builtin_popcount((mask >> (3 * j)) & 7u);
                if (hits) add(t + j, hits);
            }
        }
        for (; t < nt; ++t) {
            const uint32_t hits = (idx[3 * t] == v) + (idx[3 * t + 1] == v) + (idx[3 * t + 2] == v);
            if (hits) add(t, hits);
        }
        const V3 n = finish(sum, count);
        out[3 * (size_t)v] = n.x, out[3 * (size_t)v + 1] = n.y, out[3 * (size_t)v + 2] = n.z;
    }
    if (tid == 0 && A.refused) A.refused[m] = n_refused;
}

// the general route, 1: dev_refused starts at 0, or at 0xFFFFFFFF for a mesh that is skipped
extern "C" __global__ __launch_bounds__(NRM_WG) void k_nrm_begin(NrmArgs A) {
    const uint32_t m = blockIdx.x * NRM_WG + threadIdx.x;
    if (m >= A.n) return;
    A.refused[m] = (A.counts[2 * (size_t)m] > A.VS || A.counts[2 * (size_t)m + 1] > A.TS) ? 0xFFFFFFFFu : 0u;
}

// 2: a thread per triangle slot g = mesh slot * TS + t
extern "C" __global__ __launch_bounds__(NRM_WG) void k_nrm_faces(NrmArgs A) {
    const unsigned long long g = (unsigned long long)blockIdx.x * NRM_WG + threadIdx.x;
    if (g >= (unsigned long long)A.n * A.TS) return;
    const size_t m = (size_t)(g / A.TS);
    const uint32_t t = (uint32_t)(g % A.TS);
    const uint32_t nv = A.counts[2 * m], nt = A.counts[2 * m + 1];
    const unsigned long long none = (unsigned long long)A.n * A.VS;   // above every vertex's key
    unsigned long long k0 = none, k1 = none, k2 = none;
    if (nv <= A.VS && nt <= A.TS && t < nt) {
        const uint32_t *tri = A.indices + 3 * (size_t)g;
        const uint32_t i0 = tri[0], i1 = tri[1], i2 = tri[2];
        if (i0 >= nv || i1 >= nv || i2 >= nv) {
            if (A.refused) atomicAdd(A.refused + m, 1u);   // (a count of integers: the order does not show)
        } else {
            const float *vtx = A.vertices + m * A.VS * 4;
            const V3 n = face_normal(load_xyz(vtx, i0), load_xyz(vtx, i1), load_xyz(vtx, i2));
            float *f = A.face + 3 * (size_t)g;
            f[0] = n.x, f[1] = n.y, f[2] = n.z;
            const unsigned long long base = (unsigned long long)m * A.VS;
            k0 = base + i0, k1 = base + i1, k2 = base + i2;
        }
    }
    unsigned long long *k = A.keys + 3 * (size_t)g;
    uint32_t *v = A.vals + 3 * (size_t)g;
    k[0] = k0, k[1] = k1, k[2] = k2;
    v[0] = v[1] = v[2] = (uint32_t)g;
}

// 3 (behind the sort): a thread per vertex slot; keys / vals are the sorted pairs
extern "C" __global__ __launch_bounds__(NRM_WG) void k_nrm_gather(NrmArgs A) {
    const unsigned long long key = (unsigned long long)blockIdx.x * NRM_WG + threadIdx.x;
    if (key >= (unsigned long long)A.n * A.VS) return;
    const size_t m = (size_t)(key / A.VS);
    const uint32_t v = (uint32_t)(key % A.VS);
    const uint32_t nv = A.counts[2 * m], nt = A.counts[2 * m + 1];
    if (nv > A.VS || nt > A.TS || v >= nv) return;
    const size_t n_pairs = 3 * (size_t)A.n * A.TS, n_faces = (size_t)A.n * A.TS;
    size_t lo = 0, hi = n_pairs;   // the first pair whose key is not below this vertex's
    while (lo < hi) {
        const size_t mid = lo + (hi - lo) / 2;
        if (A.keys[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    V3 sum{0.0f, 0.0f, 0.0f};
    uint32_t count = 0;
    for (size_t j = lo; j < n_pairs && A.keys[j] == key; ++j) {
        const size_t g = A.vals[j];
        if (g >= n_faces) break;   // (a sort that went wrong must not read out of bounds)
        const float *f = A.face + 3 * g;
        sum.x = sum.x + f[0];
        sum.y = sum.y + f[1];
        sum.z = sum.z + f[2];
        ++count;
    }
    const V3 n = finish(sum, count);
    float *out = A.normals + 3 * (size_t)key;
    out[0] = n.x, out[1] = n.y, out[2] = n.z;
}

namespace {

// the four arrays' sizes in bytes and dev_refused's; false if one does not fit a size_t
bool nrm_bytes(uint32_t n, uint32_t VS, uint32_t TS, size_t bytes[5]) {
    const size_t per[5] = {8, (size_t)VS * 16, (size_t)TS * 12, (size_t)VS * 12, 4};
    for (int i = 0; i < 5; ++i)
        if (__builtin_mul_overflow((size_t)n, per[i], &bytes[i])) return false;
    size_t pairs;   // (the general route's corner pairs are counted in a size_t as well)
    return !__builtin_mul_overflow(bytes[2], (size_t)2, &pairs);
}

// what the host form refuses in its counts and indices: the first offending mesh and why
int nrm_check(const uint32_t *counts, const uint32_t *indices, uint32_t n, uint32_t VS, uint32_t TS, std::string &err) {
    size_t bytes[5];
    if (!nrm_bytes(n, VS, TS, bytes)) {
        err = "the arrays' byte sizes overflow";
        return RXR_ERR_INVALID;
    }
    if (!n) return RXR_OK;
    if (!counts) {
        err = "NULL counts";
        return RXR_ERR_INVALID;
    }
    if (TS && !indices) {
        err = "NULL indices";
        return RXR_ERR_INVALID;
    }
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t nv = counts[2 * (size_t)i], nt = counts[2 * (size_t)i + 1];
        if (nv > VS) {
            err = "mesh " + std::to_string(i) + ": its " + std::to_string(nv) + " vertices exceed vertex_stride " + std::to_string(VS);
            return RXR_ERR_INVALID;
        }
        if (nt > TS) {
            err = "mesh " + std::to_string(i) + ": its " + std::to_string(nt) + " triangles exceed triangle_stride " + std::to_string(TS);
            return RXR_ERR_INVALID;
        }
        const uint32_t *tri = indices + (size_t)i * TS * 3;
        for (size_t w = 0; w < 3 * (size_t)nt; ++w)
            if (tri[w] >= nv) {
                err = "mesh " + std::to_string(i) + ": triangle " + std::to_string(w / 3) + " has a vertex index " + std::to_string(tri[w]) +
                      " that is not below its " + std::to_string(nv) + " vertices";
                return RXR_ERR_INVALID;
            }
    }
    return RXR_OK;
}

uint32_t env_u32(const char *name, uint32_t fallback, bool zero_counts) {
    if (const char *e = getenv(name)) {
        char *end = nullptr;
        const unsigned long long v = strtoull(e, &end, 10);
        if (end != e && (v || zero_counts)) return (uint32_t)std::min<unsigned long long>(v, 0xFFFFFFFFull);
    }
    return fallback;
}

// every mesh of a call on device arrays, queued on `s`
int nrm_run(rxr_ctx *ctx, uint32_t n, const uint32_t *counts, const float *vertices, const uint32_t *indices, float *normals, uint32_t *refused,
            uint32_t VS, uint32_t TS, hipStream_t s) {
    const uint32_t small_max = std::min(env_u32("RXR_VERTEX_NORMALS_SMALL_MAX", NRM_SMALL_MAX, true), NRM_SMALL_CAP);
    const uint32_t slots = env_u32("RXR_VERTEX_NORMALS_LAUNCH_SLOTS", NRM_LAUNCH_SLOTS, false);
    const bool small = TS <= small_max;
    // meshes per launch: at most `slots` triangle slots and as many vertex slots, at least one mesh
    const uint32_t per_launch = std::max<uint32_t>(1u, std::min(slots / std::max(TS, 1u), slots / std::max(VS, 1u)));
    int rc = rxr_query_begin(ctx, ctx->lane[Q_NORMALS], s);
    if (rc != RXR_OK) return rc;
    ctx->nrm_route = small ? RXR_VERTEX_NORMALS_ROUTE_SMALL : RXR_VERTEX_NORMALS_ROUTE_GENERAL;
    ctx->nrm_launches = 0;
    NrmArgs A{};
    A.VS = VS;
    A.TS = TS;
    size_t sort_bytes = 0, o_face = 0, o_k0 = 0, o_k1 = 0, o_v0 = 0, o_v1 = 0, o_tmp = 0;
    unsigned end_bit = 1;
    if (small) {
        const size_t lds = (size_t)TS * 24;
        if (lds > 65536) HIPCHK(ctx, hipFuncSetAttribute((const void *)k_nrm_small, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(NRM_SMALL_CAP * 24u)));
    } else {
        // the largest round decides the scratch: rounds of per_launch meshes, and a last, smaller one
        const uint32_t nm = std::min(n, per_launch);
        const size_t faces = (size_t)nm * TS, pairs = 3 * faces;
        unsigned long long *knull = nullptr;
        uint32_t *vnull = nullptr;
        const unsigned long long top = (unsigned long long)nm * VS;   // the largest key
        end_bit = top ? 64u - (unsigned)__builtin_clzll(top) : 1u;
        HIPCHK(ctx, rocprim::radix_sort_pairs(nullptr, sort_bytes, knull, knull, vnull, vnull, pairs, 0u, end_bit, s));
        if (n % per_launch && n > per_launch) {   // (rocPRIM's scratch need not grow with the size)
            size_t last = 0;
            HIPCHK(ctx, rocprim::radix_sort_pairs(nullptr, last, knull, knull, vnull, vnull, 3 * (size_t)(n % per_launch) * TS, 0u, end_bit, s));
            sort_bytes = std::max(sort_bytes, last);
        }
        BlobCursor take;
        o_face = take(faces * 12), o_k0 = take(pairs * 8), o_k1 = take(pairs * 8), o_v0 = take(pairs * 4), o_v1 = take(pairs * 4), o_tmp = take(sort_bytes);
        if ((rc = rxr_ensure(ctx, ctx->d_nrm_scratch, take.o)) != RXR_OK) return rc;
    }
    uint8_t *sc = (uint8_t *)ctx->d_nrm_scratch.p;
    for (uint32_t m0 = 0; m0 < n; m0 += per_launch) {
        const uint32_t nm = std::min(n - m0, per_launch);
        A.n = nm;
        A.counts = counts + 2 * (size_t)m0;
        A.vertices = vertices + (size_t)m0 * VS * 4;
        A.indices = indices + (size_t)m0 * TS * 3;
        A.normals = normals + (size_t)m0 * VS * 3;
        A.refused = refused ? refused + m0 : nullptr;
        if (small) {
            hipLaunchKernelGGL(k_nrm_small, dim3(nm), dim3(NRM_SMALL_WG), (size_t)TS * 24, s, A);
            HIPCHK(ctx, hipGetLastError());
        } else {
            const size_t faces = (size_t)nm * TS, pairs = 3 * faces, verts = (size_t)nm * VS;
            A.face = (float *)(sc + o_face);
            A.keys = (unsigned long long *)(sc + o_k0);
            A.vals = (uint32_t *)(sc + o_v0);
            if (refused) {
                hipLaunchKernelGGL(k_nrm_begin, dim3((nm + NRM_WG - 1) / NRM_WG), dim3(NRM_WG), 0, s, A);
                HIPCHK(ctx, hipGetLastError());
            }
            if (faces) {
                hipLaunchKernelGGL(k_nrm_faces, dim3((uint32_t)((faces + NRM_WG - 1) / NRM_WG)), dim3(NRM_WG), 0, s, A);
                HIPCHK(ctx, hipGetLastError());
                const unsigned long long top = (unsigned long long)nm * VS;
                const unsigned bits = top ? 64u - (unsigned)__builtin_clzll(top) : 1u;   // (a last, smaller round may use fewer)
                HIPCHK(ctx, rocprim::radix_sort_pairs(sc + o_tmp, sort_bytes, A.keys, (unsigned long long *)(sc + o_k1), A.vals, (uint32_t *)(sc + o_v1), pairs, 0u,
                                                      std::min(bits, end_bit), s));
                A.keys = (unsigned long long *)(sc + o_k1);
                A.vals = (uint32_t *)(sc + o_v1);
            }
            if (verts) {   // (without a triangle slot every vertex is unused: no pair is read)
                hipLaunchKernelGGL(k_nrm_gather, dim3((uint32_t)((verts + NRM_WG - 1) / NRM_WG)), dim3(NRM_WG), 0, s, A);
                HIPCHK(ctx, hipGetLastError());
            }
        }
        ++ctx->nrm_launches;
    }
    return rxr_query_end(ctx, ctx->lane[Q_NORMALS], s);
}

}  // namespace

extern "C" {

int rxr_check_vertex_normals(const uint32_t *counts, const uint32_t *indices, uint32_t n, uint32_t vertex_stride, uint32_t triangle_stride, char *message,
                             uint32_t message_capacity) {
    std::string err;
    const int rc = nrm_check(counts, indices, n, vertex_stride, triangle_stride, err);
    rxr_copy_message(err, message, message_capacity);
    return rc;
}

int rxr_vertex_normals(rxr_ctx *ctx, uint32_t n, const uint32_t *counts, const float *vertices, const uint32_t *indices, float *normals, uint32_t vertex_stride,
                       uint32_t triangle_stride) {
    if (!ctx) return RXR_ERR_INVALID;
    if (ctx->group) return rxr_as_member0(ctx, [&](rxr_ctx *m) { return rxr_vertex_normals(m, n, counts, vertices, indices, normals, vertex_stride, triangle_stride); });
    std::string err;
    int rc = nrm_check(counts, indices, n, vertex_stride, triangle_stride, err);
    if (rc != RXR_OK) return rxr_fail(ctx, rc, "rxr_vertex_normals: " + err);
    if (!n) return RXR_OK;
    if (vertex_stride && (!vertices || !normals)) return rxr_fail(ctx, RXR_ERR_INVALID, std::string("rxr_vertex_normals: NULL ") + (vertices ? "normals" : "vertices"));
    size_t bytes[5];
    (void)nrm_bytes(n, vertex_stride, triangle_stride, bytes);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // the normals go up as well as down: the slots past a mesh's count come back as the caller left them
    QueryIO io{ctx, ctx->lane[Q_NORMALS]};
    const unsigned i_c = io.in(counts, bytes[0]), i_v = io.in(vertices, bytes[1]), i_i = io.in(indices, bytes[2]), i_n = io.inout(normals, bytes[3]);
    if ((rc = io.upload()) != RXR_OK) return rc;
    if ((rc = nrm_run(ctx, n, io.dev<uint32_t>(i_c), io.dev<float>(i_v), io.dev<uint32_t>(i_i), io.dev<float>(i_n), nullptr, vertex_stride, triangle_stride,
                      ctx->stream)) != RXR_OK)
        return rc;
    return io.download();
}

int rxr_vertex_normals_to(rxr_ctx *ctx, uint32_t n, const uint32_t *dev_counts, const float *dev_vertices, const uint32_t *dev_indices, float *dev_normals,
                          uint32_t *dev_refused, uint32_t vertex_stride, uint32_t triangle_stride, void *hip_stream) {
    if (!ctx) return RXR_ERR_INVALID;
    if (ctx->group) return rxr_fail(ctx, RXR_ERR_UNSUPPORTED, "rxr_vertex_normals_to on a multi-device context: device pointers and streams belong to ONE device (use rxr_member)");
    size_t bytes[5];
    if (!nrm_bytes(n, vertex_stride, triangle_stride, bytes)) return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_vertex_normals_to: the arrays' byte sizes overflow");
    if (!n) return RXR_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const struct {
        const void *p;
        const char *name;
        bool optional;
    } arrays[5] = {{dev_counts, "dev_counts", false}, {dev_vertices, "dev_vertices", false}, {dev_indices, "dev_indices", false}, {dev_normals, "dev_normals", false},
                   {dev_refused, "dev_refused", true}};
    for (int i = 0; i < 5; ++i) {
        if (!bytes[i] || (arrays[i].optional && !arrays[i].p)) continue;   // (an array of 0 bytes -- a stride of 0 -- is not looked at)
        if (!arrays[i].p || ((uintptr_t)arrays[i].p & 3u))
            return rxr_fail(ctx, RXR_ERR_INVALID, std::string("rxr_vertex_normals_to: ") + arrays[i].name + " must be 4-byte aligned device memory");
        if (!rxr_on_device(ctx, arrays[i].p, bytes[i]))
            return rxr_fail(ctx, RXR_ERR_INVALID, std::string("rxr_vertex_normals_to: ") + arrays[i].name + " is not device memory of the context's device (or is too small)");
    }
    return nrm_run(ctx, n, dev_counts, dev_vertices, dev_indices, dev_normals, dev_refused, vertex_stride, triangle_stride, hip_stream ? (hipStream_t)hip_stream : ctx->stream);
}

// test-only: the route of the last vertex-normals call (0: none yet) and, through `launches`, how many launches it made (small: k_nrm_small
// launches; general: rounds of faces, sort and gather)
uint32_t rxr_debug_vertex_normals(rxr_ctx *ctx, uint32_t *launches) {
    if (!ctx) return 0;
    if (ctx->group) return rxr_debug_vertex_normals(rxr_member(ctx, 0), launches);
    if (launches) *launches = ctx->nrm_launches;
    return ctx->nrm_route;
}

// test-only: the small route's bound as compiled (the environment's override is not applied) and what an override is cut to
void rxr_debug_vertex_normals_constants(uint32_t out[3]) {
    out[0] = NRM_SMALL_MAX;
    out[1] = NRM_SMALL_CAP;
    out[2] = NRM_LAUNCH_SLOTS;
}

}  // extern "C"
