// rxr_ray_accel.hip -- an opt-in tree of boxes over the resident triangles, built on the device, and the many-ray closest-hit
// kernel that walks it (include/rxr.h: rxr_set_ray_accel, rxr_ray_accel_info).  Both the picking path
// (rxr_intersect.hip) and the path tracer (rxr_trace.hip) reach it through rxr_isect_closest.
//
// What it must keep: a segment's result is the 64-bit minimum of (t's bits, global triangle index) over the triangles that mt_test
// (rxr_isect.h) accepts.  A minimum does not care in which order triangles are visited nor which rejected ones are skipped, so the
// tree has one duty: NEVER SKIP A TRIANGLE THAT mt_test WOULD ACCEPT.  mt_test is float32 Moeller-Trumbore: for thin triangles it
// accepts rays whose line misses the triangle's exact box by far, so the box test is padded by the conditioning of the triangles
// below a node (box_pass below; the constant comes from tests/ray_accel_ref.py, profiles/ray_accel/README.md).  Equality with the
// brute-force kernels is asserted by tests and that margin; it is not proven.
//
// Build (once per rxr_set_meshes / rxr_update_meshes, lazily, with the triangle records of isect_prepare):
//   k_accel_mesh_boxes   per mesh the box over the centroids of its tame triangles (atomics on order-preserving words)
//   k_accel_keys         per triangle (mesh << 32 | 30-bit Morton code of the centroid in its mesh's box; wild: 0xFFFFFFFF) and g
//   rocprim::radix_sort_pairs   stable: every mesh's triangles stay contiguous and in mesh order, so a segment [begin, end) of global
//                        triangle indices is the same range of sorted positions -- for the picking table and the tracer's alike
//   k_accel_records      the nine SoA record arrays in sorted order (the operations of k_isect_prep: the same bits) and perm[pos] = g
//   k_accel_leaves       a leaf per ACCEL_L consecutive positions: box over the pool's vertices, largest kappa, largest |coordinate|
//   k_accel_level        a node per ACCEL_W consecutive nodes of the level below, up to one root.  Implicit: no child pointers.
// A triangle is WILD -- its leaf and every ancestor get an infinite box and are always entered -- when a value of its record is not
// finite or its kappa = |e1| |e2| / |e1 x e2| is not finite or above ACCEL_KAPPA_CAP.
//
// Walk (k_accel_by_ray, a thread per ray): depth-first and stackless, the state is (level, index).  A passing node above the leaves
// descends to index * W; otherwise index + 1, and while that index is a multiple of W or the end of its level, up to
// (index - 1) / W + 1.  The position only moves forward, so the walk ends after at most `nodes` steps whatever the boxes hold.
// Leaves come in increasing position, hence in segment order: the segment's minimum is flushed when the position crosses its end.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>
#include <cmath>

#include "rxr_isect.h"
#include "rxr_query.h"

namespace {

using namespace isect;

constexpr uint32_t ACCEL_WG = 256;
constexpr uint32_t ACCEL_L = RXR_RAY_ACCEL_LEAF;     // positions per leaf
constexpr uint32_t ACCEL_W = RXR_RAY_ACCEL_WIDTH;    // nodes per parent
constexpr uint32_t ACCEL_MAX_LEVELS = 24;
constexpr float ACCEL_KAPPA_CAP = RXR_RAY_ACCEL_KAPPA_CAP;
// pad = ACCEL_C * eps32 * kappa * (max|o_i| + max|box coordinate|): 8 x the smallest constant that kept every accepted hit of the
// adversarial generator (tests/ray_accel_ref.py), rounded up to a power of two
constexpr float ACCEL_PAD_SCALE = RXR_RAY_ACCEL_C * 1.1920928955078125e-7f;

struct AccelSeg {   // IsectSeg of rxr_intersect.hip: RXR_ISECT_SEG_WORDS words
    uint32_t begin, end, mesh0, mesh1, rule, pid;
};
static_assert(sizeof(AccelSeg) == 4 * RXR_ISECT_SEG_WORDS, "segment layout");

struct AccelNode {   // 32 bytes
    float lo[3], kappa;
    float hi[3], maxabs;   // maxabs = +inf: a wild triangle below, always entered
};

struct AccelLevels {
    uint32_t n;                          // levels; level 0 = the leaves, level n - 1 = the root
    uint32_t off[ACCEL_MAX_LEVELS];      // first node of a level
    uint32_t cnt[ACCEL_MAX_LEVELS];
};

struct AccelBuild {
    uint32_t ntri, n_meshes, stride;
    const uint32_t *tin_prefix, *vin_prefix, *obj_idx;
    const float4 *obj_verts;
    uint32_t *box_lo, *box_hi;           // [n_meshes][3] order-preserving words each: the minimum, the maximum
    unsigned long long *keys;            // [ntri]
    uint32_t *vals;                      // [ntri]
    const uint32_t *perm;                // [ntri] sorted
    float *tris;                         // nine SoA arrays, sorted order
    AccelNode *nodes;
    unsigned long long *stats;           // [0] tests of the last counted call, [1] wild triangles
};

__device__ __forceinline__ bool finite3(F3 a) { return isfinite(a.x) && isfinite(a.y) && isfinite(a.z); }

// order-preserving map of a finite float onto unsigned words
__device__ __forceinline__ uint32_t f2ord(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ord2f(uint32_t o) { return __uint_as_float((o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o); }

struct TriInfo {
    F3 v0, v1, v2, e1, e2;
    float kappa;
    bool wild;
};
__device__ __forceinline__ TriInfo tri_info(const AccelBuild &B, uint32_t g) {
    const uint32_t m = last_le(B.tin_prefix, 0, B.n_meshes, g);
    const uint32_t vb = B.vin_prefix[m];
    const float4 a = B.obj_verts[vb + B.obj_idx[3ull * g]];
    const float4 b = B.obj_verts[vb + B.obj_idx[3ull * g + 1]];
    const float4 c = B.obj_verts[vb + B.obj_idx[3ull * g + 2]];
    TriInfo T;
    T.v0 = {a.x, a.y, a.z}, T.v1 = {b.x, b.y, b.z}, T.v2 = {c.x, c.y, c.z};
    T.e1 = sub3(T.v1, T.v0), T.e2 = sub3(T.v2, T.v0);
    const F3 n = cross3(T.e1, T.e2);
    T.kappa = (sqrtf(dot3(T.e1, T.e1)) * sqrtf(dot3(T.e2, T.e2))) / sqrtf(dot3(n, n));
    T.wild = !(finite3(T.v0) && finite3(T.e1) && finite3(T.e2)) || !(T.kappa <= ACCEL_KAPPA_CAP);   // (a NaN kappa is wild)
    return T;
}
__device__ __forceinline__ F3 centroid(const TriInfo &T) {
    return {(T.v0.x + T.v1.x + T.v2.x) / 3.0f, (T.v0.y + T.v1.y + T.v2.y) / 3.0f, (T.v0.z + T.v1.z + T.v2.z) / 3.0f};
}

__global__ __launch_bounds__(ACCEL_WG) void k_accel_mesh_boxes(AccelBuild B) {
    const uint32_t g = blockIdx.x * ACCEL_WG + threadIdx.x;
    if (g >= B.ntri) return;
    const TriInfo T = tri_info(B, g);
    const F3 c = centroid(T);
    if (T.wild || !finite3(c)) return;
    const uint32_t m = last_le(B.tin_prefix, 0, B.n_meshes, g);
    uint32_t *lo = B.box_lo + 3u * m, *hi = B.box_hi + 3u * m;
    atomicMin(lo + 0, f2ord(c.x)), atomicMin(lo + 1, f2ord(c.y)), atomicMin(lo + 2, f2ord(c.z));
    atomicMax(hi + 0, f2ord(c.x)), atomicMax(hi + 1, f2ord(c.y)), atomicMax(hi + 2, f2ord(c.z));
}

__device__ __forceinline__ uint32_t spread10(uint32_t x) {   // 10 bits -> every third bit
    x = (x | (x << 16)) & 0x030000FFu;
    x = (x | (x << 8)) & 0x0300F00Fu;
    x = (x | (x << 4)) & 0x030C30C3u;
    x = (x | (x << 2)) & 0x09249249u;
    return x;
}
// a cell 0 .. 1023 along one axis; anything not finite lands in cell 0 (the code only orders, it decides no result)
__device__ __forceinline__ uint32_t cell10(float c, float lo, float hi) {
    const float x = (c - lo) / (hi - lo) * 1024.0f;
    return (uint32_t)fminf(fmaxf(x, 0.0f), 1023.0f);
}

__global__ __launch_bounds__(ACCEL_WG) void k_accel_keys(AccelBuild B) {
    const uint32_t g = blockIdx.x * ACCEL_WG + threadIdx.x;
    const bool live = g < B.ntri;
    bool wild = false;
    if (live) {
        const TriInfo T = tri_info(B, g);
        const uint32_t m = last_le(B.tin_prefix, 0, B.n_meshes, g);
        wild = T.wild;
        uint32_t code = 0xFFFFFFFFu;
        if (!wild) {
            const uint32_t *lo = B.box_lo + 3u * m, *hi = B.box_hi + 3u * m;
            const F3 c = centroid(T);
            code = spread10(cell10(c.x, ord2f(lo[0]), ord2f(hi[0]))) | (spread10(cell10(c.y, ord2f(lo[1]), ord2f(hi[1]))) << 1) |
                   (spread10(cell10(c.z, ord2f(lo[2]), ord2f(hi[2]))) << 2);
        }
        B.keys[g] = ((unsigned long long)m << 32) | code;
        B.vals[g] = g;
    }
    const unsigned long long w = __ballot(wild);
    if (w && __lane_id() == 0) atomicAdd(B.stats + 1, (unsigned long long)__popcll(w));
}

// the records of k_isect_prep (rxr_intersect.hip), at the triangles' sorted positions
__global__ __launch_bounds__(ACCEL_WG) void k_accel_records(AccelBuild B) {
    const uint32_t pos = blockIdx.x * ACCEL_WG + threadIdx.x;
    if (pos >= B.ntri) return;
    const uint32_t g = B.perm[pos];
    if (g >= B.ntri) return;   // (a sort that went wrong must not read out of bounds)
    const TriInfo T = tri_info(B, g);
    const size_t s = B.stride;
    float *p = B.tris + pos;
    p[0] = T.v0.x, p[s] = T.v0.y, p[2 * s] = T.v0.z;
    p[3 * s] = T.e1.x, p[4 * s] = T.e1.y, p[5 * s] = T.e1.z;
    p[6 * s] = T.e2.x, p[7 * s] = T.e2.y, p[8 * s] = T.e2.z;
}

__device__ __forceinline__ AccelNode empty_node() {
    return AccelNode{{INFINITY, INFINITY, INFINITY}, 0.0f, {-INFINITY, -INFINITY, -INFINITY}, 0.0f};
}
__device__ __forceinline__ void make_wild(AccelNode &N) {
    N = AccelNode{{-INFINITY, -INFINITY, -INFINITY}, 1.0f, {INFINITY, INFINITY, INFINITY}, INFINITY};
}
__device__ __forceinline__ void grow(AccelNode &N, F3 v) {
    N.lo[0] = fminf(N.lo[0], v.x), N.lo[1] = fminf(N.lo[1], v.y), N.lo[2] = fminf(N.lo[2], v.z);
    N.hi[0] = fmaxf(N.hi[0], v.x), N.hi[1] = fmaxf(N.hi[1], v.y), N.hi[2] = fmaxf(N.hi[2], v.z);
}
__device__ __forceinline__ void finish_node(AccelNode &N) {
    float m = 0.0f;
#pragma unroll
    for (int i = 0; i < 3; ++i) m = fmaxf(m, fmaxf(fabsf(N.lo[i]), fabsf(N.hi[i])));
    N.maxabs = m;
}

__global__ __launch_bounds__(ACCEL_WG) void k_accel_leaves(AccelBuild B, uint32_t n_leaves) {
    const uint32_t leaf = blockIdx.x * ACCEL_WG + threadIdx.x;
    if (leaf >= n_leaves) return;
    AccelNode N = empty_node();
    bool wild = false;
    const uint32_t p0 = leaf * ACCEL_L, p1 = min(p0 + ACCEL_L, B.ntri);
    for (uint32_t pos = p0; pos < p1; ++pos) {
        const uint32_t g = B.perm[pos];
        if (g >= B.ntri) {
            wild = true;
            continue;
        }
        const TriInfo T = tri_info(B, g);
        wild |= T.wild;
        if (!T.wild) {
            grow(N, T.v0), grow(N, T.v1), grow(N, T.v2);
            N.kappa = fmaxf(N.kappa, T.kappa);
        }
    }
    if (wild) make_wild(N);
    else finish_node(N);
    B.nodes[leaf] = N;
}

__global__ __launch_bounds__(ACCEL_WG) void k_accel_level(AccelNode *nodes, uint32_t child_off, uint32_t n_children, uint32_t off, uint32_t n) {
    const uint32_t i = blockIdx.x * ACCEL_WG + threadIdx.x;
    if (i >= n) return;
    AccelNode N = empty_node();
    bool wild = false;
    const uint32_t c0 = i * ACCEL_W, c1 = min(c0 + ACCEL_W, n_children);
    for (uint32_t c = c0; c < c1; ++c) {
        const AccelNode C = nodes[child_off + c];
        wild |= !(C.maxabs < INFINITY);
        grow(N, {C.lo[0], C.lo[1], C.lo[2]}), grow(N, {C.hi[0], C.hi[1], C.hi[2]});
        N.kappa = fmaxf(N.kappa, C.kappa);
    }
    if (wild) make_wild(N);
    else finish_node(N);
    nodes[off + i] = N;
}

struct AccelArgs {
    uint32_t ntri, nseg, stride;
    const float *tris;          // sorted records
    const uint32_t *perm;
    const AccelNode *nodes;
    const AccelSeg *segs;
    const float *origins, *dirs;
    unsigned long long *keys;   // [rays of the batch][nseg]
    unsigned long long *stats;
    AccelLevels lev;
};

__device__ __forceinline__ uint32_t accel_seg_of(const AccelArgs &A, uint32_t pos) {
    uint32_t lo = 0, hi = A.nseg;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (A.segs[mid].begin <= pos) lo = mid;
        else hi = mid;
    }
    return lo;
}

// The cull (tests/ray_accel_ref.py: box_pass restates it operation for operation): a float32 slab test against the node's box grown
// by pad = C eps32 kappa (max|o_i| + maxabs); min / max ignore NaN operands; it passes iff t_near <= t_far and t_far >= 0.
// `omax` = max|o_i|, `inv` = 1 / d of the normalised direction.
__device__ __forceinline__ bool box_pass(const AccelNode &N, F3 o, F3 inv, float omax) {
    if (!(N.maxabs < INFINITY)) return true;
    const float pad = (ACCEL_PAD_SCALE * N.kappa) * (omax + N.maxabs);
    float tn = -INFINITY, tf = INFINITY;
    const float oo[3] = {o.x, o.y, o.z}, ii[3] = {inv.x, inv.y, inv.z};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float a = ((N.lo[i] - pad) - oo[i]) * ii[i], b = ((N.hi[i] + pad) - oo[i]) * ii[i];
        tn = fmaxf(tn, fminf(a, b));
        tf = fminf(tf, fmaxf(a, b));
    }
    return tn <= tf && tf >= 0.0f;
}

// many rays: a thread per ray walks the tree; per ray and segment one atomic with the segment's minimum.  COUNT: the ray-triangle
// tests run, summed over the wave, one atomic add per wave at the end.
template <bool COUNT>
__global__ __launch_bounds__(ACCEL_WG) void k_accel_by_ray(AccelArgs A, uint32_t r0, uint32_t nr) {
    __shared__ uint2 lev[ACCEL_MAX_LEVELS];   // (first node, nodes) per level
    if (threadIdx.x < ACCEL_MAX_LEVELS) lev[threadIdx.x] = make_uint2(A.lev.off[threadIdx.x], A.lev.cnt[threadIdx.x]);
    __syncthreads();
    const uint32_t r = blockIdx.x * ACCEL_WG + threadIdx.x;
    bool active = r < nr;
    F3 o{}, d{}, inv{};
    float omax = 0.0f;
    if (active) {
        o = load3(A.origins, (uint64_t)r0 + r);
        d = normalized3(load3(A.dirs, (uint64_t)r0 + r));
        // a ray with a component that is not finite (a zero direction normalises to NaN) is rejected by every mt_test: no walk at all
        active = finite3(o) && finite3(d);
        inv = {1.0f / d.x, 1.0f / d.y, 1.0f / d.z};
        omax = fmaxf(fmaxf(fabsf(o.x), fabsf(o.y)), fabsf(o.z));
    }
    unsigned long long tests = 0;
    if (active) {
        const uint32_t top = A.lev.n - 1;
        const size_t st = A.stride;
        unsigned long long *slot = A.keys + (uint64_t)r * A.nseg;
        uint32_t level = top, idx = 0;
        uint32_t s = 0, send = 0;   // the segment of the last leaf entered: [.., send)
        unsigned long long best = RXR_ISECT_NO_HIT;
        for (;;) {
            const uint2 lv = lev[level];
            const bool pass = box_pass(A.nodes[lv.x + idx], o, inv, omax);
            if (pass && level > 0) {
                --level;
                idx *= ACCEL_W;
                continue;
            }
            if (pass) {
                const uint32_t p0 = idx * ACCEL_L, p1 = min(p0 + ACCEL_L, A.ntri);
                if (p0 >= send) {   // the first leaf, or leaves were skipped
                    if (best != RXR_ISECT_NO_HIT) atomicMin(slot + s, best);
                    best = RXR_ISECT_NO_HIT;
                    s = accel_seg_of(A, p0);
                    send = A.segs[s].end;
                }
                for (uint32_t pos = p0; pos < p1; ++pos) {
                    if (pos == send) {   // segments are never empty and cover every position: one step
                        if (best != RXR_ISECT_NO_HIT) atomicMin(slot + s, best);
                        best = RXR_ISECT_NO_HIT;
                        ++s;
                        send = A.segs[s].end;
                    }
                    const float *p = A.tris + pos;
                    float t, u, v;
                    if (COUNT) ++tests;
                    if (mt_test(o, d, {p[0], p[st], p[2 * st]}, {p[3 * st], p[4 * st], p[5 * st]}, {p[6 * st], p[7 * st], p[8 * st]}, t, u, v)) {
                        const unsigned long long key = ((unsigned long long)__float_as_uint(t) << 32) | A.perm[pos];
                        best = key < best ? key : best;
                    }
                }
            }
            ++idx;
            while (level < top && (idx % ACCEL_W == 0 || idx == lev[level].y)) {
                idx = (idx - 1) / ACCEL_W + 1;
                ++level;
            }
            if (level == top) break;   // (the root has no sibling)
        }
        if (best != RXR_ISECT_NO_HIT) atomicMin(slot + s, best);
    }
    if (COUNT) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) tests += __shfl_xor(tests, off);
        if (__lane_id() == 0 && tests) atomicAdd(A.stats, tests);
    }
}

AccelLevels accel_levels(uint32_t ntri) {
    AccelLevels V{};
    uint32_t n = (ntri + ACCEL_L - 1) / ACCEL_L, off = 0;
    for (;;) {
        V.off[V.n] = off;
        V.cnt[V.n] = n;
        ++V.n;
        off += n;
        if (n <= 1 || V.n == ACCEL_MAX_LEVELS) break;
        n = (n + ACCEL_W - 1) / ACCEL_W;
    }
    return V;
}

}  // namespace

// the tree over the current meshes, queued on `s` behind the records of isect_prepare
int rxr_ray_accel_build(rxr_ctx *ctx, hipStream_t s) {
    const uint32_t ntri = ctx->PP.n_tris_in, n_meshes = (uint32_t)ctx->meshes.size();
    int rc;
    if ((rc = rxr_ensure(ctx, ctx->d_accel_stats, 256)) != RXR_OK) return rc;
    if (!ctx->accel_stats_zeroed) {
        HIPCHK(ctx, hipMemsetAsync(ctx->d_accel_stats.p, 0, 256, s));
        ctx->accel_stats_zeroed = true;
    }
    HIPCHK(ctx, hipMemsetAsync((unsigned long long *)ctx->d_accel_stats.p + 1, 0, 8, s));
    ctx->accel_ntri = ntri;
    ctx->accel_nodes = ctx->accel_levels = 0;
    ++ctx->accel_builds;
    ctx->accel_ready = true;
    if (!ntri) return RXR_OK;
    const AccelLevels V = accel_levels(ntri);
    if (V.cnt[V.n - 1] != 1) return rxr_fail(ctx, RXR_ERR_UNSUPPORTED, "ray accel: more triangles than the tree's levels hold");
    const uint32_t n_nodes = V.off[V.n - 1] + 1;
    const size_t stride = ctx->isect_stride;
    // scratch: mesh boxes, keys and values in and out, rocPRIM's own
    size_t sort_bytes = 0;
    unsigned long long *knull = nullptr;
    uint32_t *vnull = nullptr;
    const unsigned end_bit = 32u + (n_meshes > 1 ? 32u - (unsigned)__builtin_clz(n_meshes - 1) : 0u);
    HIPCHK(ctx, rocprim::radix_sort_pairs(nullptr, sort_bytes, knull, knull, vnull, vnull, (size_t)ntri, 0u, end_bit, s));
    BlobCursor take;
    const size_t o_box = take((size_t)n_meshes * 24), o_k0 = take((size_t)ntri * 8), o_k1 = take((size_t)ntri * 8), o_v0 = take((size_t)ntri * 4),
                 o_tmp = take(sort_bytes);
    if ((rc = rxr_ensure(ctx, ctx->d_accel_scratch, take.o)) != RXR_OK) return rc;
    if ((rc = rxr_ensure(ctx, ctx->d_accel_tris, std::max<size_t>(9 * stride * 4, 256))) != RXR_OK) return rc;
    if ((rc = rxr_ensure(ctx, ctx->d_accel_perm, (size_t)ntri * 4)) != RXR_OK) return rc;
    if ((rc = rxr_ensure(ctx, ctx->d_accel_nodes, (size_t)n_nodes * sizeof(AccelNode))) != RXR_OK) return rc;
    uint8_t *sc = (uint8_t *)ctx->d_accel_scratch.p;
    AccelBuild B{};
    B.ntri = ntri;
    B.n_meshes = n_meshes;
    B.stride = (uint32_t)stride;
    B.tin_prefix = ctx->PP.tin_prefix;
    B.vin_prefix = ctx->PP.vin_prefix;
    B.obj_idx = ctx->PP.obj_idx;
    B.obj_verts = ctx->PP.obj_verts;
    B.box_lo = (uint32_t *)(sc + o_box);
    B.box_hi = B.box_lo + 3u * (size_t)n_meshes;
    B.keys = (unsigned long long *)(sc + o_k0);
    B.vals = (uint32_t *)(sc + o_v0);
    B.perm = (const uint32_t *)ctx->d_accel_perm.p;
    B.tris = (float *)ctx->d_accel_tris.p;
    B.nodes = (AccelNode *)ctx->d_accel_nodes.p;
    B.stats = (unsigned long long *)ctx->d_accel_stats.p;
    const dim3 per_tri((ntri + ACCEL_WG - 1) / ACCEL_WG), wg(ACCEL_WG);
    // the boxes start empty: lo = the largest word, hi = the smallest
    HIPCHK(ctx, hipMemsetAsync(B.box_lo, 0xFF, (size_t)n_meshes * 12, s));
    HIPCHK(ctx, hipMemsetAsync(B.box_hi, 0, (size_t)n_meshes * 12, s));
    hipLaunchKernelGGL(k_accel_mesh_boxes, per_tri, wg, 0, s, B);
    HIPCHK(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_accel_keys, per_tri, wg, 0, s, B);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, rocprim::radix_sort_pairs(sc + o_tmp, sort_bytes, B.keys, (unsigned long long *)(sc + o_k1), B.vals, (uint32_t *)ctx->d_accel_perm.p,
                                          (size_t)ntri, 0u, end_bit, s));
    hipLaunchKernelGGL(k_accel_records, per_tri, wg, 0, s, B);
    HIPCHK(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_accel_leaves, dim3((V.cnt[0] + ACCEL_WG - 1) / ACCEL_WG), wg, 0, s, B, V.cnt[0]);
    HIPCHK(ctx, hipGetLastError());
    for (uint32_t k = 1; k < V.n; ++k) {
        hipLaunchKernelGGL(k_accel_level, dim3((V.cnt[k] + ACCEL_WG - 1) / ACCEL_WG), wg, 0, s, B.nodes, V.off[k - 1], V.cnt[k - 1], V.off[k], V.cnt[k]);
        HIPCHK(ctx, hipGetLastError());
    }
    ctx->accel_nodes = n_nodes;
    ctx->accel_levels = V.n;
    return RXR_OK;
}

bool rxr_ray_accel_takes(const rxr_ctx *ctx) { return ctx->accel_mode != RXR_RAY_ACCEL_OFF && ctx->accel_ready && ctx->accel_nodes != 0; }

int rxr_ray_accel_begin_call(rxr_ctx *ctx, hipStream_t s) {
    if (ctx->accel_mode == RXR_RAY_ACCEL_COUNT && ctx->accel_ready) HIPCHK(ctx, hipMemsetAsync(ctx->d_accel_stats.p, 0, 8, s));
    return RXR_OK;
}

int rxr_ray_accel_closest(rxr_ctx *ctx, const void *dev_segs, uint32_t nseg, const float *dev_origins, const float *dev_dirs, uint32_t r0, uint32_t nr,
                          unsigned long long *dev_keys, hipStream_t s) {
    AccelArgs A{};
    A.ntri = ctx->accel_ntri;
    A.nseg = nseg;
    A.stride = ctx->isect_stride;
    A.tris = (const float *)ctx->d_accel_tris.p;
    A.perm = (const uint32_t *)ctx->d_accel_perm.p;
    A.nodes = (const AccelNode *)ctx->d_accel_nodes.p;
    A.segs = (const AccelSeg *)dev_segs;
    A.origins = dev_origins;
    A.dirs = dev_dirs;
    A.keys = dev_keys;
    A.stats = (unsigned long long *)ctx->d_accel_stats.p;
    A.lev = accel_levels(A.ntri);
    const dim3 grid((nr + ACCEL_WG - 1) / ACCEL_WG), wg(ACCEL_WG);
    if (ctx->accel_mode == RXR_RAY_ACCEL_COUNT) hipLaunchKernelGGL(k_accel_by_ray<true>, grid, wg, 0, s, A, r0, nr);
    else hipLaunchKernelGGL(k_accel_by_ray<false>, grid, wg, 0, s, A, r0, nr);
    HIPCHK(ctx, hipGetLastError());
    ++ctx->accel_batches;
    return RXR_OK;
}

extern "C" {

int rxr_set_ray_accel(rxr_ctx *ctx, uint32_t mode) {
    if (!ctx) return RXR_ERR_INVALID;
    if (mode > RXR_RAY_ACCEL_COUNT) return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_set_ray_accel: mode must be RXR_RAY_ACCEL_OFF, _ON or _COUNT");
    if (ctx->group) return rxr_as_member0(ctx, [&](rxr_ctx *m) { return rxr_set_ray_accel(m, mode); });
    ctx->accel_mode = mode;
    return RXR_OK;
}

int rxr_ray_accel_info(rxr_ctx *ctx, uint64_t out[RXR_RAY_ACCEL_INFO_WORDS]) {
    if (!ctx) return RXR_ERR_INVALID;
    if (!out) return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_ray_accel_info: out is NULL");
    if (ctx->group) return rxr_as_member0(ctx, [&](rxr_ctx *m) { return rxr_ray_accel_info(m, out); });
    HIPCHK(ctx, hipSetDevice(ctx->device));
    unsigned long long stats[2] = {0, 0};
    if (ctx->d_accel_stats.p && ctx->accel_stats_zeroed) {
        int rc = rxr_quiesce(ctx);
        if (rc != RXR_OK) return rc;
        HIPCHK(ctx, hipMemcpy(stats, ctx->d_accel_stats.p, 16, hipMemcpyDeviceToHost));
    }
    const bool valid = ctx->isect_ready && ctx->accel_ready;
    out[RXR_RAY_ACCEL_INFO_MODE] = ctx->accel_mode;
    out[RXR_RAY_ACCEL_INFO_VALID] = valid ? 1u : 0u;
    out[RXR_RAY_ACCEL_INFO_TRIANGLES] = valid ? ctx->accel_ntri : 0u;
    out[RXR_RAY_ACCEL_INFO_NODES] = valid ? ctx->accel_nodes : 0u;
    out[RXR_RAY_ACCEL_INFO_LEVELS] = valid ? ctx->accel_levels : 0u;
    out[RXR_RAY_ACCEL_INFO_WILD] = valid ? stats[1] : 0u;
    out[RXR_RAY_ACCEL_INFO_BUILDS] = ctx->accel_builds;
    out[RXR_RAY_ACCEL_INFO_BATCHES] = ctx->accel_batches;
    out[RXR_RAY_ACCEL_INFO_TESTS] = stats[0];
    return RXR_OK;
}

}  // extern "C"
