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
// Refit (opt-in, rxr_set_ray_refresh; the kernels after the walk): after rxr_update_meshes under RXR_RAY_REFRESH_RANGED nothing above
// is run again -- the dirty meshes' sorted records, the leaves over them and their ancestors are rewritten over the same perm.
// A triangle is WILD -- its leaf and every ancestor get an infinite box and are always entered -- when a value of its record is not
// finite or its kappa = |e1| |e2| / |e1 x e2| is not finite or above ACCEL_KAPPA_CAP.
//
// Walk (k_accel_by_ray, a thread per ray): depth-first and stackless, the state is (level, index).  A passing node above the leaves
// descends to index * W; otherwise index + 1, and while that index is a multiple of W or the end of its level, up to
// (index - 1) / W + 1.  The position only moves forward, so the walk ends after at most `nodes` steps whatever the boxes hold.
// Leaves come in increasing position, hence in segment order: the segment's minimum is flushed when the position crosses its end.
// Walk (k_accel_by_wave, a wave per ray, opt-in on top: rxr_set_ray_wave): for batches too small to fill the
// device with a thread per ray -- the comment above that kernel has its visit rule and why the duty above still holds.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "rxr_debug.h"
#include "rxr_isect.h"
#include "rxr_query.h"
#include "rxr_ray_refresh.h"

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

__device__ __forceinline__ void close_node(AccelNode &N, bool wild) {
    if (wild) make_wild(N);
    else finish_node(N);
}

// a leaf's node from the pools, through the resident order: the one sequential loop both the build and a refit run (the same
// operations in the same order: the same bits, signs of zero included)
__device__ __forceinline__ AccelNode leaf_node(const AccelBuild &B, uint32_t leaf) {
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
    close_node(N, wild);
    return N;
}

// one child folded into its parent (close_node closes it): the statements of k_accel_level's loop, for the refit kernels.  (The build
// kernel keeps its own copy: calling this from it changes its register allocation, and its instructions are pinned.)
__device__ __forceinline__ void fold_child(AccelNode &N, bool &wild, const AccelNode &C) {
    wild |= !(C.maxabs < INFINITY);
    grow(N, {C.lo[0], C.lo[1], C.lo[2]}), grow(N, {C.hi[0], C.hi[1], C.hi[2]});
    N.kappa = fmaxf(N.kappa, C.kappa);
}

__global__ __launch_bounds__(ACCEL_WG) void k_accel_leaves(AccelBuild B, uint32_t n_leaves) {
    const uint32_t leaf = blockIdx.x * ACCEL_WG + threadIdx.x;
    if (leaf >= n_leaves) return;
    B.nodes[leaf] = leaf_node(B, leaf);
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

// ---- a wave per ray (rxr_set_ray_wave) -----------------------------------------------------------------------
// k_accel_by_wave: the 64 lanes of a wave walk ONE ray together over the same nodes, records, perm and segment table, for batches too
// small to fill the device with a thread per ray.  ACCEL_WG threads are four rays; the four waves never meet (no barrier: each wave
// writes the level table itself -- the same words -- and reads what it wrote).
//
// Walk: depth-first over the implicit levels, two levels a step.  Entering node (l, i):
//   l odd, >= 3   lane j runs box_pass on node i * 64 + j of level l - 2 (clipped to that level's count); the ballot of the passing
//                 ones is pushed as a frame, its set bits are entered lowest first
//   l even, >= 2  (only the root of a tree with an even top level can be: every frame below it is on an odd level) one level: lanes
//                 0 .. 7 test the children i * 8 + j of level l - 1, so that every later step ends on level 1 with 64 lanes at work
//   l == 1        the lanes take the node's sorted positions [i * 64, min(i * 64 + 64, ntri)), one each, through mt_test
//   l == 0        (a tree of one leaf) the lanes take its up to 8 positions
// The root's own box is not tested.  LEAF BOXES: at l == 1 the eight leaf boxes below the node are NOT tested (RXR_RAY_WAVE_LEAF_BOXES
// 0, the shipped choice; 1 tests them with lanes 0 .. 7 first and masks each leaf's eight lanes by its box: the A-B of
// profiles/ray_wave/README.md).  tests/ray_wave_ref.py: wave_walk restates this rule.
// The frames' masks live in LDS, ACCEL_WAVE_STACK per wave, the top one in scalar registers; a frame's level and its parent's index
// follow from the depth (a frame is two levels below the one under it; the parent's index is the child's >> 6), so nothing else is
// stacked.  ACCEL_MAX_LEVELS = 24 bounds the depth: the root's frame and one per odd level below the top, at most 12.
//
// THE ONE DUTY IS UNCHANGED.  A position is left out only because box_pass -- the same function on the same node and the same o, inv,
// omax that k_accel_by_ray computes -- failed on one of its ancestors.  The ancestors tested here are a subset of those the thread walk
// tests (every other level, never the root, by default not the leaf), so this walk enters a superset of the thread walk's leaves, and
// mt_test on the same records gives the same t bits and the same keys; whole keys go through atomicMin, whose result does not depend
// on order.  Its keys equal the brute-force keys under the measured margin of section 19 and no new one.
// TERMINATION.  Every turn of the loop either clears one bit of the top mask, or drops an empty top mask, or (entering a node) pushes
// a mask for a strictly lower level; a node is entered once per bit, bits are only ever cleared, and the level table bounds the nodes.
// The loop ends when the stack is empty whatever the boxes hold: a build or refit bug cannot hang the device.
#ifndef RXR_RAY_WAVE_LEAF_BOXES
#define RXR_RAY_WAVE_LEAF_BOXES 0
#endif
constexpr uint32_t ACCEL_WAVE_STACK = 12;
static_assert(ACCEL_W == 8 && ACCEL_L == 8, "k_accel_by_wave: 64 grandchildren a node, 64 positions a level-1 node");
static_assert(ACCEL_MAX_LEVELS / 2 <= ACCEL_WAVE_STACK, "k_accel_by_wave: a frame per odd level and the root's");

__device__ __forceinline__ uint32_t uniform32(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }
__device__ __forceinline__ unsigned long long uniform64(unsigned long long x) {
    return ((unsigned long long)uniform32((uint32_t)(x >> 32)) << 32) | uniform32((uint32_t)x);
}

template <bool COUNT>
__global__ __launch_bounds__(ACCEL_WG) void k_accel_by_wave(AccelArgs A, uint32_t r0, uint32_t nr) {
    __shared__ uint2 lev[ACCEL_MAX_LEVELS];   // (first node, nodes) per level
    __shared__ unsigned long long stack[ACCEL_WG / 64][ACCEL_WAVE_STACK];   // a wave's masks: written by lane 0, read back by all
    const uint32_t lane = threadIdx.x & 63u, wave = uniform32(threadIdx.x >> 6);
    if (lane < ACCEL_MAX_LEVELS) lev[lane] = make_uint2(A.lev.off[lane], A.lev.cnt[lane]);
    const uint32_t r = blockIdx.x * (ACCEL_WG / 64) + wave;
    if (r >= nr) return;
    const F3 o = load3(A.origins, (uint64_t)r0 + r);
    const F3 d = normalized3(load3(A.dirs, (uint64_t)r0 + r));
    if (!(finite3(o) && finite3(d))) return;   // as k_accel_by_ray: every mt_test rejects such a ray
    const F3 inv = {1.0f / d.x, 1.0f / d.y, 1.0f / d.z};
    const float omax = fmaxf(fmaxf(fabsf(o.x), fabsf(o.y)), fabsf(o.z));
    const size_t st = A.stride;
    unsigned long long *slot = A.keys + (uint64_t)r * A.nseg;

    // flush: the wave's minimum of `best` into the segment's slot, one atomic
    unsigned long long best = RXR_ISECT_NO_HIT;
    uint32_t s = 0, send = 0;   // the segment of the last positions taken: [.., send)
    auto flush = [&]() {
        if (__ballot(best != RXR_ISECT_NO_HIT)) {
            unsigned long long m = best;
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                const unsigned long long x = __shfl_xor(m, off);
                m = x < m ? x : m;
            }
            if (lane == 0) atomicMin(slot + s, m);
        }
        best = RXR_ISECT_NO_HIT;
    };

    unsigned long long tests = 0;
    // the frames: `cur` = the top mask, over nodes pidx * 64 + bit of level `flevel`; the root is a frame of one bit
    unsigned long long cur = 1;
    uint32_t sp = 1, pidx = 0, flevel = A.lev.n - 1;
    while (sp) {
        if (!cur) {   // the frame is done: back to the one below
            --sp;
            __builtin_amdgcn_wave_barrier();   // (no instruction: LDS operations of one wave complete in order)
            if (sp) cur = uniform64(stack[wave][sp - 1]);
            pidx >>= 6;
            flevel += 2;
            continue;
        }
        const uint32_t bit = (uint32_t)__builtin_ctzll(cur);
        cur &= cur - 1;
        const uint32_t level = flevel, idx = (pidx << 6) + bit;
        if (level >= 2) {
            const uint32_t down = (level & 1u) ? 2u : 1u, fan = (level & 1u) ? 64u : 8u;
            const uint32_t off = uniform32(lev[level - down].x), cnt = uniform32(lev[level - down].y);
            const uint32_t c = idx * fan + lane;
            bool pass = false;
            if (lane < fan && c < cnt) pass = box_pass(A.nodes[off + c], o, inv, omax);
            const unsigned long long m = __ballot(pass);
            if (m && sp < ACCEL_WAVE_STACK) {   // (sp cannot reach the bound: the static_assert above)
                if (lane == 0) stack[wave][sp - 1] = cur;
                __builtin_amdgcn_wave_barrier();
                cur = m;
                ++sp;
                pidx = idx;
                flevel = level - down;
            }
            continue;
        }
        // level 1: the 64 positions below the node; level 0 (a tree of one leaf): its 8
        const uint32_t p0 = idx * (level ? ACCEL_L * ACCEL_W : ACCEL_L), p1 = min(p0 + (level ? ACCEL_L * ACCEL_W : ACCEL_L), A.ntri);
        if (p0 >= p1) continue;
        const uint32_t pos = p0 + lane;
        bool take = pos < p1;
#if RXR_RAY_WAVE_LEAF_BOXES
        {
            const uint32_t leaf = p0 / ACCEL_L + lane, cnt0 = uniform32(lev[0].y);
            bool pass = false;
            if (lane < ACCEL_W && leaf < cnt0) pass = box_pass(A.nodes[uniform32(lev[0].x) + leaf], o, inv, omax);
            take = take && ((__ballot(pass) >> (lane / ACCEL_L)) & 1ull);
        }
#endif
        if (p0 >= send) {   // the first positions, or positions were skipped
            flush();
            s = uniform32(accel_seg_of(A, p0));
            send = uniform32(A.segs[s].end);
        }
        const bool one_segment = p1 <= send;
        if (!one_segment) flush();
        if (COUNT) tests += (unsigned long long)__popcll(__ballot(take));
        if (take) {
            const float *p = A.tris + pos;
            float t, u, v;
            if (mt_test(o, d, {p[0], p[st], p[2 * st]}, {p[3 * st], p[4 * st], p[5 * st]}, {p[6 * st], p[7 * st], p[8 * st]}, t, u, v)) {
                const unsigned long long key = ((unsigned long long)__float_as_uint(t) << 32) | A.perm[pos];
                if (one_segment) best = key < best ? key : best;
                else atomicMin(slot + accel_seg_of(A, pos), key);   // the positions straddle segments: each lane finds its own
            }
        }
    }
    flush();
    if (COUNT && lane == 0 && tests) atomicAdd(A.stats, tests);
}

// ---- the ranged refit after rxr_update_meshes (rxr_set_ray_refresh) ------------------------------------------
// The order of the last build stays (perm is not touched): a dirty mesh's triangles keep their range of sorted positions, so their
// records, the leaves over those positions and the leaves' ancestors are rewritten, each by the build's arithmetic over the same
// perm.  The tree's duty -- never skip a triangle mt_test would accept -- does not depend on the order the triangles sit in.

// wild as tri_info decides it, from a sorted record (v0, e1, e2 are its nine words: the same operands, the same kappa)
__device__ __forceinline__ bool record_wild(F3 v0, F3 e1, F3 e2) {
    const F3 n = cross3(e1, e2);
    const float kappa = (sqrtf(dot3(e1, e1)) * sqrtf(dot3(e2, e2))) / sqrtf(dot3(n, n));
    return !(finite3(v0) && finite3(e1) && finite3(e2)) || !(kappa <= ACCEL_KAPPA_CAP);
}

// a thread per dirty sorted position: the record of k_accel_records; stats[1] moves by (wild now) - (wild before), one atomic a wave
__global__ __launch_bounds__(ACCEL_WG) void k_accel_refresh_records(AccelBuild B, RxrDirtyTris D) {
    const uint32_t t = blockIdx.x * ACCEL_WG + threadIdx.x;
    bool was = false, is = false;
    if (t < D.total) {
        const uint32_t i = last_le(D.pre, 0, D.n, t);
        const uint32_t pos = D.base[i] + (t - D.pre[i]);
        const uint32_t g = pos < B.ntri ? B.perm[pos] : 0xFFFFFFFFu;
        if (g < B.ntri) {   // (k_accel_records leaves such a position alone, and k_accel_keys never counted it)
            const size_t s = B.stride;
            float *p = B.tris + pos;
            was = record_wild({p[0], p[s], p[2 * s]}, {p[3 * s], p[4 * s], p[5 * s]}, {p[6 * s], p[7 * s], p[8 * s]});
            const TriInfo T = tri_info(B, g);
            is = T.wild;
            p[0] = T.v0.x, p[s] = T.v0.y, p[2 * s] = T.v0.z;
            p[3 * s] = T.e1.x, p[4 * s] = T.e1.y, p[5 * s] = T.e1.z;
            p[6 * s] = T.e2.x, p[7 * s] = T.e2.y, p[8 * s] = T.e2.z;
        }
    }
    const long long delta = (long long)__popcll(__ballot(is && !was)) - (long long)__popcll(__ballot(was && !is));
    if (delta && __lane_id() == 0) atomicAdd(B.stats + 1, (unsigned long long)delta);   // (modulo 2^64: the sum never leaves [0, ntri])
}

// the dirty nodes of one level: n_iv intervals, first nodes lo[], prefix counts pre[] (pre[n_iv] = total)
struct RefitLevel {
    const uint32_t *lo, *pre;
    uint32_t n_iv, total;
};
__device__ __forceinline__ uint32_t refit_node(const RefitLevel &R, uint32_t t) {
    const uint32_t i = last_le(R.pre, 0, R.n_iv, t);
    return R.lo[i] + (t - R.pre[i]);
}
// the slot of node c among the level's dirty nodes, or 0xFFFFFFFF for a node that is not dirty
__device__ __forceinline__ uint32_t refit_slot(const RefitLevel &R, uint32_t c) {
    if (!R.n_iv || c < R.lo[0]) return 0xFFFFFFFFu;
    const uint32_t i = last_le(R.lo, 0, R.n_iv, c);
    return c - R.lo[i] < R.pre[i + 1] - R.pre[i] ? R.pre[i] + (c - R.lo[i]) : 0xFFFFFFFFu;
}

// general route: a launch per level, a thread per dirty node
__global__ __launch_bounds__(ACCEL_WG) void k_accel_refit_leaves(AccelBuild B, RefitLevel R, uint32_t n_leaves) {
    const uint32_t t = blockIdx.x * ACCEL_WG + threadIdx.x;
    if (t >= R.total) return;
    const uint32_t leaf = refit_node(R, t);
    if (leaf >= n_leaves) return;
    B.nodes[leaf] = leaf_node(B, leaf);
}

__global__ __launch_bounds__(ACCEL_WG) void k_accel_refit_level(AccelNode *nodes, uint32_t child_off, uint32_t n_children, uint32_t off, uint32_t n, RefitLevel R) {
    const uint32_t t = blockIdx.x * ACCEL_WG + threadIdx.x;
    if (t >= R.total) return;
    const uint32_t i = refit_node(R, t);
    if (i >= n) return;
    AccelNode N = empty_node();
    bool wild = false;
    const uint32_t c0 = i * ACCEL_W, c1 = min(c0 + ACCEL_W, n_children);
    for (uint32_t c = c0; c < c1; ++c) fold_child(N, wild, nodes[child_off + c]);
    close_node(N, wild);
    nodes[off + i] = N;
}

// small route: one workgroup, every level, a barrier between levels.  S holds the nodes of the level just written, in slot order; a
// parent takes a child this launch rewrote from S and any other from global memory, so nothing written here is read back through
// global memory.  A level's nodes overwrite S in place: parent slot j only reads child slots >= j (every dirty parent has a dirty child
// of its own), a pass of ACCEL_WG parents computes, meets at a barrier, then writes slots below the next pass's children.
struct RefitSmall {
    uint32_t n_levels;
    uint32_t off[ACCEL_MAX_LEVELS], n_iv[ACCEL_MAX_LEVELS], total[ACCEL_MAX_LEVELS];   // RxrRefitLaunch's
};
__global__ __launch_bounds__(ACCEL_WG) void k_accel_refit_small(AccelBuild B, AccelLevels V, RefitSmall Q, const uint32_t *table) {
    __shared__ AccelNode S[RXR_RAY_REFIT_SMALL_MAX];
    RefitLevel R{table + Q.off[0], table + Q.off[0] + Q.n_iv[0], Q.n_iv[0], min(Q.total[0], RXR_RAY_REFIT_SMALL_MAX)};
    for (uint32_t t = threadIdx.x; t < R.total; t += ACCEL_WG) {
        const uint32_t leaf = refit_node(R, t);
        if (leaf >= V.cnt[0]) continue;
        const AccelNode N = leaf_node(B, leaf);
        S[t] = N;
        B.nodes[leaf] = N;
    }
    __syncthreads();
    for (uint32_t k = 1; k < Q.n_levels; ++k) {
        const RefitLevel C = R;   // the level below: its dirty nodes are in S
        R = RefitLevel{table + Q.off[k], table + Q.off[k] + Q.n_iv[k], Q.n_iv[k], min(Q.total[k], C.total)};
        const uint32_t child_off = V.off[k - 1], n_children = V.cnt[k - 1];
        for (uint32_t t0 = 0; t0 < R.total; t0 += ACCEL_WG) {   // (uniform: every thread meets both barriers)
            const uint32_t t = t0 + threadIdx.x;
            const uint32_t i = t < R.total ? refit_node(R, t) : 0xFFFFFFFFu;
            const bool live = i < V.cnt[k];
            AccelNode N = empty_node();
            if (live) {
                bool wild = false;
                const uint32_t c0 = i * ACCEL_W, c1 = min(c0 + ACCEL_W, n_children);
                for (uint32_t c = c0; c < c1; ++c) {
                    const uint32_t slot = refit_slot(C, c);
                    const AccelNode Ch = slot < C.total ? S[slot] : B.nodes[child_off + c];
                    fold_child(N, wild, Ch);
                }
                close_node(N, wild);
            }
            __syncthreads();
            if (live) {
                S[t] = N;
                B.nodes[V.off[k] + i] = N;
            }
            __syncthreads();
        }
    }
}

// rxr_ray_refresh_verify: words of a[r * stride + i] and b[..] (rows r < rows, i < n) that differ; nodes (8 words) that differ; the
// wild triangles as k_accel_keys counts them
__global__ __launch_bounds__(ACCEL_WG) void k_accel_diff_words(const uint32_t *a, const uint32_t *b, uint32_t n, uint32_t stride, uint32_t rows, unsigned long long *out) {
    const uint32_t i = blockIdx.x * ACCEL_WG + threadIdx.x;
    uint32_t d = 0;
    if (i < n)
        for (uint32_t r = 0; r < rows; ++r) d += a[(size_t)r * stride + i] != b[(size_t)r * stride + i];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) d += __shfl_xor(d, off);
    if (d && __lane_id() == 0) atomicAdd(out, (unsigned long long)d);
}
__global__ __launch_bounds__(ACCEL_WG) void k_accel_diff_nodes(const AccelNode *a, const AccelNode *b, uint32_t n, unsigned long long *out) {
    const uint32_t i = blockIdx.x * ACCEL_WG + threadIdx.x;
    bool differ = false;
    if (i < n) {
        const uint32_t *x = (const uint32_t *)(a + i), *y = (const uint32_t *)(b + i);
        for (int w = 0; w < 8; ++w) differ |= x[w] != y[w];
    }
    const unsigned long long m = __ballot(differ);
    if (m && __lane_id() == 0) atomicAdd(out, (unsigned long long)__popcll(m));
}
__global__ __launch_bounds__(ACCEL_WG) void k_accel_count_wild(AccelBuild B, unsigned long long *out) {
    const uint32_t g = blockIdx.x * ACCEL_WG + threadIdx.x;
    const bool wild = g < B.ntri && tri_info(B, g).wild;
    const unsigned long long w = __ballot(wild);
    if (w && __lane_id() == 0) atomicAdd(out, (unsigned long long)__popcll(w));
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

namespace {

// the resident tree as the build's kernels see it (no build scratch: the refit and the verification read perm, never the keys)
AccelBuild accel_resident(rxr_ctx *ctx) {
    AccelBuild B{};
    B.ntri = ctx->accel_ntri;
    B.n_meshes = (uint32_t)ctx->meshes.size();
    B.stride = ctx->isect_stride;
    B.tin_prefix = ctx->PP.tin_prefix;
    B.vin_prefix = ctx->PP.vin_prefix;
    B.obj_idx = ctx->PP.obj_idx;
    B.obj_verts = ctx->PP.obj_verts;
    B.perm = (const uint32_t *)ctx->d_accel_perm.p;
    B.tris = (float *)ctx->d_accel_tris.p;
    B.nodes = (AccelNode *)ctx->d_accel_nodes.p;
    B.stats = (unsigned long long *)ctx->d_accel_stats.p;
    return B;
}

}  // namespace

RxrRefitLaunch rxr_ray_accel_refit_plan(const rxr_ctx *ctx, const uint32_t *ranges, uint32_t n, std::vector<uint32_t> &table) {
    static_assert(RXR_REFIT_MAX_LEVELS == ACCEL_MAX_LEVELS, "rxr_ray_refresh.h mirrors the tree's shape");
    const RxrRefitPlan P = rxr_refit_plan(ctx->accel_ntri, ACCEL_L, ACCEL_W, ranges, n);
    RxrRefitLaunch R{};
    R.n_levels = P.n_levels;
    for (uint32_t k = 0; k < P.n_levels; ++k) {
        R.off[k] = (uint32_t)table.size();
        R.n_iv[k] = (uint32_t)P.iv[k].size();
        R.total[k] = P.dirty[k];
        for (const RxrRefitInterval &c : P.iv[k]) table.push_back(c.lo);
        uint32_t pre = 0;
        for (const RxrRefitInterval &c : P.iv[k]) {
            table.push_back(pre);
            pre += c.hi - c.lo + 1;
        }
        table.push_back(pre);
    }
    // RXR_RAY_REFIT_SMALL_MAX=<n> in the environment lowers the bound (0: always a launch per level): the sweep of tools/ray_refresh_bench.py
    static const uint32_t small_max = [] {
        const char *e = getenv("RXR_RAY_REFIT_SMALL_MAX");
        return e ? std::min<uint32_t>((uint32_t)strtoul(e, nullptr, 10), RXR_RAY_REFIT_SMALL_MAX) : RXR_RAY_REFIT_SMALL_MAX;
    }();
    R.route = !P.n_levels || !P.dirty[0] ? RXR_RAY_REFIT_NONE : P.dirty[0] <= small_max ? RXR_RAY_REFIT_SMALL : RXR_RAY_REFIT_GENERAL;
    return R;
}

int rxr_ray_accel_refit(rxr_ctx *ctx, const RxrDirtyTris &D, const RxrRefitLaunch &R, const uint32_t *dev_table, hipStream_t s) {
    if (R.route == RXR_RAY_REFIT_NONE) return RXR_OK;
    const AccelBuild B = accel_resident(ctx);
    const AccelLevels V = accel_levels(B.ntri);
    const dim3 wg(ACCEL_WG);
    hipLaunchKernelGGL(k_accel_refresh_records, dim3((D.total + ACCEL_WG - 1) / ACCEL_WG), wg, 0, s, B, D);
    HIPCHK(ctx, hipGetLastError());
    if (R.route == RXR_RAY_REFIT_SMALL) {
        RefitSmall Q{};
        Q.n_levels = R.n_levels;
        for (uint32_t k = 0; k < R.n_levels; ++k) Q.off[k] = R.off[k], Q.n_iv[k] = R.n_iv[k], Q.total[k] = R.total[k];
        hipLaunchKernelGGL(k_accel_refit_small, dim3(1), wg, 0, s, B, V, Q, dev_table);
        HIPCHK(ctx, hipGetLastError());
        return RXR_OK;
    }
    for (uint32_t k = 0; k < R.n_levels; ++k) {
        const RefitLevel L{dev_table + R.off[k], dev_table + R.off[k] + R.n_iv[k], R.n_iv[k], R.total[k]};
        const dim3 grid((L.total + ACCEL_WG - 1) / ACCEL_WG);
        if (k == 0) hipLaunchKernelGGL(k_accel_refit_leaves, grid, wg, 0, s, B, L, V.cnt[0]);
        else hipLaunchKernelGGL(k_accel_refit_level, grid, wg, 0, s, B.nodes, V.off[k - 1], V.cnt[k - 1], V.off[k], V.cnt[k], L);
        HIPCHK(ctx, hipGetLastError());
    }
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

bool rxr_ray_wave_route(const rxr_ctx *ctx, uint32_t nr) {
    if (ctx->wave_mode == RXR_RAY_WAVE_OFF || !nr || !rxr_ray_accel_takes(ctx)) return false;
    return ctx->wave_mode == RXR_RAY_WAVE_FORCE || rxr_ray_wave_takes(nr, ctx->accel_ntri) != 0;
}

int rxr_ray_wave_closest(rxr_ctx *ctx, const void *dev_segs, uint32_t nseg, const float *dev_origins, const float *dev_dirs, uint32_t r0, uint32_t nr,
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
    const uint32_t per_group = ACCEL_WG / 64;   // a wave per ray
    const dim3 grid((nr + per_group - 1) / per_group), wg(ACCEL_WG);
    if (ctx->accel_mode == RXR_RAY_ACCEL_COUNT) hipLaunchKernelGGL(k_accel_by_wave<true>, grid, wg, 0, s, A, r0, nr);
    else hipLaunchKernelGGL(k_accel_by_wave<false>, grid, wg, 0, s, A, r0, nr);
    HIPCHK(ctx, hipGetLastError());
    ++ctx->wave_batches;
    ctx->wave_rays += nr;
    return RXR_OK;
}

extern "C" {

int rxr_set_ray_wave(rxr_ctx *ctx, uint32_t mode) {
    if (!ctx) return RXR_ERR_INVALID;
    if (mode > RXR_RAY_WAVE_FORCE) return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_set_ray_wave: mode must be RXR_RAY_WAVE_OFF, _ON or _FORCE");
    if (ctx->group) return rxr_as_member0(ctx, [&](rxr_ctx *m) { return rxr_set_ray_wave(m, mode); });
    ctx->wave_mode = mode;
    return RXR_OK;
}

int rxr_ray_wave_takes(uint32_t n_rays, uint32_t n_triangles) {
    return n_rays >= RXR_RAY_WAVE_MIN_RAYS && n_rays <= RXR_RAY_WAVE_MAX_RAYS && n_triangles >= RXR_RAY_WAVE_MIN_TRIANGLES;
}

int rxr_ray_wave_info(rxr_ctx *ctx, uint64_t out[RXR_RAY_WAVE_INFO_WORDS]) {
    if (!ctx) return RXR_ERR_INVALID;
    if (!out) return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_ray_wave_info: out is NULL");
    if (ctx->group) return rxr_as_member0(ctx, [&](rxr_ctx *m) { return rxr_ray_wave_info(m, out); });
    out[RXR_RAY_WAVE_INFO_MODE] = ctx->wave_mode;
    out[RXR_RAY_WAVE_INFO_BATCHES] = ctx->wave_batches;
    out[RXR_RAY_WAVE_INFO_RAYS] = ctx->wave_rays;
    return RXR_OK;
}

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
    const bool valid = ctx->isect_ready && ctx->accel_ready && !ctx->refresh_pending;   // (pending: rxr_set_ray_refresh)
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

int rxr_debug_ray_accel_nodes(rxr_ctx *ctx, float *nodes, uint64_t capacity, uint64_t *n_nodes) {
    if (!ctx) return RXR_ERR_INVALID;
    if (!n_nodes) return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_debug_ray_accel_nodes: n_nodes is NULL");
    if (ctx->group) return rxr_as_member0(ctx, [&](rxr_ctx *m) { return rxr_debug_ray_accel_nodes(m, nodes, capacity, n_nodes); });
    static_assert(sizeof(AccelNode) == 32, "eight floats a node");
    *n_nodes = ctx->accel_ready ? ctx->accel_nodes : 0u;
    if (!*n_nodes || !nodes || !capacity) return RXR_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc = rxr_quiesce(ctx);
    if (rc != RXR_OK) return rc;
    HIPCHK(ctx, hipMemcpy(nodes, ctx->d_accel_nodes.p, (size_t)std::min<uint64_t>(*n_nodes, capacity) * sizeof(AccelNode), hipMemcpyDeviceToHost));
    return RXR_OK;
}

int rxr_ray_accel_invalidate(rxr_ctx *ctx) {
    if (!ctx) return RXR_ERR_INVALID;
    if (ctx->group) return rxr_as_member0(ctx, [&](rxr_ctx *m) { return rxr_ray_accel_invalidate(m); });
    ctx->accel_ready = false;
    return RXR_OK;
}

int rxr_ray_refresh_verify(rxr_ctx *ctx, uint64_t out[RXR_RAY_REFRESH_VERIFY_WORDS]) {
    if (!ctx) return RXR_ERR_INVALID;
    if (!out) return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_ray_refresh_verify: out is NULL");
    if (ctx->group) return rxr_as_member0(ctx, [&](rxr_ctx *m) { return rxr_ray_refresh_verify(m, out); });
    for (uint32_t i = 0; i < RXR_RAY_REFRESH_VERIFY_WORDS; ++i) out[i] = 0;
    if (!ctx->meshes_valid || !ctx->isect_ready) return RXR_OK;   // (no records stand: nothing to compare)
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc = rxr_quiesce(ctx);
    if (rc != RXR_OK) return rc;
    const uint32_t ntri = ctx->PP.n_tris_in;
    const size_t stride = ctx->isect_stride;
    const bool tree = ctx->accel_ready && ctx->accel_nodes != 0 && ctx->accel_ntri == ntri;
    out[RXR_RAY_REFRESH_VERIFY_CHECKED] = 1u | (tree ? 2u : 0u);
    if (!ntri) return RXR_OK;
    BlobCursor take;
    const size_t o_cnt = take(64), o_pick = take(9 * stride * 4), o_sorted = take(tree ? 9 * stride * 4 : 0),
                 o_nodes = take(tree ? (size_t)ctx->accel_nodes * sizeof(AccelNode) : 0);
    if ((rc = rxr_ensure(ctx, ctx->d_refresh_verify, take.o)) != RXR_OK) return rc;
    uint8_t *sc = (uint8_t *)ctx->d_refresh_verify.p;
    unsigned long long *cnt = (unsigned long long *)(sc + o_cnt);
    hipStream_t s = ctx->stream;
    const dim3 per_tri((ntri + ACCEL_WG - 1) / ACCEL_WG), wg(ACCEL_WG);
    HIPCHK(ctx, hipMemsetAsync(cnt, 0, 64, s));
    if ((rc = rxr_isect_prep_into(ctx, (float *)(sc + o_pick), s)) != RXR_OK) return rc;
    hipLaunchKernelGGL(k_accel_diff_words, per_tri, wg, 0, s, (const uint32_t *)ctx->d_isect_tris.p, (const uint32_t *)(sc + o_pick), ntri, (uint32_t)stride, 9u, cnt);
    HIPCHK(ctx, hipGetLastError());
    if (tree) {
        AccelBuild B = accel_resident(ctx);
        const AccelLevels V = accel_levels(ntri);
        hipLaunchKernelGGL(k_accel_count_wild, per_tri, wg, 0, s, B, cnt + 3);
        HIPCHK(ctx, hipGetLastError());
        B.tris = (float *)(sc + o_sorted);
        B.nodes = (AccelNode *)(sc + o_nodes);
        hipLaunchKernelGGL(k_accel_records, per_tri, wg, 0, s, B);
        HIPCHK(ctx, hipGetLastError());
        hipLaunchKernelGGL(k_accel_leaves, dim3((V.cnt[0] + ACCEL_WG - 1) / ACCEL_WG), wg, 0, s, B, V.cnt[0]);
        HIPCHK(ctx, hipGetLastError());
        for (uint32_t k = 1; k < V.n; ++k) {
            hipLaunchKernelGGL(k_accel_level, dim3((V.cnt[k] + ACCEL_WG - 1) / ACCEL_WG), wg, 0, s, B.nodes, V.off[k - 1], V.cnt[k - 1], V.off[k], V.cnt[k]);
            HIPCHK(ctx, hipGetLastError());
        }
        hipLaunchKernelGGL(k_accel_diff_words, per_tri, wg, 0, s, (const uint32_t *)ctx->d_accel_tris.p, (const uint32_t *)B.tris, ntri, (uint32_t)stride, 9u, cnt + 1);
        HIPCHK(ctx, hipGetLastError());
        hipLaunchKernelGGL(k_accel_diff_nodes, dim3((ctx->accel_nodes + ACCEL_WG - 1) / ACCEL_WG), wg, 0, s, (const AccelNode *)ctx->d_accel_nodes.p, (const AccelNode *)B.nodes,
                           ctx->accel_nodes, cnt + 2);
        HIPCHK(ctx, hipGetLastError());
    }
    unsigned long long h[4] = {0, 0, 0, 0};
    HIPCHK(ctx, hipMemcpyAsync(h, cnt, 32, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    out[RXR_RAY_REFRESH_VERIFY_PICK_WORDS] = h[0];
    out[RXR_RAY_REFRESH_VERIFY_SORTED_WORDS] = h[1];
    out[RXR_RAY_REFRESH_VERIFY_NODES] = h[2];
    out[RXR_RAY_REFRESH_VERIFY_WILD] = h[3];
    return RXR_OK;
}

}  // extern "C"
