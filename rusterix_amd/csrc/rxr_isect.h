// rxr_isect.h -- what the path tracer (rxr_trace.hip) shares with the ray picking of rxr_intersect.hip: the vek arithmetic and
// Batch3D::intersect's triangle test as device functions, and the host entry points that build the resident triangle records and run
// the closest-hit kernels over a segment table of the caller's.  Private to those two files.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

struct rxr_ctx;

namespace isect {

struct F3 {
    float x, y, z;
};
__device__ __forceinline__ F3 sub3(F3 a, F3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ float dot3(F3 a, F3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ F3 cross3(F3 a, F3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ F3 normalized3(F3 a) {
    const float m = sqrtf(dot3(a, a));
    return {a.x / m, a.y / m, a.z / m};
}
__device__ __forceinline__ F3 load3(const float *p, uint64_t i) { return {p[3 * i], p[3 * i + 1], p[3 * i + 2]}; }

// Batch3D::intersect's test of one triangle (batch3d.rs:870-897); true: accepted, with its t (and u, v)
__device__ __forceinline__ bool mt_test(F3 o, F3 d, F3 p0, F3 e1, F3 e2, float &t, float &u, float &v) {
    const F3 h = cross3(d, e2);
    const float a = dot3(e1, h);
    if (fabsf(a) < 1e-6f) return false;
    const float f = 1.0f / a;
    const F3 s = sub3(o, p0);
    u = f * dot3(s, h);
    if (!(u >= 0.0f && u <= 1.0f)) return false;
    const F3 q = cross3(s, e1);
    v = f * dot3(d, q);
    if (v < 0.0f || u + v > 1.0f) return false;
    t = f * dot3(e2, q);
    return t > 1e-4f;
}

// last index i in [lo, hi) with a[i] <= x (a non-decreasing, a[lo] <= x)
__device__ __forceinline__ uint32_t last_le(const uint32_t *a, uint32_t lo, uint32_t hi, uint32_t x) {
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (a[mid] <= x) lo = mid;
        else hi = mid;
    }
    return lo;
}

}  // namespace isect

// A segment of the closest-hit kernels: six words, global triangles [begin, end) of meshes [mesh0, mesh1), the fold's rule and a
// profile id.  The segments of a table are in triangle order and cover every registered triangle; a segment is never empty.
#define RXR_ISECT_SEG_WORDS 6u
#define RXR_ISECT_NO_HIT (~0ull)

// the (p0, edge1, edge2) records of the current meshes (ctx->d_isect_tris, ctx->isect_stride), built once per rxr_set_meshes; queued
// on `s` inside the picking lane (the caller has ordered `s` behind it)
int rxr_isect_prepare(rxr_ctx *ctx, hipStream_t s);
// the largest number of rays rxr_isect_closest takes at once for a table of nseg segments (a multiple of a workgroup)
uint32_t rxr_isect_batch_rays(uint32_t n_rays, uint32_t nseg);
// keys[(r - r0) * nseg + s] for rays r0 .. r0 + nr of origins / dirs [..][3] (device memory): the minimum of (t's bits << 32 | global
// triangle) over segment s's triangles that Batch3D::intersect accepts, RXR_ISECT_NO_HIT for none -- the kernels of rxr_intersect,
// with its choice between a thread per triangle and a thread per ray, over the table dev_segs.  Queued on `s`.
int rxr_isect_closest(rxr_ctx *ctx, const void *dev_segs, uint32_t nseg, const float *dev_origins, const float *dev_dirs, uint32_t r0,
                      uint32_t nr, unsigned long long *dev_keys, hipStream_t s);

// ---- rxr_ray_accel.hip: the opt-in box tree behind rxr_isect_closest's many-ray path (rxr_set_ray_accel, include/rxr.h) -----------
#ifndef RXR_RAY_ACCEL_LEAF               // (-D: the A-B runs of profiles/ray_accel/README.md)
#define RXR_RAY_ACCEL_LEAF 8u            // sorted positions per leaf
#endif
#ifndef RXR_RAY_ACCEL_WIDTH
#define RXR_RAY_ACCEL_WIDTH 8u           // nodes per parent
#endif
#define RXR_RAY_ACCEL_KAPPA_CAP 4096.0f  // a triangle whose |e1| |e2| / |e1 x e2| is above it is always tested
#define RXR_RAY_ACCEL_C 4096.0f          // the pad's constant (tests/ray_accel_ref.py measures it; profiles/ray_accel/README.md)
// the tree over the current meshes, queued on `s` behind the records of rxr_isect_prepare (which calls it while the mode is on)
int rxr_ray_accel_build(rxr_ctx *ctx, hipStream_t s);
// does rxr_isect_closest's many-ray path go through the tree?
bool rxr_ray_accel_takes(const rxr_ctx *ctx);
// the start of a picking or tracing call: the count of RXR_RAY_ACCEL_COUNT starts again
int rxr_ray_accel_begin_call(rxr_ctx *ctx, hipStream_t s);
// ---- a wave per ray through the same tree (rxr_set_ray_wave) -------------------------------------------------
// The rule of RXR_RAY_WAVE_ON, rxr_ray_wave_takes(n_rays, n_triangles): RXR_RAY_WAVE_MIN_RAYS <= n_rays <= RXR_RAY_WAVE_MAX_RAYS and
// n_triangles >= RXR_RAY_WAVE_MIN_TRIANGLES.  The ray bounds are the measured ray counts between which the wave walk's median was ahead
// of the better of brute force and the thread walk by more than twice the larger spread on every scene of profiles/ray_wave/README.md
// (at 64 rays and at 1920 x 1080 it is not); the triangle bound is the smallest measured scene above the teapot's 2 256 triangles,
// which stays with the existing routes whatever the ray count.
#define RXR_RAY_WAVE_MIN_RAYS 256u
#define RXR_RAY_WAVE_MAX_RAYS 65536u
#define RXR_RAY_WAVE_MIN_TRIANGLES 12288u
// does this batch of nr rays go a wave per ray?  (rxr_isect_closest asks ahead of its own two routes)
bool rxr_ray_wave_route(const rxr_ctx *ctx, uint32_t nr);
// rxr_isect_closest's keys, a wave per ray through the tree (k_accel_by_wave)
int rxr_ray_wave_closest(rxr_ctx *ctx, const void *dev_segs, uint32_t nseg, const float *dev_origins, const float *dev_dirs, uint32_t r0,
                         uint32_t nr, unsigned long long *dev_keys, hipStream_t s);
// ---- the ranged refresh after rxr_update_meshes (rxr_set_ray_refresh) -----------------------------------------
// The dirty triangles of a refresh, as the kernels of both files read them: per dirty mesh (in mesh order, none empty) its first global
// triangle = its first sorted position, its first vertex in the pools, and the prefix of the dirty meshes' triangle counts
// (pre[n] = total).  Device memory.
struct RxrDirtyTris {
    const uint32_t *base, *vbase, *pre;
    uint32_t n, total;
};
// A refit's node intervals inside the refresh table (word offsets; rxr_ray_refresh.h computes the intervals): per level n_iv[k] first
// nodes at off[k] and n_iv[k] + 1 prefix counts behind them; total[k] dirty nodes.
struct RxrRefitLaunch {
    uint32_t route, n_levels;    // RXR_RAY_REFIT_*
    uint32_t off[24], n_iv[24], total[24];
};
// appends the intervals above the position ranges (n pairs begin, end; increasing) to `table` and chooses the route; nothing is queued
RxrRefitLaunch rxr_ray_accel_refit_plan(const rxr_ctx *ctx, const uint32_t *ranges, uint32_t n, std::vector<uint32_t> &table);
// the dirty positions' sorted records (the wild count kept exact), then the leaves and levels of `R`, over the uploaded table; on `s`
int rxr_ray_accel_refit(rxr_ctx *ctx, const RxrDirtyTris &D, const RxrRefitLaunch &R, const uint32_t *dev_table, hipStream_t s);
// k_isect_prep over every registered triangle into `out` (nine arrays, ctx->isect_stride apart), on `s`: rxr_ray_refresh_verify
int rxr_isect_prep_into(rxr_ctx *ctx, float *out, hipStream_t s);
// rxr_isect_closest's keys for more than a few rays, through the tree
int rxr_ray_accel_closest(rxr_ctx *ctx, const void *dev_segs, uint32_t nseg, const float *dev_origins, const float *dev_dirs, uint32_t r0,
                          uint32_t nr, unsigned long long *dev_keys, hipStream_t s);
