// rxr_intersect.hip -- ray picking on the resident meshes: Scene::intersect (src/scene.rs:216-276) over the batches registered by
// rxr_set_meshes, and the screen rays of Rasterizer::screen_ray (src/rasterizer.rs:1843-1870).  include/rxr.h: rxr_intersect,
// rxr_intersect_to, rxr_screen_rays_to.
//
// Semantics (exact, bit for bit):
//   * per mesh, Batch3D::intersect (src/batch/batch3d.rs:844-948): local_dir = dir.normalized(); the triangles in index order,
//     Moeller-Trumbore on the OBJECT-SPACE vertices[..][0..3] -- transform_3d is ignored, as in the reference;
//     edge1 = p1-p0, edge2 = p2-p0, h = cross(local_dir, edge2), a = dot(edge1, h); reject |a| < 1e-6; f = 1/a, s = origin-p0,
//     u = f*dot(s,h), reject unless 0 <= u <= 1 (NaN rejects); q = cross(s, edge1), v = f*dot(local_dir, q), reject v < 0 or
//     u+v > 1 (a NaN v does NOT reject); t = f*dot(edge2, q), accepted if t > 1e-4; the closest hit by a strict `<`, so on equal t
//     the earliest triangle;
//   * the scene fold (scene.rs:216-276), meshes in rxr_set_meshes order (= chunk opacity / chunk / terrain per chunk, then static,
//     dynamic, overlay: the order the host mirror registers them in): best t starts at f32::MAX without a profile id;
//     RXR_LIST_CHUNK_OPACITY / _CHUNK_TERRAIN / _STATIC / _DYNAMIC replace the best if hit.t < best.t; RXR_LIST_CHUNK the same
//     except that a hit whose profile id equals the best's keeps the best; RXR_LIST_OVERLAY: any hit replaces the best;
//   * hitpoint = origin + dir*t with the UN-normalised dir (Ray::at, src/tracer/mod.rs:30-32); full mode (RXR_INTERSECT_FULL,
//     Batch3D::intersect(ray, false), batch3d.rs:906-940): uv = w*uv0 + u*uv1 + v*uv2 with w = (1-u)-v, normal =
//     (n0*w + n1*u + n2*v).normalized(), negated if dot(normal, dir) > 0.  (Registered meshes always carry normals, so the
//     reference's cross-product fallback for batches without normals never applies here.)
//   * vek conventions (include/rusterix_vek.hpp): dot = (x*x' + y*y') + z*z', its cross, normalized = v / sqrt(dot(v,v)) (three
//     divisions); Mat4 * Vec4 with mul_add.  Division and sqrt are the compiler's correctly rounded ones, nothing is contracted
//     (-ffp-contract=off), f32 subnormals are kept; no early-out runs ahead of the exact division.
//
// Device layout: per registered triangle, in global (mesh-order) index, the record (p0, edge1, edge2) as nine SoA arrays
// (d_isect_tris, built by k_isect_prep from the resident pools on the first intersect after each rxr_set_meshes; every value is one
// subtraction or a copy, so it is bit-identical to what the test computes).  Consecutive meshes are grouped into segments: a run of
// plain-rule meshes (and chunk meshes without a profile id) folds to ONE lexicographic minimum of (t, global triangle index) -- t is
// positive, so that minimum is a single 64-bit key (t's bits high, the index low) merged with atomicMin; a chunk mesh with a
// profile id and every overlay mesh is a segment of its own.  k_isect_by_tri (few rays: a thread per triangle, the rays uniform,
// one atomic per wave and segment) or k_isect_by_ray (many rays: a thread per ray, triangle chunks staged in LDS, the triangle
// range split across workgroups) fills the keys of a batch of rays; k_isect_fold then walks each ray's segments in order with the
// rules above and writes the outputs (full mode: it runs the winner's test again for u and v -- the same operations, the same bits).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/rusterix_vek.hpp"  // (RXR_VEK_FUSED_MATVEC: the screen rays' Mat4 * Vec4 follows the host's choice)
#include "rxr_isect.h"
#include "rxr_query.h"

namespace {

constexpr uint32_t ISECT_WG = 256;
constexpr uint32_t ISECT_FEW_RAYS = 64;             // up to this many rays in a batch: a thread per triangle
constexpr uint32_t ISECT_RAYS_PER_Y = 8;            // ... each workgroup row of k_isect_by_tri tests this many rays
constexpr uint64_t ISECT_KEYS_MAX = 8ull << 20;     // keys (8 B) of one batch of rays: 64 MiB of scratch -- more only beyond 32 768 segments,
                                                    // where a batch stays at ISECT_WG rays (ISECT_WG * nseg keys: 67.6 MB at 33 000 segments)
constexpr unsigned long long NO_HIT = ~0ull;

enum : uint32_t { SEG_PLAIN = 0, SEG_CHUNK_PID = 1, SEG_OVERLAY = 2 };

// a run of consecutive meshes: global triangles [begin, end), meshes [mesh0, mesh1)
struct IsectSeg {
    uint32_t begin, end, mesh0, mesh1, rule, pid;
};

struct IsectArgs {
    uint32_t ntri, nseg, stride;       // stride: elements between two of the nine SoA arrays of `tris`
    const float *tris;                 // p0.xyz, edge1.xyz, edge2.xyz
    const IsectSeg *segs;
    const uint32_t *mesh_pid;          // per mesh: has_profile_id, profile_id
    const uint32_t *tin_prefix, *vin_prefix;
    const uint32_t *obj_idx;
    const float4 *obj_verts;
    const float2 *obj_uvs;
    const float *obj_normals;
    const float *origins, *dirs;       // [n][3]
    unsigned long long *keys;          // [rays of the batch][nseg]
};

using namespace isect;   // F3 and its vek arithmetic, mt_test (Batch3D::intersect's triangle test), last_le: rxr_isect.h

__device__ __forceinline__ void load_tri(const IsectArgs &A, uint32_t g, F3 &p0, F3 &e1, F3 &e2) {
    const float *p = A.tris + g;
    const size_t s = A.stride;
    p0 = {p[0], p[s], p[2 * s]};
    e1 = {p[3 * s], p[4 * s], p[5 * s]};
    e2 = {p[6 * s], p[7 * s], p[8 * s]};
}

__device__ __forceinline__ uint32_t seg_of(const IsectArgs &A, uint32_t g) {
    uint32_t lo = 0, hi = A.nseg;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (A.segs[mid].begin <= g) lo = mid;
        else hi = mid;
    }
    return lo;
}

// one-time per rxr_set_meshes: the (p0, edge1, edge2) record of every registered triangle
__global__ __launch_bounds__(ISECT_WG) void k_isect_prep(IsectArgs A, uint32_t n_meshes, float *out) {
    const uint32_t g = blockIdx.x * ISECT_WG + threadIdx.x;
    if (g >= A.ntri) return;
    const uint32_t m = last_le(A.tin_prefix, 0, n_meshes, g);
    const uint32_t vb = A.vin_prefix[m];
    const float4 v0 = A.obj_verts[vb + A.obj_idx[3ull * g]];
    const float4 v1 = A.obj_verts[vb + A.obj_idx[3ull * g + 1]];
    const float4 v2 = A.obj_verts[vb + A.obj_idx[3ull * g + 2]];
    const size_t s = A.stride;
    float *p = out + g;
    p[0] = v0.x, p[s] = v0.y, p[2 * s] = v0.z;
    p[3 * s] = v1.x - v0.x, p[4 * s] = v1.y - v0.y, p[5 * s] = v1.z - v0.z;
    p[6 * s] = v2.x - v0.x, p[7 * s] = v2.y - v0.y, p[8 * s] = v2.z - v0.z;
}

// few rays: a thread per triangle, the rays of this workgroup row uniform; per ray and wave one min over the lanes' keys and
// one atomic when the wave's hits lie in one segment (else one per hitting lane)
__global__ __launch_bounds__(ISECT_WG) void k_isect_by_tri(IsectArgs A, uint32_t r0, uint32_t nr) {
    const uint32_t g = blockIdx.x * ISECT_WG + threadIdx.x;
    const bool live = g < A.ntri;
    F3 p0{}, e1{}, e2{};
    uint32_t seg = 0;
    if (live) {
        load_tri(A, g, p0, e1, e2);
        seg = seg_of(A, g);
    }
    const uint32_t ra = blockIdx.y * ISECT_RAYS_PER_Y, rb = min(ra + ISECT_RAYS_PER_Y, nr);
    for (uint32_t r = ra; r < rb; ++r) {
        const F3 o = load3(A.origins, (uint64_t)r0 + r);
        const F3 d = normalized3(load3(A.dirs, (uint64_t)r0 + r));
        float t, u, v;
        const bool hit = live && mt_test(o, d, p0, e1, e2, t, u, v);
        const unsigned long long hits = __ballot(hit);
        if (!hits) continue;
        unsigned long long key = hit ? (((unsigned long long)__float_as_uint(t) << 32) | g) : NO_HIT;
        const uint32_t ref = __shfl(seg, (int)(__ffsll((long long)hits) - 1));
        unsigned long long *slot = A.keys + (uint64_t)r * A.nseg;
        if (__all(!hit || seg == ref)) {
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                const unsigned long long o2 = __shfl_xor(key, off);
                key = o2 < key ? o2 : key;
            }
            if (__lane_id() == 0) atomicMin(slot + ref, key);
        } else if (hit) {
            atomicMin(slot + seg, key);
        }
    }
}

// many rays: a thread per ray; workgroup row y tests triangles [y*slice, (y+1)*slice) staged through LDS, 256 at a time, and
// merges each segment's minimum into the keys with one atomic per ray and segment
__global__ __launch_bounds__(ISECT_WG) void k_isect_by_ray(IsectArgs A, uint32_t r0, uint32_t nr, uint32_t slice) {
    __shared__ float4 L[3 * ISECT_WG];
    const uint32_t r = blockIdx.x * ISECT_WG + threadIdx.x;
    const bool active = r < nr;
    F3 o{}, d{};
    if (active) {
        o = load3(A.origins, (uint64_t)r0 + r);
        d = normalized3(load3(A.dirs, (uint64_t)r0 + r));
    }
    const uint32_t tb = blockIdx.y * slice;
    if (tb >= A.ntri) return;  // (uniform for the workgroup)
    const uint32_t te = min(tb + slice, A.ntri);
    uint32_t s = seg_of(A, tb), send = A.segs[s].end;
    uint32_t best_t = 0xFFFFFFFFu, best_g = 0;  // t's bits: t > 1e-4 (+inf included) orders like its unsigned bits
    unsigned long long *slot = A.keys + (uint64_t)r * A.nseg;
    for (uint32_t c = tb; c < te; c += ISECT_WG) {
        __syncthreads();
        if (c + threadIdx.x < te) {
            F3 p0, e1, e2;
            load_tri(A, c + threadIdx.x, p0, e1, e2);
            L[3 * threadIdx.x] = make_float4(p0.x, p0.y, p0.z, e1.x);
            L[3 * threadIdx.x + 1] = make_float4(e1.y, e1.z, e2.x, e2.y);
            L[3 * threadIdx.x + 2] = make_float4(e2.z, 0.0f, 0.0f, 0.0f);
        }
        __syncthreads();
        const uint32_t m = min(ISECT_WG, te - c);
        for (uint32_t j = 0; j < m; ++j) {
            const uint32_t gi = c + j;
            if (gi == send) {  // segments are never empty: one step
                if (active && best_t != 0xFFFFFFFFu) atomicMin(slot + s, ((unsigned long long)best_t << 32) | best_g);
                best_t = 0xFFFFFFFFu;
                ++s;
                send = A.segs[s].end;
            }
            const float4 a = L[3 * j], b = L[3 * j + 1], cc = L[3 * j + 2];
            float t, u, v;
            if (mt_test(o, d, {a.x, a.y, a.z}, {a.w, b.x, b.y}, {b.z, b.w, cc.x}, t, u, v)) {
                const uint32_t tbits = __float_as_uint(t);
                if (tbits < best_t) {
                    best_t = tbits;
                    best_g = gi;
                }
            }
        }
    }
    if (active && best_t != 0xFFFFFFFFu) atomicMin(slot + s, ((unsigned long long)best_t << 32) | best_g);
}

struct IsectOut {
    float *t;
    uint32_t *mesh, *tri;
    float *hitpoint, *uv, *normal;
    uint32_t full;
};

// Scene::intersect's fold over one ray's segments (scene.rs:216-276) and the outputs
__global__ __launch_bounds__(ISECT_WG) void k_isect_fold(IsectArgs A, uint32_t r0, uint32_t nr, IsectOut O) {
    const uint32_t r = blockIdx.x * ISECT_WG + threadIdx.x;
    if (r >= nr) return;
    const uint64_t ray = (uint64_t)r0 + r;
    float bt = FLT_MAX;
    uint32_t bm = 0xFFFFFFFFu, bg = 0, bhas = 0, bpid = 0;
    const unsigned long long *slot = A.keys + (uint64_t)r * A.nseg;
    for (uint32_t s = 0; s < A.nseg; ++s) {
        const unsigned long long key = slot[s];
        if (key == NO_HIT) continue;
        const float t = __uint_as_float((uint32_t)(key >> 32));
        const uint32_t g = (uint32_t)key;
        const IsectSeg S = A.segs[s];
        const bool replace = S.rule == SEG_OVERLAY || (t < bt && !(S.rule == SEG_CHUNK_PID && bhas && bpid == S.pid));
        if (replace) {
            bm = last_le(A.tin_prefix, S.mesh0, S.mesh1, g);
            bt = t;
            bg = g;
            bhas = A.mesh_pid[2 * bm];
            bpid = A.mesh_pid[2 * bm + 1];
        }
    }
    const bool hit = bm != 0xFFFFFFFFu;
    O.t[ray] = bt;
    O.mesh[ray] = bm;
    O.tri[ray] = hit ? bg - A.tin_prefix[bm] : 0u;
    const F3 o = load3(A.origins, ray), dir = load3(A.dirs, ray);
    if (O.hitpoint) {
        F3 hp{0.0f, 0.0f, 0.0f};
        if (hit) hp = {o.x + dir.x * bt, o.y + dir.y * bt, o.z + dir.z * bt};
        O.hitpoint[3 * ray] = hp.x, O.hitpoint[3 * ray + 1] = hp.y, O.hitpoint[3 * ray + 2] = hp.z;
    }
    if (!O.full || (!O.uv && !O.normal)) return;
    float uvx = 0.0f, uvy = 0.0f;
    F3 n{0.0f, 0.0f, 0.0f};
    if (hit) {
        F3 p0, e1, e2;
        load_tri(A, bg, p0, e1, e2);
        float t, u = 0.0f, v = 0.0f;
        (void)mt_test(o, normalized3(dir), p0, e1, e2, t, u, v);  // (accepted: the key came from this very test)
        const float w = (1.0f - u) - v;
        const uint32_t vb = A.vin_prefix[bm];
        const uint32_t i0 = vb + A.obj_idx[3ull * bg], i1 = vb + A.obj_idx[3ull * bg + 1], i2 = vb + A.obj_idx[3ull * bg + 2];
        const float2 uv0 = A.obj_uvs[i0], uv1 = A.obj_uvs[i1], uv2 = A.obj_uvs[i2];
        uvx = (w * uv0.x + u * uv1.x) + v * uv2.x;
        uvy = (w * uv0.y + u * uv1.y) + v * uv2.y;
        const F3 n0 = load3(A.obj_normals, i0), n1 = load3(A.obj_normals, i1), n2 = load3(A.obj_normals, i2);
        n = normalized3({(n0.x * w + n1.x * u) + n2.x * v, (n0.y * w + n1.y * u) + n2.y * v, (n0.z * w + n1.z * u) + n2.z * v});
        if (dot3(n, dir) > 0.0f) n = {-n.x, -n.y, -n.z};
    }
    if (O.uv) O.uv[2 * ray] = uvx, O.uv[2 * ray + 1] = uvy;
    if (O.normal) O.normal[3 * ray] = n.x, O.normal[3 * ray + 1] = n.y, O.normal[3 * ray + 2] = n.z;
}

struct ScreenRayArgs {
    float iv[16], ip[16];   // inverse view / inverse projection, column-major
    float width, height;
    uint32_t x0, y0, w;
    uint64_t n;
    float *origins, *dirs;
};

__device__ __forceinline__ float vek_madd(float a, float b, float c) {
#if RXR_VEK_FUSED_MATVEC
    return fmaf(a, b, c);
#else
    return a * b + c;
#endif
}
__device__ __forceinline__ float4 mat_vec(const float *m, float4 v) {
    float o[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        float acc = m[r] * v.x;
        acc = vek_madd(m[4 + r], v.y, acc);
        acc = vek_madd(m[8 + r], v.z, acc);
        acc = vek_madd(m[12 + r], v.w, acc);
        o[r] = acc;
    }
    return make_float4(o[0], o[1], o[2], o[3]);
}
__device__ __forceinline__ float4 div4(float4 a, float s) { return make_float4(a.x / s, a.y / s, a.z / s, a.w / s); }

// Rasterizer::screen_ray (rasterizer.rs:1843-1870) for pixel (x0 + i % w, y0 + i / w)
__global__ __launch_bounds__(ISECT_WG) void k_screen_rays(ScreenRayArgs S) {
    const uint64_t i = (uint64_t)blockIdx.x * ISECT_WG + threadIdx.x;
    if (i >= S.n) return;
    const float x = (float)(S.x0 + (uint32_t)(i % S.w)), y = (float)(S.y0 + (uint32_t)(i / S.w));
    const float ndc_x = 2.0f * (x / S.width) - 1.0f;
    const float ndc_y = 1.0f - 2.0f * (y / S.height);
    float4 vn = mat_vec(S.ip, make_float4(ndc_x, ndc_y, -1.0f, 1.0f));
    float4 vf = mat_vec(S.ip, make_float4(ndc_x, ndc_y, 1.0f, 1.0f));
    vn = div4(vn, vn.w);
    vf = div4(vf, vf.w);
    const float4 wn = mat_vec(S.iv, vn), wf = mat_vec(S.iv, vf);
    const F3 d = normalized3({wf.x - wn.x, wf.y - wn.y, wf.z - wn.z});
    S.origins[3 * i] = wn.x, S.origins[3 * i + 1] = wn.y, S.origins[3 * i + 2] = wn.z;
    S.dirs[3 * i] = d.x, S.dirs[3 * i + 1] = d.y, S.dirs[3 * i + 2] = d.z;
}

// after rxr_update_meshes under RXR_RAY_REFRESH_RANGED: the same record for the triangles of the dirty meshes alone, a thread each
// (k_isect_prep's operations on the same operands: the same bits)
__global__ __launch_bounds__(ISECT_WG) void k_isect_refresh(IsectArgs A, RxrDirtyTris D, float *out) {
    const uint32_t t = blockIdx.x * ISECT_WG + threadIdx.x;
    if (t >= D.total) return;
    const uint32_t i = last_le(D.pre, 0, D.n, t);
    const uint32_t g = D.base[i] + (t - D.pre[i]);
    if (g >= A.ntri) return;   // (a table that went wrong must not write out of bounds)
    const uint32_t vb = D.vbase[i];
    const float4 v0 = A.obj_verts[vb + A.obj_idx[3ull * g]];
    const float4 v1 = A.obj_verts[vb + A.obj_idx[3ull * g + 1]];
    const float4 v2 = A.obj_verts[vb + A.obj_idx[3ull * g + 2]];
    const size_t s = A.stride;
    float *p = out + g;
    p[0] = v0.x, p[s] = v0.y, p[2 * s] = v0.z;
    p[3 * s] = v1.x - v0.x, p[4 * s] = v1.y - v0.y, p[5 * s] = v1.z - v0.z;
    p[6 * s] = v2.x - v0.x, p[7 * s] = v2.y - v0.y, p[8 * s] = v2.z - v0.z;
}

// RXR_RAY_REFRESH_RANGED: the records of the meshes that updates named since the last query, rewritten in place, and the tree above
// them refitted (or dropped while its mode is off); queued on `s`.  The segments and profile ids depend on counts and lists alone,
// which an update cannot change.
int isect_refresh(rxr_ctx *ctx, hipStream_t s) {
    const uint32_t n_meshes = (uint32_t)ctx->meshes.size();
    std::vector<uint32_t> &h = ctx->refresh_host;
    h.clear();
    std::vector<uint32_t> ranges, vbase;
    for (uint32_t m = 0; m < n_meshes && m < ctx->refresh_named.size(); ++m) {
        const DevMesh &M = ctx->meshes[m].dev;
        if (!ctx->refresh_named[m] || !M.n_tris) continue;
        ranges.push_back(M.tin_base);
        ranges.push_back(M.tin_base + M.n_tris);
        vbase.push_back(M.vin_base);
    }
    ctx->refresh_named.clear();
    ctx->refresh_pending = 0;
    const uint32_t nd = (uint32_t)vbase.size();
    uint32_t total = 0;
    for (uint32_t i = 0; i < nd; ++i) h.push_back(ranges[2 * i]);
    h.insert(h.end(), vbase.begin(), vbase.end());
    for (uint32_t i = 0; i < nd; ++i) {
        h.push_back(total);
        total += ranges[2 * i + 1] - ranges[2 * i];
    }
    h.push_back(total);
    const bool tree = ctx->accel_ready && ctx->accel_nodes != 0;
    const bool refit = tree && ctx->accel_mode != RXR_RAY_ACCEL_OFF && total != 0;
    if (ctx->accel_ready && ctx->accel_mode == RXR_RAY_ACCEL_OFF) ctx->accel_ready = false;   // (mode off pays nothing; the next switch-on builds)
    RxrRefitLaunch R{};
    if (refit) R = rxr_ray_accel_refit_plan(ctx, ranges.data(), nd, h);
    ++ctx->refresh_count;
    ctx->refresh_last_tris = total;
    ctx->refresh_last_leaves = refit ? R.total[0] : 0u;
    ctx->refresh_last_nodes = 0;
    for (uint32_t k = 0; refit && k < R.n_levels; ++k) ctx->refresh_last_nodes += R.total[k];
    ctx->refresh_last_route = R.route;
    if (!total) return RXR_OK;
    int rc;
    if ((rc = rxr_ensure(ctx, ctx->d_refresh_table, h.size() * 4)) != RXR_OK) return rc;
    HIPCHK(ctx, hipMemcpyAsync(ctx->d_refresh_table.p, h.data(), h.size() * 4, hipMemcpyHostToDevice, s));
    const uint32_t *tab = (const uint32_t *)ctx->d_refresh_table.p;
    const RxrDirtyTris D{tab, tab + nd, tab + 2 * (size_t)nd, nd, total};
    IsectArgs A{};
    A.ntri = ctx->PP.n_tris_in;
    A.stride = ctx->isect_stride;
    A.obj_idx = ctx->PP.obj_idx;
    A.obj_verts = ctx->PP.obj_verts;
    hipLaunchKernelGGL(k_isect_refresh, dim3((total + ISECT_WG - 1) / ISECT_WG), dim3(ISECT_WG), 0, s, A, D, (float *)ctx->d_isect_tris.p);
    HIPCHK(ctx, hipGetLastError());
    if (!refit) return RXR_OK;
    ++ctx->refit_count;
    return rxr_ray_accel_refit(ctx, D, R, tab, s);
}

// the segments and per-triangle records of the current meshes (once per rxr_set_meshes), queued on `s`
int isect_prepare(rxr_ctx *ctx, hipStream_t s) {
    const bool want_accel = ctx->accel_mode != RXR_RAY_ACCEL_OFF;   // (the box tree of rxr_ray_accel.hip: built with the records, or when switched on)
    if (ctx->isect_ready) {
        int rc = ctx->refresh_pending ? isect_refresh(ctx, s) : RXR_OK;
        if (rc != RXR_OK) {
            ctx->isect_ready = false;   // (the set is gone and the records are stale: the next query takes the full path)
            return rc;
        }
        return want_accel && !ctx->accel_ready ? rxr_ray_accel_build(ctx, s) : RXR_OK;
    }
    ctx->refresh_named.clear();
    ctx->refresh_pending = 0;
    ctx->accel_ready = false;
    const uint32_t n_meshes = (uint32_t)ctx->meshes.size();
    std::vector<uint32_t> &h = ctx->isect_host;
    h.clear();
    // segments (IsectSeg, six words each) first, then the per-mesh profile ids
    uint32_t nseg = 0;
    for (uint32_t m = 0; m < n_meshes; ++m) {
        const HostMesh &M = ctx->meshes[m];
        if (!M.dev.n_tris) continue;  // (no hit: nothing to fold, and no reason to end a run)
        const uint32_t rule = M.list == RXR_LIST_OVERLAY ? SEG_OVERLAY : (M.list == RXR_LIST_CHUNK && M.has_profile_id) ? SEG_CHUNK_PID : SEG_PLAIN;
        if (rule == SEG_PLAIN && nseg && h[6 * (nseg - 1) + 4] == SEG_PLAIN) {
            h[6 * (nseg - 1) + 1] = M.dev.tin_base + M.dev.n_tris;
            h[6 * (nseg - 1) + 3] = m + 1;
            continue;
        }
        const uint32_t seg[6] = {M.dev.tin_base, M.dev.tin_base + M.dev.n_tris, m, m + 1, rule, M.profile_id};
        h.insert(h.end(), seg, seg + 6);
        ++nseg;
    }
    const size_t off_pid = h.size();
    for (uint32_t m = 0; m < n_meshes; ++m) {
        h.push_back(ctx->meshes[m].has_profile_id ? 1u : 0u);
        h.push_back(ctx->meshes[m].profile_id);
    }
    h.push_back(0u);  // (never empty)
    const uint32_t ntri = ctx->PP.n_tris_in;
    const size_t stride = ((size_t)ntri + 63) / 64 * 64;
    int rc;
    if ((rc = rxr_ensure(ctx, ctx->d_isect_misc, h.size() * 4)) != RXR_OK) return rc;
    if ((rc = rxr_ensure(ctx, ctx->d_isect_tris, std::max<size_t>(9 * stride * 4, 256))) != RXR_OK) return rc;
    HIPCHK(ctx, hipMemcpyAsync(ctx->d_isect_misc.p, h.data(), h.size() * 4, hipMemcpyHostToDevice, s));
    ctx->isect_nseg = nseg;
    ctx->isect_off_pid = off_pid;
    ctx->isect_stride = (uint32_t)stride;
    if (ntri) {
        IsectArgs A{};
        A.ntri = ntri;
        A.stride = (uint32_t)stride;
        A.tin_prefix = ctx->PP.tin_prefix;
        A.vin_prefix = ctx->PP.vin_prefix;
        A.obj_idx = ctx->PP.obj_idx;
        A.obj_verts = ctx->PP.obj_verts;
        hipLaunchKernelGGL(k_isect_prep, dim3((ntri + ISECT_WG - 1) / ISECT_WG), dim3(ISECT_WG), 0, s, A, n_meshes, (float *)ctx->d_isect_tris.p);
        HIPCHK(ctx, hipGetLastError());
    }
    ctx->isect_ready = true;
    return want_accel ? rxr_ray_accel_build(ctx, s) : RXR_OK;
}

// the kernels' view of the resident records, over the segment table `segs` (the mesh_pid words are the picking table's: only
// k_isect_fold reads them)
IsectArgs isect_args(rxr_ctx *ctx, const void *segs, uint32_t nseg, const float *origins, const float *dirs, unsigned long long *keys) {
    IsectArgs A{};
    A.ntri = ctx->PP.n_tris_in;
    A.nseg = nseg;
    A.stride = ctx->isect_stride;
    A.tris = (const float *)ctx->d_isect_tris.p;
    A.segs = (const IsectSeg *)segs;
    A.mesh_pid = (const uint32_t *)ctx->d_isect_misc.p + ctx->isect_off_pid;
    A.tin_prefix = ctx->PP.tin_prefix;
    A.vin_prefix = ctx->PP.vin_prefix;
    A.obj_idx = ctx->PP.obj_idx;
    A.obj_verts = ctx->PP.obj_verts;
    A.obj_uvs = ctx->PP.obj_uvs;
    A.obj_normals = ctx->PP.obj_normals;
    A.origins = origins;
    A.dirs = dirs;
    A.keys = keys;
    return A;
}

// the keys of rays r0 .. r0 + nr (A.keys holds at least nr * nseg of them), queued on `s`
int isect_closest(rxr_ctx *ctx, const IsectArgs &A, uint32_t r0, uint32_t nr, hipStream_t s) {
    const uint32_t ntri = A.ntri;
    if (!ntri || !A.nseg || !nr) return RXR_OK;
    HIPCHK(ctx, hipMemsetAsync(A.keys, 0xFF, (size_t)nr * A.nseg * 8, s));
    if (rxr_ray_wave_route(ctx, nr))   // opt-in: the same keys through the box tree, a wave per ray (rxr_set_ray_wave)
        return rxr_ray_wave_closest(ctx, A.segs, A.nseg, A.origins, A.dirs, r0, nr, A.keys, s);
    if (nr > ISECT_FEW_RAYS && rxr_ray_accel_takes(ctx))   // opt-in: the same keys through the box tree
        return rxr_ray_accel_closest(ctx, A.segs, A.nseg, A.origins, A.dirs, r0, nr, A.keys, s);
    if (nr <= ISECT_FEW_RAYS) {
        const dim3 grid((ntri + ISECT_WG - 1) / ISECT_WG, (nr + ISECT_RAYS_PER_Y - 1) / ISECT_RAYS_PER_Y);
        hipLaunchKernelGGL(k_isect_by_tri, grid, dim3(ISECT_WG), 0, s, A, r0, nr);
    } else {
        // enough workgroups to fill the device: split the triangle range when the rays alone do not
        const uint32_t ray_groups = (nr + ISECT_WG - 1) / ISECT_WG;
        const uint32_t max_slices = std::max(1u, (ntri + 1023u) / 1024u);
        const uint32_t slices = std::min(max_slices, std::max(1u, (4096u + ray_groups - 1) / ray_groups));
        const uint32_t slice = (ntri + slices - 1) / slices;
        const dim3 grid(ray_groups, (ntri + slice - 1) / slice);
        hipLaunchKernelGGL(k_isect_by_ray, grid, dim3(ISECT_WG), 0, s, A, r0, nr, slice);
    }
    HIPCHK(ctx, hipGetLastError());
    return RXR_OK;
}

// the whole intersect on device arrays, queued on `s`
int isect_run(rxr_ctx *ctx, const float *origins, const float *dirs, uint32_t n, uint32_t flags, const IsectOut &out, hipStream_t s) {
    if (!ctx->meshes_valid) return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_intersect: the last rxr_set_meshes failed: no meshes are registered");
    int rc = rxr_query_begin(ctx, ctx->lane[Q_ISECT], s);  // (the scratch of an intersect on another stream)
    if (rc != RXR_OK || (rc = isect_prepare(ctx, s)) != RXR_OK || (rc = rxr_ray_accel_begin_call(ctx, s)) != RXR_OK) return rc;
    const uint32_t nseg = ctx->isect_nseg;
    const uint32_t per_batch = rxr_isect_batch_rays(n, nseg);
    if ((rc = rxr_ensure(ctx, ctx->d_isect_keys, std::max<size_t>((size_t)std::min(per_batch, n) * nseg * 8, 256))) != RXR_OK) return rc;
    IsectArgs A = isect_args(ctx, ctx->d_isect_misc.p, nseg, origins, dirs, (unsigned long long *)ctx->d_isect_keys.p);
    IsectOut O = out;
    O.full = (flags & RXR_INTERSECT_FULL) ? 1u : 0u;
    for (uint32_t r0 = 0; r0 < n; r0 += per_batch) {
        const uint32_t nr = std::min(per_batch, n - r0);
        if ((rc = isect_closest(ctx, A, r0, nr, s)) != RXR_OK) return rc;
        hipLaunchKernelGGL(k_isect_fold, dim3((nr + ISECT_WG - 1) / ISECT_WG), dim3(ISECT_WG), 0, s, A, r0, nr, O);
        HIPCHK(ctx, hipGetLastError());
    }
    return rxr_query_end(ctx, ctx->lane[Q_ISECT], s);
}

}  // namespace

// ---- rxr_isect.h: the same records and kernels for the path tracer ------------------------------------------------------------
int rxr_isect_prepare(rxr_ctx *ctx, hipStream_t s) { return isect_prepare(ctx, s); }

int rxr_isect_prep_into(rxr_ctx *ctx, float *out, hipStream_t s) {
    const uint32_t ntri = ctx->PP.n_tris_in;
    if (!ntri) return RXR_OK;
    IsectArgs A{};
    A.ntri = ntri;
    A.stride = ctx->isect_stride;
    A.tin_prefix = ctx->PP.tin_prefix;
    A.vin_prefix = ctx->PP.vin_prefix;
    A.obj_idx = ctx->PP.obj_idx;
    A.obj_verts = ctx->PP.obj_verts;
    hipLaunchKernelGGL(k_isect_prep, dim3((ntri + ISECT_WG - 1) / ISECT_WG), dim3(ISECT_WG), 0, s, A, (uint32_t)ctx->meshes.size(), out);
    HIPCHK(ctx, hipGetLastError());
    return RXR_OK;
}

uint32_t rxr_isect_batch_rays(uint32_t n_rays, uint32_t nseg) {
    if (nseg && (uint64_t)n_rays * nseg > ISECT_KEYS_MAX)
        return (uint32_t)std::max<uint64_t>(ISECT_WG, ISECT_KEYS_MAX / nseg / ISECT_WG * ISECT_WG);
    return n_rays;
}

int rxr_isect_closest(rxr_ctx *ctx, const void *dev_segs, uint32_t nseg, const float *dev_origins, const float *dev_dirs, uint32_t r0,
                      uint32_t nr, unsigned long long *dev_keys, hipStream_t s) {
    return isect_closest(ctx, isect_args(ctx, dev_segs, nseg, dev_origins, dev_dirs, dev_keys), r0, nr, s);
}

extern "C" {

int rxr_intersect(rxr_ctx *ctx, const float *origins, const float *dirs, uint32_t n_rays, uint32_t flags, float *t, uint32_t *mesh,
                  uint32_t *triangle, float *hitpoint, float *uv, float *normal) {
    if (!ctx) return RXR_ERR_INVALID;
    if (!origins || !dirs || !t || !mesh || !triangle) return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_intersect: NULL ray or output array");
    if (flags & ~RXR_INTERSECT_FULL) return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_intersect: unknown flags");
    if (ctx->group) return rxr_as_member0(ctx, [&](rxr_ctx *m) { return rxr_intersect(m, origins, dirs, n_rays, flags, t, mesh, triangle, hitpoint, uv, normal); });
    if (!n_rays) return RXR_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const bool full = (flags & RXR_INTERSECT_FULL) != 0;
    const size_t n = n_rays;
    QueryIO io{ctx, ctx->lane[Q_ISECT]};
    const unsigned i_o = io.in(origins, n * 12), i_d = io.in(dirs, n * 12);
    const unsigned i_t = io.out(t, n * 4), i_m = io.out(mesh, n * 4), i_tri = io.out(triangle, n * 4), i_hp = io.out(hitpoint, n * 12);
    const unsigned i_uv = io.out(full ? uv : nullptr, n * 8), i_nrm = io.out(full ? normal : nullptr, n * 12);
    int rc = io.upload();
    if (rc != RXR_OK) return rc;
    IsectOut O{};
    O.t = io.dev<float>(i_t);
    O.mesh = io.dev<uint32_t>(i_m);
    O.tri = io.dev<uint32_t>(i_tri);
    O.hitpoint = io.dev<float>(i_hp);
    O.uv = io.dev<float>(i_uv);
    O.normal = io.dev<float>(i_nrm);
    if ((rc = isect_run(ctx, io.dev<float>(i_o), io.dev<float>(i_d), n_rays, flags, O, ctx->stream)) != RXR_OK) return rc;
    return io.download();
}

int rxr_intersect_to(rxr_ctx *ctx, const float *dev_origins, const float *dev_dirs, uint32_t n_rays, uint32_t flags, float *dev_t,
                     uint32_t *dev_mesh, uint32_t *dev_triangle, float *dev_hitpoint, float *dev_uv, float *dev_normal, void *hip_stream) {
    if (!ctx) return RXR_ERR_INVALID;
    if (!dev_origins || !dev_dirs || !dev_t || !dev_mesh || !dev_triangle)
        return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_intersect_to: NULL ray or output array");
    if (flags & ~RXR_INTERSECT_FULL) return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_intersect_to: unknown flags");
    if (ctx->group) return rxr_fail(ctx, RXR_ERR_UNSUPPORTED, "rxr_intersect_to on a multi-device context: device pointers and streams belong to ONE device (use rxr_member)");
    if (!n_rays) return RXR_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    IsectOut O{};
    O.t = dev_t;
    O.mesh = dev_mesh;
    O.tri = dev_triangle;
    O.hitpoint = dev_hitpoint;
    O.uv = dev_uv;
    O.normal = dev_normal;
    return isect_run(ctx, dev_origins, dev_dirs, n_rays, flags, O, hip_stream ? (hipStream_t)hip_stream : ctx->stream);
}

int rxr_set_ray_refresh(rxr_ctx *ctx, uint32_t mode) {
    if (!ctx) return RXR_ERR_INVALID;
    if (mode > RXR_RAY_REFRESH_RANGED) return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_set_ray_refresh: mode must be RXR_RAY_REFRESH_FULL or _RANGED");
    if (ctx->group) return rxr_as_member0(ctx, [&](rxr_ctx *m) { return rxr_set_ray_refresh(m, mode); });
    if (mode == RXR_RAY_REFRESH_FULL && ctx->refresh_pending) {   // what the updates would have done under _FULL
        ctx->isect_ready = false;
        ctx->refresh_named.clear();
        ctx->refresh_pending = 0;
    }
    ctx->refresh_mode = mode;
    return RXR_OK;
}

int rxr_ray_refresh_info(rxr_ctx *ctx, uint64_t out[RXR_RAY_REFRESH_INFO_WORDS]) {
    if (!ctx) return RXR_ERR_INVALID;
    if (!out) return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_ray_refresh_info: out is NULL");
    if (ctx->group) return rxr_as_member0(ctx, [&](rxr_ctx *m) { return rxr_ray_refresh_info(m, out); });
    out[RXR_RAY_REFRESH_INFO_MODE] = ctx->refresh_mode;
    out[RXR_RAY_REFRESH_INFO_PENDING] = ctx->refresh_pending;
    out[RXR_RAY_REFRESH_INFO_REFRESHES] = ctx->refresh_count;
    out[RXR_RAY_REFRESH_INFO_REFITS] = ctx->refit_count;
    out[RXR_RAY_REFRESH_INFO_TRIANGLES] = ctx->refresh_last_tris;
    out[RXR_RAY_REFRESH_INFO_LEAVES] = ctx->refresh_last_leaves;
    out[RXR_RAY_REFRESH_INFO_NODES] = ctx->refresh_last_nodes;
    out[RXR_RAY_REFRESH_INFO_ROUTE] = ctx->refresh_last_route;
    return RXR_OK;
}

int rxr_screen_rays_to(rxr_ctx *ctx, const float *inverse_view, const float *inverse_projection, float width, float height, uint32_t x0,
                       uint32_t y0, uint32_t w, uint32_t h, float *dev_origins, float *dev_dirs, void *hip_stream) {
    if (!ctx) return RXR_ERR_INVALID;
    if (!inverse_view || !inverse_projection || !dev_origins || !dev_dirs)
        return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_screen_rays_to: NULL matrix or output array");
    if (ctx->group) return rxr_fail(ctx, RXR_ERR_UNSUPPORTED, "rxr_screen_rays_to on a multi-device context: device pointers and streams belong to ONE device (use rxr_member)");
    const uint64_t n = (uint64_t)w * h;
    if (!n) return RXR_OK;
    if ((uint64_t)x0 + w > (1u << 24) || (uint64_t)y0 + h > (1u << 24))
        return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_screen_rays_to: pixel coordinates beyond 2^24 are not exact in f32");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    ScreenRayArgs S{};
    memcpy(S.iv, inverse_view, 64);
    memcpy(S.ip, inverse_projection, 64);
    S.width = width;
    S.height = height;
    S.x0 = x0;
    S.y0 = y0;
    S.w = w;
    S.n = n;
    S.origins = dev_origins;
    S.dirs = dev_dirs;
    hipLaunchKernelGGL(k_screen_rays, dim3((unsigned)((n + ISECT_WG - 1) / ISECT_WG)), dim3(ISECT_WG), 0,
                       hip_stream ? (hipStream_t)hip_stream : ctx->stream, S);
    HIPCHK(ctx, hipGetLastError());
    return RXR_OK;
}

}  // extern "C"
