// rxr_terrain_hit.hip -- the editor's terrain pick: Terrain::ray_terrain_hit (src/terrain/mod.rs:427-479) with sample_height (:148-152),
// sample_height_bilinear (:155-173) and get_height (:82-89).  include/rxr.h: rxr_check_terrain_heights, rxr_set_terrain_heights,
// rxr_terrain_hits, rxr_terrain_hits_to.
//
// Semantics, per ray, all f32, one operation per reference operation in its order, nothing fused (the build's -ffp-contract=off):
//   t = 0; 1500 times: p = origin + dir * t; h = get_height(round(p.x) as i32, round(p.z) as i32) (half away from zero, saturating,
//   NaN -> 0; WORLD coordinates, the scale is not applied); p.y - h < 0.01: refine and return; t = t + 0.1; t > max_distance: leave.
//   refine: low = max(t - 0.1, 0), high = t; four bisections over the bilinear height; t_hit = (low + high) * 0.5;
//   q = origin + dir * t_hit; world_pos = (q.x, bilinear(q.x, q.z), q.z); grid_pos = floor(q.xz / scale) as i32.
// The t of step k does not depend on the ray: t_0 = 0, t_{k+1} = fl(t_k + 0.1f) (NOT k * 0.1f).  Step k >= 1 is tested iff
// t_k <= max_distance (a NaN max_distance never leaves), so the number of steps K is ONE value per call: the host computes it from the
// table of t_k and passes it as a kernel argument; no kernel compares t with max_distance.  Whether step k hits depends on t_k alone:
// the answer is the lowest k < K whose test holds.
//
// Two launch shapes, the same refine():
//   k_terrain_hit_lane  one ray per lane, workgroups of 256.  t is accumulated in a register (the same additions as the table's).  The
//     height address of a step does not depend on earlier loads, only the exit does: the loop issues HIT_UNROLL steps' loads, then tests
//     them in order, and leaves when every lane of the wave has hit or K is reached.
//   k_terrain_hit_wave  one ray per wave (the click).  In a round lane l tests step 64 r + l with t_k from the table; the lowest set bit
//     of the first non-empty ballot is the step.  HIT_UNROLL rounds' loads are in flight together: at most 24 rounds instead of a chain
//     of up to 1500 dependent iterations.  Every lane then runs refine() redundantly and lane 0 stores.
// A call is cut into launches of a bounded number of rays (RXR_TERRAIN_HIT_LAUNCH_RAYS overrides the bound).  Rays travel as device
// arrays; nothing a queued launch reads can change under it except the resident heights, which rxr_set_terrain_heights replaces only
// after rxr_quiesce.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "rxr_debug.h"
#include "rxr_query.h"
#include "rxr_exact_math.h"

#define HIT_WG 256u       // k_terrain_hit_lane's workgroup
#define HIT_UNROLL 4u     // steps (rounds) whose loads are in flight together
// The ray count up to which the per-wave kernel runs: where the two measured curves cross on rays that run all 1500 steps
// (profiles/terrain_hit/README.md: per-wave 14 us against 217 us at one ray, 359 against 390 us at 262 144, 1320 against 1177 us at
// 1 048 576).  Coherent rays that hit early favour the per-lane kernel at screen size (1.32 against 2.17 ms at 1920 x 1080).
#define TERRAIN_HIT_FEW_RAYS (1u << 18)
// Rays a launch: at the 0.75 ps (no step loads a height) to 1.72 ps (every step does) per ray-step of the per-lane kernel on a full
// chip, a launch whose 2^20 rays all run 1500 steps takes 1.2 - 2.7 ms, about what a full terrain-bake launch takes.
#define TERRAIN_HIT_DEFAULT_LAUNCH_RAYS (1u << 20)

struct HitArgs {
    const float *heights;   // [gh][gw], row-major
    const float *tk;        // [RXR_TERRAIN_MARCH_STEPS]: t_k
    int32_t x0, y0;         // the grid's first cell
    uint32_t gw, gh;        // its size (0: the plane at 0)
    float sx, sy;
    const float *origins, *dirs;   // [n][3]
    uint32_t first, end;    // the rays of this launch
    uint32_t K;             // steps 0 .. K-1 are tested
    uint32_t *hit;
    float *t, *world_pos;   // may be null
    int32_t *grid_pos;      // may be null
};

namespace {

__device__ __forceinline__ float fdiv(float n, float d) { return rxm::div1_known(n, d, rxm::in_window(n) && rxm::in_window(d)); }

// Rust's `x as i32`: saturating, NaN -> 0.  Selects, no branches: the march runs it twice a step.
__device__ __forceinline__ int32_t sat_i32(float x) {
    const int32_t r = (int32_t)fminf(fmaxf(x, -2147483648.0f), 2147483520.0f);   // (fmaxf drops a NaN: the cast is always in range)
    return x != x ? 0 : (x >= 2147483648.0f ? INT32_MAX : r);
}

// Terrain::get_height (:82-89): 0.0 for a cell that does not exist
__device__ __forceinline__ float height_at(const HitArgs &A, int32_t x, int32_t y) {
    const uint32_t gx = (uint32_t)x - (uint32_t)A.x0, gy = (uint32_t)y - (uint32_t)A.y0;
    return (gx < A.gw && gy < A.gh) ? A.heights[(size_t)gy * A.gw + gx] : 0.0f;
}

// sample_height (:148-152)
__device__ __forceinline__ float sample_nearest(const HitArgs &A, float x, float z) { return height_at(A, sat_i32(roundf(x)), sat_i32(roundf(z))); }

// sample_height_bilinear (:155-173); x0 + 1 wraps as in a release build (the height there is 0.0 either way: cells lie within +-2^30)
__device__ __forceinline__ float sample_bilinear(const HitArgs &A, float x, float y) {
    const int32_t x0 = sat_i32(floorf(x)), y0 = sat_i32(floorf(y));
    const int32_t x1 = (int32_t)((uint32_t)x0 + 1u), y1 = (int32_t)((uint32_t)y0 + 1u);
    const float tx = x - (float)x0, ty = y - (float)y0;
    const float h00 = height_at(A, x0, y0), h10 = height_at(A, x1, y0), h01 = height_at(A, x0, y1), h11 = height_at(A, x1, y1);
    const float h0 = h00 * (1.0f - tx) + h10 * tx;
    const float h1 = h01 * (1.0f - tx) + h11 * tx;
    return h0 * (1.0f - ty) + h1 * ty;
}

struct Ray {
    float ox, oy, oz, dx, dy, dz;
};

__device__ __forceinline__ Ray load_ray(const HitArgs &A, uint32_t i) {
    const float *o = A.origins + 3 * (size_t)i, *d = A.dirs + 3 * (size_t)i;
    return Ray{o[0], o[1], o[2], d[0], d[1], d[2]};
}

// the coarse test of one step (:432-436)
__device__ __forceinline__ void coarse(const HitArgs &A, const Ray &r, float t, float &py, float &h) {
    const float px = r.ox + r.dx * t, pz = r.oz + r.dz * t;
    py = r.oy + r.dy * t;
    h = sample_nearest(A, px, pz);
}

// :437-470 for a hit at t (the coarse step's t), stored for ray i
__device__ __forceinline__ void refine_store(const HitArgs &A, const Ray &r, float t, uint32_t i, bool stores) {
    float low = fmaxf(t - 0.1f, 0.0f), high = t;
    for (int it = 0; it < 4; ++it) {
        const float mid = (low + high) * 0.5f;
        const float mx = r.ox + r.dx * mid, my = r.oy + r.dy * mid, mz = r.oz + r.dz * mid;
        if (my - sample_bilinear(A, mx, mz) < 0.01f) high = mid;
        else low = mid;
    }
    const float t_hit = (low + high) * 0.5f;
    const float qx = r.ox + r.dx * t_hit, qz = r.oz + r.dz * t_hit;
    const float hh = sample_bilinear(A, qx, qz);
    const int32_t gx = sat_i32(floorf(fdiv(qx, A.sx))), gy = sat_i32(floorf(fdiv(qz, A.sy)));
    if (!stores) return;
    A.hit[i] = 1u;
    if (A.t) A.t[i] = t_hit;
    if (A.world_pos) {
        float *w = A.world_pos + 3 * (size_t)i;
        w[0] = qx;
        w[1] = hh;
        w[2] = qz;
    }
    if (A.grid_pos) {
        A.grid_pos[2 * (size_t)i] = gx;
        A.grid_pos[2 * (size_t)i + 1] = gy;
    }
}

__device__ __forceinline__ void store_miss(const HitArgs &A, uint32_t i) {
    A.hit[i] = 0u;
    if (A.t) A.t[i] = FLT_MAX;
    if (A.world_pos) {
        float *w = A.world_pos + 3 * (size_t)i;
        w[0] = w[1] = w[2] = 0.0f;
    }
    if (A.grid_pos) A.grid_pos[2 * (size_t)i] = A.grid_pos[2 * (size_t)i + 1] = 0;
}

}  // namespace

extern "C" __global__ __launch_bounds__(HIT_WG) void k_terrain_hit_lane(HitArgs A) {
    const uint32_t i = A.first + blockIdx.x * HIT_WG + threadIdx.x;
    const bool live = i < A.end;
    const Ray r = load_ray(A, live ? i : A.first);   // (a lane past the end repeats a ray and stores nothing)
    bool found = !live;
    float t = 0.0f, t_found = 0.0f;
    for (uint32_t k = 0; k < A.K; k += HIT_UNROLL) {
        float tt[HIT_UNROLL], py[HIT_UNROLL], h[HIT_UNROLL];
#pragma unroll
        for (uint32_t j = 0; j < HIT_UNROLL; ++j) {
            tt[j] = t;
            coarse(A, r, t, py[j], h[j]);
            t = t + 0.1f;
        }
#pragma unroll
        for (uint32_t j = 0; j < HIT_UNROLL; ++j)
            if (!found && k + j < A.K && py[j] - h[j] < 0.01f) {
                found = true;
                t_found = tt[j];
            }
        if (rxm::wave_all(found)) break;
    }
    if (!live) return;
    if (found) refine_store(A, r, t_found, i, true);
    else store_miss(A, i);
}

extern "C" __global__ __launch_bounds__(64) void k_terrain_hit_wave(HitArgs A) {
    const uint32_t i = A.first + blockIdx.x;   // (the grid is end - first)
    const uint32_t lane = threadIdx.x;
    const Ray r = load_ray(A, i);
    uint32_t step = 0xFFFFFFFFu;
    for (uint32_t base = 0; base < A.K && step == 0xFFFFFFFFu; base += 64u * HIT_UNROLL) {
        float py[HIT_UNROLL], h[HIT_UNROLL];
#pragma unroll
        for (uint32_t j = 0; j < HIT_UNROLL; ++j) {
            const uint32_t k = base + 64u * j + lane;
            coarse(A, r, A.tk[min(k, RXR_TERRAIN_MARCH_STEPS - 1u)], py[j], h[j]);
        }
#pragma unroll
        for (uint32_t j = 0; j < HIT_UNROLL; ++j) {
            const uint32_t k = base + 64u * j + lane;
            const uint64_t b = __builtin_amdgcn_ballot_w64(k < A.K && py[j] - h[j] < 0.01f);
            if (b && step == 0xFFFFFFFFu) step = base + 64u * j + (uint32_t)__builtin_ctzll(b);
        }
    }
    if (step != 0xFFFFFFFFu) refine_store(A, r, A.tk[step], i, lane == 0u);
    else if (lane == 0u) store_miss(A, i);
}

namespace {

// t_k by the reference's additions
const float *march_table() {
    static const std::vector<float> table = [] {
        std::vector<float> v(RXR_TERRAIN_MARCH_STEPS);
        float t = 0.0f;
        for (uint32_t k = 0; k < RXR_TERRAIN_MARCH_STEPS; ++k) {
            v[k] = t;
            t = t + 0.1f;
        }
        return v;
    }();
    return table.data();
}

// the steps a call tests: 0, then every k whose t_k does not exceed max_distance (:473-476)
uint32_t steps_of(float max_distance) {
    const float *tk = march_table();
    uint32_t K = 1;
    while (K < RXR_TERRAIN_MARCH_STEPS && !(tk[K] > max_distance)) ++K;
    return K;
}

struct HeightShape {
    int32_t x0 = 0, y0 = 0;
    uint32_t gw = 0, gh = 0;
};

int check_heights(const float *scale, const int32_t *cell_xy, const float *cell_height, uint32_t n_cells, HeightShape &shape, std::string &err) {
    auto bad = [&](const std::string &m) {
        err = m;
        return (int)RXR_ERR_INVALID;
    };
    if (!scale) return bad("NULL scale");
    if (!(std::isfinite(scale[0]) && std::isfinite(scale[1]) && scale[0] > 0.0f && scale[1] > 0.0f)) return bad("scale must be finite and > 0");
    if (n_cells && (!cell_xy || !cell_height)) return bad("NULL cell array");
    int64_t lo[2] = {INT32_MAX, INT32_MAX}, hi[2] = {INT32_MIN, INT32_MIN};
    for (uint32_t i = 0; i < n_cells; ++i)
        for (int a = 0; a < 2; ++a) {
            const int64_t c = cell_xy[2 * (size_t)i + a];
            if (c < -(1ll << 30) || c > (1ll << 30))
                return bad("cell " + std::to_string(i) + " (" + std::to_string(cell_xy[2 * (size_t)i]) + ", " + std::to_string(cell_xy[2 * (size_t)i + 1]) + "): coordinate outside +-2^30");
            lo[a] = std::min(lo[a], c);
            hi[a] = std::max(hi[a], c);
        }
    shape = HeightShape{};
    if (n_cells) {
        const int64_t w = hi[0] - lo[0] + 1, h = hi[1] - lo[1] + 1;
        if (w > RXR_TERRAIN_MAX_CELLS || h > RXR_TERRAIN_MAX_CELLS || w * h > RXR_TERRAIN_MAX_CELLS)
            return bad("the cells' bounding rectangle (" + std::to_string(w) + " x " + std::to_string(h) + ") holds more than RXR_TERRAIN_MAX_CELLS cells");
        shape.x0 = (int32_t)lo[0];
        shape.y0 = (int32_t)lo[1];
        shape.gw = (uint32_t)w;
        shape.gh = (uint32_t)h;
    }
    return RXR_OK;
}

// every ray of a call on device arrays, queued on `s`
int hits_run(rxr_ctx *ctx, const float *origins, const float *dirs, uint32_t n, float max_distance, uint32_t *hit, float *t, float *world_pos,
             int32_t *grid_pos, hipStream_t s) {
    uint32_t bound = TERRAIN_HIT_DEFAULT_LAUNCH_RAYS;
    if (const char *e = getenv("RXR_TERRAIN_HIT_LAUNCH_RAYS")) {
        const unsigned long long v = strtoull(e, nullptr, 10);
        if (v) bound = (uint32_t)std::min<unsigned long long>(v, 0xFFFFFFFFull);
    }
    bool wave = n <= TERRAIN_HIT_FEW_RAYS;
    if (const char *e = getenv("RXR_TERRAIN_HIT_ROUTE")) {
        if (!strcmp(e, "lane")) wave = false;
        else if (!strcmp(e, "wave")) wave = true;
        else if (e[0]) return rxr_fail(ctx, RXR_ERR_INVALID, std::string("RXR_TERRAIN_HIT_ROUTE must be lane or wave, not ") + e);
    }
    HitArgs A{};
    // (rxr_set_terrain_height_source: the processed grid lies over the same rectangle; rxr_flatten_terrain_to writes it in stream order)
    const bool processed = ctx->height_source == RXR_TERRAIN_HEIGHTS_PROCESSED;
    A.heights = (const float *)(processed ? ctx->d_pheights.p : ctx->d_heights.p);
    A.tk = (const float *)ctx->d_heights_tk.p;
    A.x0 = ctx->heights_x0;
    A.y0 = ctx->heights_y0;
    A.gw = ctx->heights_gw;
    A.gh = ctx->heights_gh;
    A.sx = ctx->heights_scale[0];
    A.sy = ctx->heights_scale[1];
    A.origins = origins;
    A.dirs = dirs;
    A.K = steps_of(max_distance);
    A.hit = hit;
    A.t = t;
    A.world_pos = world_pos;
    A.grid_pos = grid_pos;
    int rc = rxr_query_begin(ctx, ctx->lane[Q_HEIGHTS], s);
    if (rc != RXR_OK || (processed && (rc = rxr_query_begin(ctx, ctx->lane[Q_FLATTEN], s)) != RXR_OK)) return rc;
    ctx->heights_launches = 0;
    ctx->heights_kernel = wave ? "k_terrain_hit_wave" : "k_terrain_hit_lane";
    for (uint32_t first = 0; first < n;) {
        // (a launch takes at least one workgroup: bound >= 1; the per-wave grid is one workgroup a ray)
        const uint32_t count = std::min(n - first, wave ? std::min(bound, 1u << 24) : bound);
        A.first = first;
        A.end = first + count;
        if (wave) hipLaunchKernelGGL(k_terrain_hit_wave, dim3(count), dim3(64), 0, s, A);
        else hipLaunchKernelGGL(k_terrain_hit_lane, dim3((count + HIT_WG - 1u) / HIT_WG), dim3(HIT_WG), 0, s, A);
        HIPCHK(ctx, hipGetLastError());
        ++ctx->heights_launches;
        first += count;
    }
    return rxr_query_end(ctx, ctx->lane[Q_HEIGHTS], s);
}

}  // namespace

extern "C" {

int rxr_check_terrain_heights(const float scale[2], const int32_t *cell_xy, const float *cell_height, uint32_t n_cells, char *message,
                              uint32_t message_capacity) {
    HeightShape shape;
    std::string err;
    const int rc = check_heights(scale, cell_xy, cell_height, n_cells, shape, err);
    rxr_copy_message(err, message, message_capacity);
    return rc;
}

int rxr_set_terrain_heights(rxr_ctx *ctx, const float scale[2], const int32_t *cell_xy, const float *cell_height, uint32_t n_cells) {
    if (!ctx) return RXR_ERR_INVALID;
    if (ctx->group) return rxr_as_member0(ctx, [&](rxr_ctx *m) { return rxr_set_terrain_heights(m, scale, cell_xy, cell_height, n_cells); });
    HeightShape shape;
    std::string err;
    int rc = check_heights(scale, cell_xy, cell_height, n_cells, shape, err);
    if (rc != RXR_OK) return rxr_fail(ctx, rc, "rxr_set_terrain_heights: " + err);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if ((rc = rxr_quiesce(ctx)) != RXR_OK) return rc;   // queued hit and mesh calls read what is replaced here
    ctx->heights_set = false;
    // the dense grid; a coordinate given twice: the later entry wins
    const size_t n_grid = (size_t)shape.gw * shape.gh;
    // ... and the presence mask over the same rectangle (rxr_terrain_mesh.hip): 1 where the caller listed the cell, whatever its height
    std::vector<float> grid(n_grid, 0.0f);
    std::vector<uint8_t> mask(n_grid, 0);
    for (uint32_t i = 0; i < n_cells; ++i) {
        const size_t at = (size_t)((int64_t)cell_xy[2 * (size_t)i + 1] - shape.y0) * shape.gw + (size_t)((int64_t)cell_xy[2 * (size_t)i] - shape.x0);
        grid[at] = cell_height[i];
        mask[at] = 1;
    }
    hipStream_t s = ctx->stream;
    if ((rc = rxr_ensure(ctx, ctx->d_heights, std::max<size_t>(n_grid * sizeof(float), 256))) != RXR_OK) return rc;
    if ((rc = rxr_ensure(ctx, ctx->d_heights_mask, std::max<size_t>(n_grid, 256))) != RXR_OK) return rc;
    const bool table_new = !ctx->d_heights_tk.p;
    if ((rc = rxr_ensure(ctx, ctx->d_heights_tk, RXR_TERRAIN_MARCH_STEPS * sizeof(float))) != RXR_OK) return rc;
    if (n_grid) HIPCHK(ctx, hipMemcpyAsync(ctx->d_heights.p, grid.data(), n_grid * sizeof(float), hipMemcpyHostToDevice, s));
    if (n_grid) HIPCHK(ctx, hipMemcpyAsync(ctx->d_heights_mask.p, mask.data(), n_grid, hipMemcpyHostToDevice, s));
    if (table_new) HIPCHK(ctx, hipMemcpyAsync(ctx->d_heights_tk.p, march_table(), RXR_TERRAIN_MARCH_STEPS * sizeof(float), hipMemcpyHostToDevice, s));
    // the processed grid (rxr_terrain_flatten.hip) starts over as a copy of the registered one
    if ((rc = rxr_ensure(ctx, ctx->d_pheights, std::max<size_t>(n_grid * sizeof(float), 256))) != RXR_OK) return rc;
    if ((rc = rxr_ensure(ctx, ctx->d_pheights_mask, std::max<size_t>(n_grid, 256))) != RXR_OK) return rc;
    if (n_grid) HIPCHK(ctx, hipMemcpyAsync(ctx->d_pheights.p, ctx->d_heights.p, n_grid * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (n_grid) HIPCHK(ctx, hipMemcpyAsync(ctx->d_pheights_mask.p, ctx->d_heights_mask.p, n_grid, hipMemcpyDeviceToDevice, s));
    HIPCHK(ctx, hipStreamSynchronize(s));   // (the host vectors above are read until here)
    ctx->heights_scale[0] = scale[0];
    ctx->heights_scale[1] = scale[1];
    ctx->heights_x0 = shape.x0;
    ctx->heights_y0 = shape.y0;
    ctx->heights_gw = shape.gw;
    ctx->heights_gh = shape.gh;
    ctx->heights_set = true;
    return RXR_OK;
}

int rxr_terrain_hits(rxr_ctx *ctx, const float *origins, const float *dirs, uint32_t n_rays, float max_distance, uint32_t *hit, float *t,
                     float *world_pos, int32_t *grid_pos) {
    if (!ctx) return RXR_ERR_INVALID;
    if (ctx->group) return rxr_as_member0(ctx, [&](rxr_ctx *m) { return rxr_terrain_hits(m, origins, dirs, n_rays, max_distance, hit, t, world_pos, grid_pos); });
    if (!ctx->heights_set) return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_terrain_hits: no terrain heights are resident (rxr_set_terrain_heights)");
    if (!n_rays) return RXR_OK;
    if (!origins || !dirs || !hit) return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_terrain_hits: NULL ray or hit array");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t n = n_rays;
    QueryIO io{ctx, ctx->lane[Q_HEIGHTS]};
    const unsigned i_o = io.in(origins, n * 12), i_d = io.in(dirs, n * 12);
    const unsigned i_hit = io.out(hit, n * 4), i_t = io.out(t, n * 4), i_wp = io.out(world_pos, n * 12), i_gp = io.out(grid_pos, n * 8);
    int rc = io.upload();
    if (rc != RXR_OK) return rc;
    if ((rc = hits_run(ctx, io.dev<float>(i_o), io.dev<float>(i_d), n_rays, max_distance, io.dev<uint32_t>(i_hit), io.dev<float>(i_t), io.dev<float>(i_wp),
                       io.dev<int32_t>(i_gp), ctx->stream)) != RXR_OK)
        return rc;
    return io.download();
}

int rxr_terrain_hits_to(rxr_ctx *ctx, const float *dev_origins, const float *dev_dirs, uint32_t n_rays, float max_distance, uint32_t *dev_hit,
                        float *dev_t, float *dev_world_pos, int32_t *dev_grid_pos, void *hip_stream) {
    if (!ctx) return RXR_ERR_INVALID;
    if (ctx->group) return rxr_fail(ctx, RXR_ERR_UNSUPPORTED, "rxr_terrain_hits_to on a multi-device context: device pointers and streams belong to ONE device (use rxr_member)");
    if (!ctx->heights_set) return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_terrain_hits_to: no terrain heights are resident (rxr_set_terrain_heights)");
    if (!n_rays) return RXR_OK;
    if (!dev_origins || !dev_dirs || !dev_hit) return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_terrain_hits_to: NULL ray or hit array");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t n = n_rays;
    const struct {
        const void *p;
        size_t bytes;
        const char *name;
    } arrays[] = {{dev_origins, n * 12, "dev_origins"}, {dev_dirs, n * 12, "dev_dirs"}, {dev_hit, n * 4, "dev_hit"}, {dev_t, n * 4, "dev_t"},
                  {dev_world_pos, n * 12, "dev_world_pos"}, {dev_grid_pos, n * 8, "dev_grid_pos"}};
    for (const auto &a : arrays) {
        if (!a.p) continue;
        if ((uintptr_t)a.p & 3u) return rxr_fail(ctx, RXR_ERR_INVALID, std::string("rxr_terrain_hits_to: ") + a.name + " must be 4-byte aligned device memory");
        if (!rxr_on_device(ctx, a.p, a.bytes))
            return rxr_fail(ctx, RXR_ERR_INVALID, std::string("rxr_terrain_hits_to: ") + a.name + " is not device memory of the context's device (or is too small)");
    }
    return hits_run(ctx, dev_origins, dev_dirs, n_rays, max_distance, dev_hit, dev_t, dev_world_pos, dev_grid_pos, hip_stream ? (hipStream_t)hip_stream : ctx->stream);
}

// test-only: the symbol name of the last call's march kernel ("" before any) and, in *launches, its launches
const char *rxr_debug_terrain_hit_kernel(rxr_ctx *ctx, uint32_t *launches) {
    if (!ctx) return "";
    if (ctx->group) return rxr_debug_terrain_hit_kernel(rxr_member(ctx, 0), launches);
    if (launches) *launches = ctx->heights_launches;
    return ctx->heights_kernel;
}

uint32_t rxr_debug_terrain_hit_few_rays(void) { return TERRAIN_HIT_FEW_RAYS; }

}  // extern "C"
