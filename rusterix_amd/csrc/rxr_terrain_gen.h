// rxr_terrain_gen.h -- what the two files of the generated terrain share (rxr_terrain_gen.hip: the height field; rxr_terrain_excl.hip:
// the chunk meshes with their excluded sectors): the resident records, sample_height_at as ONE device function -- a grid point's
// height is the same word whichever kernel evaluates it --, generate_grid's bounds of a box, and the small helpers of their hosts.
// The semantics are written out at the head of rxr_terrain_gen.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <string>

#include "rxr_query.h"
#include "rxr_exact_math.h"

#define GEN_WG 256u
// device records, in floats: every one a multiple of four, read as float4
#define GEN_CP_FLOATS 8u      // x, y, height, radius = smoothness * 2.0 | 2.0 * radius, 0, 0, 0
#define GEN_EDGE_FLOATS 8u    // x0, y0, seg.x, seg.y | len_sq, degenerate (1.0 / 0.0), 0, 0
#define GEN_LINE_FLOATS 12u   // x0, y0, seg.x, seg.y | len_sq, degenerate, start_height, end_height - start_height | width, falloff_distance, falloff_steepness, 0
// point-records a launch: a full chip evaluates one in 2.4 ps (profiles/terrain_gen/README.md: 278 784 points x 1 024 control points
// in 695 us), so a launch of 2^30 takes about 2.6 ms, what a full terrain-bake launch takes; the launch's fixed part (13 us) is
// half a percent of that.
#define GEN_LAUNCH_WORK (1ull << 30)

struct GenRecords {
    const float4 *cp, *ridge, *edge, *line;
    const uint32_t *ridge_off;   // [R + 1]
    uint32_t C, R, L;
    float bx0, by0, bx1, by1;    // map_box
};
struct GenBox {
    float min_x, min_y;     // floor of the box's min
    int32_t sx, sy;         // steps_x, steps_y, negative ones as 0
};

namespace rxgen {

__device__ __forceinline__ float fdiv(float n, float d) { return rxm::div1_known(n, d, rxm::in_window(n) && rxm::in_window(d)); }
// Rust's f32::clamp(0.0, 1.0): a NaN stays, -0.0 stays
__device__ __forceinline__ float clamp01(float t) { return t < 0.0f ? 0.0f : (t > 1.0f ? 1.0f : t); }
__device__ __forceinline__ float magnitude2(float x, float y) { return rxm::sqrt_exact(x * x + y * y); }

// calculate_map_edge_falloff (:718-743)
__device__ __forceinline__ float edge_falloff(const GenRecords &G, float px, float py) {
    const float m = fminf(fminf(fminf(px - G.bx0, G.bx1 - px), py - G.by0), G.by1 - py);
    const float t = fdiv(m, 10.0f);
    const float s = t * t * (3.0f - 2.0f * t);
    return m <= 0.0f ? 0.0f : (m >= 10.0f ? 1.0f : s);
}

// distance_point_to_segment (:1037-1055) and the same lines of apply_linedef_smoothing (:575-586); `a` = x0, y0, seg.x, seg.y
__device__ __forceinline__ float segment_distance(float px, float py, float4 a, float len_sq, bool degenerate, float &t_param) {
    const float dx = px - a.x, dy = py - a.y;
    if (degenerate) {   // (wave-uniform)
        t_param = 0.0f;
        return magnitude2(dx, dy);
    }
    const float t = clamp01(fdiv(dx * a.z + dy * a.w, len_sq));
    const float qx = a.x + a.z * t, qy = a.y + a.w * t;
    t_param = t;
    return magnitude2(px - qx, py - qy);
}

// a linedef's influence beyond its width (:597-604): 0.0 from falloff_distance on, else powf(1 - d / falloff_distance, steepness)
__device__ __forceinline__ float power_falloff(float falloff_dist, float falloff_distance, float steepness) {
    if (falloff_dist >= falloff_distance) return 0.0f;
    const float t = 1.0f - fdiv(falloff_dist, falloff_distance);
    return powf(t, steepness);
}

// sample_height_at for the NP points of a lane
template <int NP>
__device__ __forceinline__ void gen_eval(const GenRecords &G, const float (&px)[NP], const float (&py)[NP], float (&out)[NP]) {
    float h[NP];
    // ---- interpolate_height_at (:650-714)
    if (G.C == 0u) {
#pragma unroll
        for (int k = 0; k < NP; ++k) h[k] = 0.0f;
    } else {
        float best[NP], exact_h[NP];
        bool exact[NP];
#pragma unroll
        for (int k = 0; k < NP; ++k) best[k] = 0.0f, exact_h[k] = 0.0f, exact[k] = false;
        for (uint32_t i = 0; i < G.C; ++i) {
            const float4 a = G.cp[2u * i];            // x, y, height, radius
            const float two_r = G.cp[2u * i + 1u].x;  // 2.0 * radius
#pragma unroll
            for (int k = 0; k < NP; ++k) {
                const float m = magnitude2(px[k] - a.x, py[k] - a.y);
                if (!exact[k] && m < 1e-6f) exact[k] = true, exact_h[k] = a.z;
                const float sdf = m - a.w;
                const float t = fdiv(a.w - sdf, two_r);
                const float smooth = t * t * (3.0f - 2.0f * t);
                const float falloff = sdf < -a.w ? 1.0f : (sdf > a.w ? 0.0f : smooth);
                const float c = a.z * falloff;
                if (c > best[k]) best[k] = c;
            }
        }
#pragma unroll
        for (int k = 0; k < NP; ++k) h[k] = (exact[k] ? exact_h[k] : best[k]) * edge_falloff(G, px[k], py[k]);
    }
    // ---- calculate_ridge_height_at (:513-550)
    float ridge[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) ridge[k] = 0.0f;
    for (uint32_t r = 0; r < G.R; ++r) {
        const float4 rr = G.ridge[r];   // height, plateau_width, falloff_distance, falloff_steepness
        const uint32_t e0 = G.ridge_off[r], e1 = G.ridge_off[r + 1u];
        float md[NP];
#pragma unroll
        for (int k = 0; k < NP; ++k) md[k] = INFINITY;
        for (uint32_t e = e0; e < e1; ++e) {
            const float4 a = G.edge[2u * e], b = G.edge[2u * e + 1u];
#pragma unroll
            for (int k = 0; k < NP; ++k) {
                float t_unused;
                md[k] = fminf(md[k], segment_distance(px[k], py[k], a, b.x, b.y != 0.0f, t_unused));
            }
        }
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            float c = rr.x;   // inside the plateau: the full height
            if (!(md[k] <= rr.y)) {
                const float falloff_dist = md[k] - rr.y;
                if (falloff_dist >= rr.z) c = 0.0f;
                else c = rr.x * powf(1.0f - fdiv(falloff_dist, rr.z), rr.w);
            }
            ridge[k] = ridge[k] + c;
        }
    }
    // ---- apply_linedef_smoothing (:555-623)
    float current[NP], total[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        current[k] = h[k] + ridge[k];
        h[k] = current[k];
        total[k] = 0.0f;
    }
    for (uint32_t l = 0; l < G.L; ++l) {
        const float4 a = G.line[3u * l], b = G.line[3u * l + 1u], c = G.line[3u * l + 2u];
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            float t_param;
            const float dist = segment_distance(px[k], py[k], a, b.x, b.y != 0.0f, t_param);
            const float target = b.z + b.w * t_param;
            const float influence = dist <= c.x ? 1.0f : power_falloff(dist - c.x, c.y, c.z);
            if (influence > 0.0f) {
                total[k] = total[k] + influence;
                h[k] = h[k] * (1.0f - influence) + target * influence;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        if (total[k] > 1.0f) {
            const float excess = total[k] - 1.0f;
            h[k] = h[k] * (1.0f - excess * 0.5f) + current[k] * (excess * 0.5f);
        }
        out[k] = h[k];
    }
}

// ---- host ----
inline GenRecords records_of(const rxr_ctx *ctx) {
    GenRecords G{};
    const uint8_t *base = (const uint8_t *)ctx->d_gen.p;
    G.cp = (const float4 *)(base + ctx->gen_off[0]);
    G.ridge = (const float4 *)(base + ctx->gen_off[1]);
    G.ridge_off = (const uint32_t *)(base + ctx->gen_off[2]);
    G.edge = (const float4 *)(base + ctx->gen_off[3]);
    G.line = (const float4 *)(base + ctx->gen_off[4]);
    G.C = ctx->gen_n[0], G.R = ctx->gen_n[1], G.L = ctx->gen_n[3];
    G.bx0 = ctx->gen_box[0], G.by0 = ctx->gen_box[1], G.bx1 = ctx->gen_box[2], G.by1 = ctx->gen_box[3];
    return G;
}

// Rust's `x as i32`: saturating, NaN -> 0
inline int32_t as_i32(float x) {
    if (x != x) return 0;
    if (x >= 2147483648.0f) return INT32_MAX;
    if (x <= -2147483648.0f) return INT32_MIN;
    return (int32_t)x;
}

// generate_grid's bounds of one box (:464-474), negative steps as 0
inline GenBox grid_box(const float *b, float cell_size) {
    const float min_x = std::floor(b[0]), min_y = std::floor(b[1]), max_x = std::ceil(b[2]), max_y = std::ceil(b[3]);
    // (`as i32 + 1` on a saturated cast wraps, as in a release build of the reference: a negative step, an empty grid)
    const int32_t sx = (int32_t)((uint32_t)as_i32(std::ceil((max_x - min_x) / cell_size)) + 1u);
    const int32_t sy = (int32_t)((uint32_t)as_i32(std::ceil((max_y - min_y) / cell_size)) + 1u);
    return GenBox{min_x, min_y, std::max(sx, 0), std::max(sy, 0)};
}

// the `_to` forms' pointer checks
inline int device_arrays(rxr_ctx *ctx, const char *who, const void *const *p, const size_t *bytes, const char *const *names, int n) {
    for (int i = 0; i < n; ++i) {
        if (!p[i]) continue;
        if ((uintptr_t)p[i] & 3u) return rxr_fail(ctx, RXR_ERR_INVALID, std::string(who) + ": " + names[i] + " must be 4-byte aligned device memory");
        if (!rxr_on_device(ctx, p[i], bytes[i]))
            return rxr_fail(ctx, RXR_ERR_INVALID, std::string(who) + ": " + names[i] + " is not device memory of the context's device (or is too small)");
    }
    return RXR_OK;
}

}  // namespace rxgen
