// rxr_trace.hip -- path tracing the resident scene: Tracer::trace (src/tracer/trace.rs:105-475) into an AccumBuffer
// (src/tracer/buffer.rs) over the meshes of rxr_set_meshes and the tiles of rxr_set_textures.  include/rxr.h: rxr_check_trace_scene,
// rxr_set_trace_scene, rxr_trace_srgb_table, rxr_trace, rxr_trace_to, rxr_accum_to_rgba, rxr_accum_to_rgba_to; DESIGN.md section 18.
//
// Wavefront, one round per bounce, a thread per pixel:
//   k_trace_rays        the camera's create_ray with its jitter; throughput 1, radiance 0, path live
//   rxr_isect_closest   the closest-hit kernels of rxr_intersect.hip (k_isect_by_tri / k_isect_by_ray) over the resident triangle
//                       records and THIS file's segment table: runs of participating meshes (RXR_LIST_CHUNK, _CHUNK_TERRAIN, _STATIC,
//                       _DYNAMIC) are one plain-rule segment each, runs of opacity / overlay meshes a segment the shading ignores.
//                       The reference's fold `hit.t < best.t` in mesh order is the minimum of (t, global triangle) over the plain
//                       segments: equal t goes to the earliest mesh, within it to the earliest triangle
//   k_trace_shade       the winner's test again for u and v (the same operations, the same bits), uv and normal as
//                       Batch3D::intersect(ray, false); evaluate_hit; the lights; reflect or sample_cosine; the roulette; the next
//                       ray, or the path retires (its origin becomes NaN: every later triangle test rejects it at once)
//   k_trace_accumulate  the running average
// A dead path stays in its slot: there is no compaction between rounds.
//
// Arithmetic as everywhere: nothing contracted (-ffp-contract=off), vek's dot / cross / normalized, correctly rounded division and
// sqrt.  The device runs no libm function before a path's first diffuse bounce (cosf, sinf) or spot light (acosf): srgb_to_linear is
// a table of 256 floats built by the host's powf.
//
// sample_texture, terrain_texel and light_color_at are RESTATED here from rxr_kernels.hip (sample_nearest / sample_linear /
// sample_texture, terrain_texel, smoothstep_rs / apply_flicker / light_color_at): that file's text is what the run-time compiler embeds and the resource tests pin,
// so nothing moves out of it.  tests/test_gpu_trace.py holds these copies to the oracle's texture_sample and light_radiance_at.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "rxr_isect.h"
#include "rxr_query.h"

using namespace isect;

namespace {

constexpr uint32_t TRACE_WG = 256;
constexpr uint32_t SEG_TRACED = 0, SEG_IGNORED = 3;   // the `rule` word of this file's segments (rxr_isect.h: six words each)
constexpr uint32_t MESH_WORDS = 8;
enum : uint32_t { MR_KIND = 0, MR_TEX, MR_PIXEL, MR_REPEAT, MR_ROLE, MR_MODIFIER, MR_VALUE };
enum : uint32_t { TEXEL_ZERO = 0, TEXEL_PIXEL = 1, TEXEL_TEXTURE = 2, TEXEL_TERRAIN = 3 };
constexpr uint32_t TERRAIN_WORDS = 6;   // per terrain-sourced mesh (MR_TEX names it): the slot's place in the chunk-texture pool, its width and height, chunk.origin, pixels_per_tile
enum : uint32_t { ROLE_MATTE = 0, ROLE_GLOSSY, ROLE_METALLIC, ROLE_TRANSPARENT, ROLE_EMISSIVE };
enum : uint32_t { MOD_NONE = 0, MOD_LUMINANCE, MOD_SATURATION, MOD_INV_LUMINANCE, MOD_INV_SATURATION };
constexpr float PI_F = 3.14159265358979323846f;   // std::f32::consts::PI
constexpr float INV_255 = 1.0f / 255.0f;          // lib.rs: pixel_to_vec4

// the generator of include/rxr.h
__host__ __device__ inline uint32_t pcg(uint32_t v) {
    const uint32_t s = v * 747796405u + 2891336453u;
    const uint32_t w = ((s >> ((s >> 28) + 4u)) ^ s) * 277803737u;
    return (w >> 22) ^ w;
}
__host__ __device__ inline float trace_rand(uint32_t seed, uint32_t frame, uint32_t pixel, uint32_t slot) {
    const uint32_t u = pcg(pcg(pcg(seed + frame) + pixel) + slot);
    return (float)(u >> 8) * 5.9604644775390625e-08f;   // 2^-24
}

struct TraceCamera {
    uint32_t kind, width, height;
    float pos[3], forward[3], right[3], up[3], half_width, half_height;
};

struct TraceArgs {
    // the resident geometry (rxr_intersect.hip's records and the object-space pools)
    const float *tris;
    uint32_t stride, nseg;
    const uint32_t *segs, *tin_prefix, *vin_prefix, *obj_idx;
    const float2 *obj_uvs;
    const float *obj_normals;
    // the trace scene
    const uint32_t *mesh_rec;
    const rxr_light *lights;
    const float *srgb;
    const DevTexDesc *tex;
    const uint32_t *texels;
    const uint32_t *terrain_rec, *chunk_texels;   // the pool of rxr_set_chunk_textures
    uint32_t n_lights, hash_anim, sample_mode;
    // the paths
    float *origins, *dirs, *thr, *ret;
    uint32_t *live;
    const unsigned long long *keys;   // of rays r0 .. r0 + nr; null: no triangle takes part
    uint32_t seed, frame, bounce;
};

__device__ __forceinline__ F3 add3(F3 a, F3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ F3 mul3(F3 a, F3 b) { return {a.x * b.x, a.y * b.y, a.z * b.z}; }
__device__ __forceinline__ F3 scale3(F3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }
__device__ __forceinline__ F3 div3(F3 a, float s) { return {a.x / s, a.y / s, a.z / s}; }
__device__ __forceinline__ F3 arr3(const float *p) { return {p[0], p[1], p[2]}; }
__device__ __forceinline__ void store3(float *p, uint64_t i, F3 v) { p[3 * i] = v.x, p[3 * i + 1] = v.y, p[3 * i + 2] = v.z; }
// f32::clamp: a NaN stays
__device__ __forceinline__ float rclamp(float x, float lo, float hi) { return x < lo ? lo : (x > hi ? hi : x); }
// Rust's `x as u32`: saturating, NaN -> 0
__device__ __forceinline__ uint32_t sat_u32(float x) {
    if (!(x > 0.0f)) return 0u;
    return x >= 4294967296.0f ? 0xFFFFFFFFu : (uint32_t)x;
}
__device__ __forceinline__ uint32_t sat_index(float x, uint32_t hi) { return min(sat_u32(x), hi); }

// ---- the cameras' create_ray behind their host-computed constants ----------------------------------------------------------------
__global__ __launch_bounds__(TRACE_WG) void k_trace_rays(TraceCamera C, TraceArgs A, uint32_t n) {
    const uint32_t i = blockIdx.x * TRACE_WG + threadIdx.x;
    if (i >= n) return;
    const float sx = (float)C.width, sy = (float)C.height;
    const float uvx = (float)(i % C.width) / sx;
    float uvy = 1.0f - (float)(i / C.width) / sy;
    const float jx = trace_rand(A.seed, A.frame, i, 0u), jy = trace_rand(A.seed, A.frame, i, 1u);
    const F3 pos = arr3(C.pos), fwd = arr3(C.forward), right = arr3(C.right), up = arr3(C.up);
    F3 o = pos, d;
    if (C.kind == RXR_TRACE_CAMERA_FIRSTP) {   // d3firstp.rs:112-138
        const float psx = 1.0f / sx, psy = 1.0f / sy;
        const F3 lower_left = sub3(sub3(add3(pos, fwd), scale3(right, C.half_width)), scale3(up, C.half_height));
        const F3 horizontal = scale3(right, 2.0f * C.half_width), vertical = scale3(up, 2.0f * C.half_height);
        const F3 sample_pos = add3(add3(lower_left, scale3(horizontal, psx * jx + uvx)), scale3(vertical, psy * jy + uvy));
        d = normalized3(sub3(sample_pos, pos));
    } else if (C.kind == RXR_TRACE_CAMERA_ORBIT) {   // d3orbit.rs:117-153
        const float psx = 1.0f / sx, psy = 1.0f / sy;
        uvy = 1.0f - uvy;
        const float nx = (psx * jx + uvx) * 2.0f - 1.0f, ny = (psy * jy + uvy) * 2.0f - 1.0f;
        d = normalized3(sub3(add3(fwd, scale3(scale3(right, nx), C.half_width)), scale3(scale3(up, ny), C.half_height)));
    } else {   // d3iso.rs:159-182: a shifted origin, one direction
        const F3 horizontal = scale3({-right.x, -right.y, -right.z}, 2.0f * C.half_width), vertical = scale3(up, 2.0f * C.half_height);
        const float psx = 1.0f / fmaxf(sx, 1.0f), psy = 1.0f / fmaxf(sy, 1.0f);
        o = add3(add3(pos, scale3(horizontal, (psx * jx + uvx) - 0.5f)), scale3(vertical, (psy * jy + uvy) - 0.5f));
        d = fwd;
    }
    store3(A.origins, i, o);
    store3(A.dirs, i, d);
    store3(A.thr, i, {1.0f, 1.0f, 1.0f});
    store3(A.ret, i, {0.0f, 0.0f, 0.0f});
    A.live[i] = 1u;
}

// ---- Texture::sample (texture.rs:203-232, :307-323, :414-460): rxr_kernels.hip's sample_nearest / sample_linear / sample_texture ---
// (colour channels only: nothing in the tracer reads a texel's alpha)
__device__ __forceinline__ uint32_t sample_nearest(const DevTexDesc &d, const uint32_t *texels, float u, float v) {
    const uint32_t tx = sat_index(roundf(u * ((float)d.w - 1.0f)), d.w - 1u);
    const uint32_t ty = sat_index(roundf(v * ((float)d.h - 1.0f)), d.h - 1u);
    return texels[d.offset + ty * d.w + tx];
}
__device__ __forceinline__ uint32_t sample_linear(const DevTexDesc &d, const uint32_t *texels, float u, float v) {
    const float x = u * ((float)d.w - 1.0f), y = v * ((float)d.h - 1.0f);
    const float fx = floorf(x), fy = floorf(y);
    const uint32_t x0 = sat_index(fx, d.w - 1u), y0 = sat_index(fy, d.h - 1u);
    const uint32_t x1 = min(x0 + 1u, d.w - 1u), y1 = min(y0 + 1u, d.h - 1u);
    const float dx = x - fx, dy = y - fy;
    const uint32_t c00 = texels[d.offset + y0 * d.w + x0], c10 = texels[d.offset + y0 * d.w + x1];
    const uint32_t c01 = texels[d.offset + y1 * d.w + x0], c11 = texels[d.offset + y1 * d.w + x1];
    uint32_t out = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float v00 = (float)((c00 >> (8 * i)) & 0xFFu), v10 = (float)((c10 >> (8 * i)) & 0xFFu);
        const float v01 = (float)((c01 >> (8 * i)) & 0xFFu), v11 = (float)((c11 >> (8 * i)) & 0xFFu);
        const float a = v00 + dx * (v10 - v00);
        const float b = v01 + dx * (v11 - v01);
        const float c = a + dy * (b - a);
        out |= min(sat_u32(roundf(c)), 255u) << (8 * i);
    }
    return out;
}
__device__ __forceinline__ uint32_t sample_texture(const DevTexDesc &d, const uint32_t *texels, float u, float v, uint32_t sample_mode,
                                                   uint32_t repeat_mode) {
    switch (repeat_mode) {
        case RXR_REPEAT_CLAMP_XY:
            u = rclamp(u, 0.0f, 1.0f);
            v = rclamp(v, 0.0f, 1.0f);
            break;
        case RXR_REPEAT_REPEAT_XY:
            u = u - floorf(u);
            v = v - floorf(v);
            break;
        case RXR_REPEAT_REPEAT_X:
            u = u - floorf(u);
            v = rclamp(v, 0.0f, 1.0f);
            break;
        default:  // RepeatY
            u = rclamp(u, 0.0f, 1.0f);
            v = v - floorf(v);
            break;
    }
    return sample_mode == RXR_SAMPLE_NEAREST ? sample_nearest(d, texels, u, v) : sample_linear(d, texels, u, v);
}

// Chunk::sample_terrain_texture(world_pos, Vec2::one()) (chunk.rs:133-151) with Texture::get_pixel: rxr_kernels.hip's terrain_texel
__device__ __forceinline__ uint32_t terrain_texel(const uint32_t *rec, const uint32_t *pool, float wx, float wy) {
    const uint32_t w = rec[1], h = rec[2];
    const float ppt = (float)(int32_t)rec[5];
    const float local_x = (wx / 1.0f) - (float)(int32_t)rec[3];
    const float local_y = (wy / 1.0f) - (float)(int32_t)rec[4];
    const float pixel_x = local_x * ppt, pixel_y = local_y * ppt;
    const uint32_t px = min(sat_u32(rclamp(floorf(pixel_x), 0.0f, (float)w - 1.0f)), w - 1u);
    const uint32_t py = min(sat_u32(rclamp(floorf(pixel_y), 0.0f, (float)h - 1.0f)), h - 1u);
    return pool[rec[0] + py * w + px];
}

// ---- CompiledLight::color_at / radiance_at (map/light.rs:491-677): rxr_kernels.hip's smoothstep_rs / apply_flicker / light_color_at --
__device__ __forceinline__ float smoothstep_rs(float e0, float e1, float x) {
    const float t = rclamp((x - e0) / (e1 - e0), 0.0f, 1.0f);
    return t * t * (3.0f - 2.0f * t);
}
__device__ __forceinline__ F3 apply_flicker(const rxr_light &l, float intensity, uint32_t hash) {
    float ff;
    if (l.flicker > 0.0f) {
        const uint32_t combined = hash + (sat_u32(l.position[0]) + sat_u32(l.position[1]) + sat_u32(l.position[2])) * 100u;
        const float fv = rclamp((float)combined / 4294967296.0f /* u32::MAX as f32 */, 0.0f, 1.0f);
        ff = 1.0f - fv * l.flicker;
    } else {
        ff = 1.0f;
    }
    return {l.color[0] * intensity * ff, l.color[1] * intensity * ff, l.color[2] * intensity * ff};
}
// color_at(point, hash, false); false for None
__device__ __forceinline__ bool light_color_at(const rxr_light &l, F3 point, uint32_t hash, F3 &out) {
    if (!l.emitting) return false;
    const F3 lp = arr3(l.position);
    switch (l.light_type) {
        case RXR_LIGHT_POINT: {
            const float distance = sqrtf(dot3(sub3(point, lp), sub3(point, lp)));
            if (distance >= l.end_distance) return false;
            if (distance <= l.start_distance) {
                out = apply_flicker(l, l.intensity, hash);
                return true;
            }
            out = apply_flicker(l, l.intensity * smoothstep_rs(l.end_distance, l.start_distance, distance), hash);
            return true;
        }
        case RXR_LIGHT_AMBIENT:
        case RXR_LIGHT_AMBIENT_DAYLIGHT:
            out = apply_flicker(l, l.intensity, hash);
            return true;
        case RXR_LIGHT_SPOT: {
            const F3 tp = sub3(point, lp);
            const float distance = sqrtf(dot3(tp, tp));
            if (distance >= l.end_distance) return false;
            const float att = (distance <= l.start_distance) ? 1.0f : 1.0f - ((distance - l.start_distance) / (l.end_distance - l.start_distance));
            const float angle = acosf(dot3(arr3(l.direction), normalized3(tp)));
            if (angle > l.cone_angle) return false;
            out = apply_flicker(l, l.intensity * att, hash);
            return true;
        }
        case RXR_LIGHT_AREA: {
            const F3 to_point = sub3(point, lp);
            const float distance = sqrtf(dot3(to_point, to_point));
            if (distance >= l.end_distance) return false;
            if (distance < 0.1f) {
                out = arr3(l.color);
                return true;
            }
            const float datt = (distance <= l.start_distance) ? 1.0f : smoothstep_rs(l.end_distance, l.start_distance, distance);
            const float area = l.width * l.height;
            const F3 direction = normalized3(to_point);
            float att;
            if (l.from_linedef) {
                att = datt * area * l.intensity;
            } else {
                const float aa = fmaxf(dot3(arr3(l.normal), direction), 0.0f);
                att = aa * datt * area * l.intensity;
            }
            out = {l.color[0] * att, l.color[1] * att, l.color[2] * att};
            return true;
        }
        default: {  // Daylight
            const F3 to_point = sub3(point, lp);
            const float distance = sqrtf(dot3(to_point, to_point));
            if (distance >= l.end_distance) return false;
            const F3 direction = normalized3(to_point);
            const float aa = fmaxf(dot3(arr3(l.normal), direction), 0.0f);
            const float datt = (distance <= l.start_distance) ? 1.0f : smoothstep_rs(l.end_distance, l.start_distance, distance);
            const float att = aa * datt * l.intensity;
            out = {l.color[0] * att, l.color[1] * att, l.color[2] * att};
            return true;
        }
    }
}
// radiance_at(point, Some(normal), hash) (light.rs:504-533)
__device__ __forceinline__ bool light_radiance_at(const rxr_light &l, F3 point, F3 n, uint32_t hash, F3 &out) {
    F3 incoming;
    if (!light_color_at(l, point, hash, incoming)) return false;
    if (l.light_type == RXR_LIGHT_AMBIENT || l.light_type == RXR_LIGHT_AMBIENT_DAYLIGHT || l.light_type == RXR_LIGHT_DAYLIGHT) {
        out = incoming;
        return true;
    }
    const F3 dir_to_light = normalized3(sub3(arr3(l.position), point));
    out = scale3(incoming, fmaxf(dot3(n, dir_to_light), 0.0f));
    return true;
}

// MaterialModifier::modify (shapestack/material.rs:80-110) over the texel as pixel_to_vec4 gives it
__device__ __forceinline__ float material_modify(uint32_t modifier, F3 c, float strength) {
    if (modifier == MOD_LUMINANCE || modifier == MOD_INV_LUMINANCE) {
        const float lum = (0.2126f * c.x + 0.7152f * c.y) + 0.0722f * c.z;
        return modifier == MOD_LUMINANCE ? lum * strength : (1.0f - lum) * strength;
    }
    if (modifier == MOD_SATURATION || modifier == MOD_INV_SATURATION) {
        const float mx = fmaxf(c.x, fmaxf(c.y, c.z)), mn = fminf(c.x, fminf(c.y, c.z));
        const float sat = mx > 0.0f ? (mx - mn) / mx : 0.0f;
        return modifier == MOD_SATURATION ? sat * strength : (1.0f - sat) * strength;
    }
    return strength;
}

// trace.rs:493-512 with its two draws handed in
__device__ __forceinline__ F3 sample_cosine(F3 n, float r1, float r2) {
    const float phi = (2.0f * PI_F) * r1;
    const float r = sqrtf(r2);
    const F3 local = {cosf(phi) * r, sinf(phi) * r, sqrtf(1.0f - r2)};
    const F3 w = n;
    const F3 a = fabsf(w.x) > 0.1f ? F3{0.0f, 1.0f, 0.0f} : F3{1.0f, 0.0f, 0.0f};
    const F3 v = normalized3(cross3(w, a));
    const F3 u = cross3(v, w);
    return normalized3(add3(add3(scale3(u, local.x), scale3(v, local.y)), scale3(w, local.z)));
}

__device__ __forceinline__ void retire(const TraceArgs &A, uint32_t ray) {
    A.live[ray] = 0u;
    const float nan = __uint_as_float(0x7FC00000u);
    store3(A.origins, ray, {nan, nan, nan});   // (Batch3D::intersect's `u` is a NaN for every triangle: rejected)
}

// one bounce of rays r0 .. r0 + nr (trace.rs:188-331)
__global__ __launch_bounds__(TRACE_WG) void k_trace_shade(TraceArgs A, uint32_t r0, uint32_t nr) {
    const uint32_t r = blockIdx.x * TRACE_WG + threadIdx.x;
    if (r >= nr) return;
    const uint32_t ray = r0 + r;
    if (!A.live[ray]) return;
    // the fold: `hit.t < hitinfo.t` over the participating meshes in order
    unsigned long long best = RXR_ISECT_NO_HIT;
    uint32_t bseg = 0;
    if (A.keys) {
        const unsigned long long *slot = A.keys + (uint64_t)r * A.nseg;
        for (uint32_t s = 0; s < A.nseg; ++s) {
            if (A.segs[RXR_ISECT_SEG_WORDS * s + 4] != SEG_TRACED) continue;
            const unsigned long long key = slot[s];
            if (key < best) best = key, bseg = s;
        }
    }
    if (best == RXR_ISECT_NO_HIT) {   // a miss adds nothing (no render graph) and ends the path
        retire(A, ray);
        return;
    }
    const float t = __uint_as_float((uint32_t)(best >> 32));
    const uint32_t g = (uint32_t)best;
    const uint32_t m = last_le(A.tin_prefix, A.segs[RXR_ISECT_SEG_WORDS * bseg + 2], A.segs[RXR_ISECT_SEG_WORDS * bseg + 3], g);
    const F3 o = load3(A.origins, ray), dir = load3(A.dirs, ray);
    // Batch3D::intersect(ray, false)'s uv and normal (batch3d.rs:906-940), as k_isect_fold computes them
    const float *tp = A.tris + g;
    const size_t st = A.stride;
    float tt, u = 0.0f, v = 0.0f;
    (void)mt_test(o, normalized3(dir), {tp[0], tp[st], tp[2 * st]}, {tp[3 * st], tp[4 * st], tp[5 * st]}, {tp[6 * st], tp[7 * st], tp[8 * st]}, tt, u, v);
    const float w = (1.0f - u) - v;
    const uint32_t vb = A.vin_prefix[m];
    const uint32_t i0 = vb + A.obj_idx[3ull * g], i1 = vb + A.obj_idx[3ull * g + 1], i2 = vb + A.obj_idx[3ull * g + 2];
    const float2 uv0 = A.obj_uvs[i0], uv1 = A.obj_uvs[i1], uv2 = A.obj_uvs[i2];
    const float uvx = (w * uv0.x + u * uv1.x) + v * uv2.x, uvy = (w * uv0.y + u * uv1.y) + v * uv2.y;
    const F3 n0 = load3(A.obj_normals, i0), n1 = load3(A.obj_normals, i1), n2 = load3(A.obj_normals, i2);
    F3 n = normalized3({(n0.x * w + n1.x * u) + n2.x * v, (n0.y * w + n1.y * u) + n2.y * v, (n0.z * w + n1.z * u) + n2.z * v});
    if (dot3(n, dir) > 0.0f) n = {-n.x, -n.y, -n.z};

    // evaluate_hit (trace.rs:377-475)
    const uint32_t *M = A.mesh_rec + (size_t)MESH_WORDS * m;
    const F3 world = add3(o, scale3(dir, t));   // ray.at(t)
    uint32_t texel = 0u;
    if (M[MR_KIND] == TEXEL_PIXEL) texel = M[MR_PIXEL];
    else if (M[MR_KIND] == TEXEL_TEXTURE) texel = sample_texture(A.tex[M[MR_TEX]], A.texels, uvx, uvy, A.sample_mode, M[MR_REPEAT]);
    else if (M[MR_KIND] == TEXEL_TERRAIN) texel = terrain_texel(A.terrain_rec + (size_t)TERRAIN_WORDS * M[MR_TEX], A.chunk_texels, world.x, world.z);
    const uint32_t b0 = texel & 0xFFu, b1 = (texel >> 8) & 0xFFu, b2 = (texel >> 16) & 0xFFu;
    const F3 tex_lin = {A.srgb[b0], A.srgb[b1], A.srgb[b2]};
    float specular_weight = 0.0f;
    F3 emissive = {0.0f, 0.0f, 0.0f};
    if (M[MR_ROLE] != RXR_TRACE_NO_MATERIAL) {
        const float mvalue = __uint_as_float(M[MR_VALUE]);
        const float value = material_modify(M[MR_MODIFIER], {(float)b0 * INV_255, (float)b1 * INV_255, (float)b2 * INV_255}, mvalue);
        switch (M[MR_ROLE]) {
            case ROLE_MATTE: specular_weight = 1.0f - value; break;
            case ROLE_GLOSSY:
            case ROLE_METALLIC: specular_weight = value; break;   // (Metallic's tint lands in a texel nothing reads afterwards)
            case ROLE_EMISSIVE: emissive = scale3(scale3(tex_lin, mvalue), 10.0f); break;
            default: break;
        }
    }
    const F3 albedo = tex_lin;

    F3 thr = load3(A.thr, ray), ret = load3(A.ret, ray);
    if (emissive.x != 0.0f || emissive.y != 0.0f || emissive.z != 0.0f) {
        store3(A.ret, ray, add3(ret, mul3(emissive, thr)));
        retire(A, ray);
        return;
    }
    // direct lighting
    F3 direct = {0.0f, 0.0f, 0.0f};
    for (uint32_t li = 0; li < A.n_lights; ++li) {
        F3 lc;
        if (light_radiance_at(A.lights[li], world, n, A.hash_anim, lc)) direct = add3(direct, scale3(lc, 10.0f));
    }
    ret = add3(ret, mul3(direct, mul3(thr, div3(albedo, PI_F))));
    store3(A.ret, ray, ret);

    // the new direction
    const uint32_t slot = 2u + 4u * A.bounce;
    const float r_spec = trace_rand(A.seed, A.frame, ray, slot), r1 = trace_rand(A.seed, A.frame, ray, slot + 1u);
    const float r2 = trace_rand(A.seed, A.frame, ray, slot + 2u), r_roulette = trace_rand(A.seed, A.frame, ray, slot + 3u);
    const float p_spec = rclamp(specular_weight, 0.0f, 1.0f);
    const float p_diff = 1.0f - p_spec;
    const bool choose_spec = r_spec < p_spec;
    const float pdf = choose_spec ? p_spec : p_diff;
    F3 ndir;
    if (choose_spec) {
        ndir = sub3(dir, scale3(n, 2.0f * dot3(dir, n)));   // reflect: i - 2.0 * i.dot(n) * n
        thr = scale3(thr, specular_weight / pdf);
    } else {
        ndir = sample_cosine(n, r1, r2);
        thr = mul3(thr, div3(scale3(albedo, p_diff), pdf * PI_F));
    }
    // ray.dir is assigned first: ray.at(t) runs along the NEW direction (trace.rs:301-309)
    const F3 norigin = add3(add3(o, scale3(ndir, t)), scale3(n, 0.01f));
    // Russian roulette
    const float p = rclamp(fmaxf(thr.x, fmaxf(thr.y, thr.z)), 0.001f, 1.0f);
    if (r_roulette > p) {
        retire(A, ray);
        return;
    }
    thr = scale3(thr, 1.0f / p);
    store3(A.origins, ray, norigin);
    store3(A.dirs, ray, ndir);
    store3(A.thr, ray, thr);
}

// trace.rs:359-374: old * (1 - t) + new * t with new = (ret, 1)
__global__ __launch_bounds__(TRACE_WG) void k_trace_accumulate(const float *ret, float4 *accum, uint32_t n, float t) {
    const uint32_t i = blockIdx.x * TRACE_WG + threadIdx.x;
    if (i >= n) return;
    const float4 old = accum[i];
    const float k = 1.0f - t;
    accum[i] = make_float4(old.x * k + ret[3 * (uint64_t)i] * t, old.y * k + ret[3 * (uint64_t)i + 1] * t, old.z * k + ret[3 * (uint64_t)i + 2] * t,
                           old.w * k + 1.0f * t);
}

// AccumBuffer::linear_to_srgb_u8 and the alpha byte (buffer.rs:68-91)
__device__ __forceinline__ uint32_t linear_to_srgb_u8(float x) {
    const float srgb = x <= 0.0031308f ? x * 12.92f : 1.055f * powf(x, 1.0f / 2.4f) - 0.055f;
    return min(sat_u32(rclamp(srgb, 0.0f, 1.0f) * 255.0f + 0.5f), 255u);
}
__global__ __launch_bounds__(TRACE_WG) void k_accum_to_rgba(const float4 *accum, uint32_t *rgba, uint32_t n) {
    const uint32_t i = blockIdx.x * TRACE_WG + threadIdx.x;
    if (i >= n) return;
    const float4 a = accum[i];
    const uint32_t alpha = min(sat_u32(rclamp(a.w, 0.0f, 1.0f) * 255.0f + 0.5f), 255u);
    rgba[i] = linear_to_srgb_u8(a.x) | (linear_to_srgb_u8(a.y) << 8) | (linear_to_srgb_u8(a.z) << 16) | (alpha << 24);
}

// trace.rs:14-20 over pixel_to_vec4's 256 values, with the host's powf
const float *srgb_table() {
    static const std::vector<float> table = [] {
        std::vector<float> t(256);
        for (int b = 0; b < 256; ++b) {
            const float c = (float)b * INV_255;
            t[b] = c <= 0.04045f ? c / 12.92f : std::pow((c + 0.055f) / 1.055f, 2.4f);
        }
        return t;
    }();
    return table.data();
}

// trace.rs:119-128
uint32_t hash_u32(uint32_t seed) {
    uint32_t state = seed;
    state = (state ^ 61u) ^ (state >> 16);
    state = state + (state << 3);
    state ^= state >> 4;
    state = state * 0x27d4eb2du;
    state ^= state >> 15;
    return state;
}

bool traced_list(uint32_t list) {
    return list == RXR_LIST_CHUNK || list == RXR_LIST_CHUNK_TERRAIN || list == RXR_LIST_STATIC || list == RXR_LIST_DYNAMIC;
}

int check_scene(const uint32_t *material_kinds, const float *material_values, uint32_t n_meshes, const rxr_light *lights, uint32_t n_lights,
                uint32_t sample_mode, std::string &err) {
    if (n_lights && !lights) return err = "trace scene: lights is NULL with n_lights > 0", RXR_ERR_INVALID;
    if (n_lights > RXR_TRACE_MAX_LIGHTS) return err = "trace scene: more than RXR_TRACE_MAX_LIGHTS lights", RXR_ERR_UNSUPPORTED;
    if (sample_mode != RXR_SAMPLE_NEAREST && sample_mode != RXR_SAMPLE_LINEAR) return err = "trace scene: unknown sample mode", RXR_ERR_INVALID;
    if ((material_kinds == nullptr) != (material_values == nullptr))
        return err = "trace scene: material_kinds and material_values come together (or both NULL)", RXR_ERR_INVALID;
    for (uint32_t i = 0; i < n_lights; ++i)
        if (lights[i].light_type > RXR_LIGHT_DAYLIGHT) return err = "trace scene: light " + std::to_string(i) + ": unknown light type", RXR_ERR_INVALID;
    if (material_kinds)
        for (uint32_t m = 0; m < n_meshes; ++m) {
            const uint32_t role = material_kinds[2 * m], modifier = material_kinds[2 * m + 1];
            if (role != RXR_TRACE_NO_MATERIAL && role > ROLE_EMISSIVE) return err = "trace scene: mesh " + std::to_string(m) + ": unknown material role", RXR_ERR_INVALID;
            if (modifier > MOD_INV_SATURATION) return err = "trace scene: mesh " + std::to_string(m) + ": unknown material modifier", RXR_ERR_INVALID;
        }
    return RXR_OK;
}

// n_frames samples of width x height pixels into dev_accum, queued on `s`
int trace_run(rxr_ctx *ctx, const TraceCamera &cam, uint32_t first_frame, uint32_t n_frames, uint32_t seed, uint32_t bounces, float *dev_accum,
              hipStream_t s) {
    const uint32_t n = cam.width * cam.height;
    // the triangle records are the picking lane's, the rest this lane's
    int rc = rxr_query_begin(ctx, ctx->lane[Q_ISECT], s);
    if (rc != RXR_OK || (rc = rxr_query_begin(ctx, ctx->lane[Q_TRACE], s)) != RXR_OK) return rc;
    if ((rc = rxr_isect_prepare(ctx, s)) != RXR_OK || (rc = rxr_ray_accel_begin_call(ctx, s)) != RXR_OK) return rc;
    const uint32_t nseg = ctx->trace_nseg, ntri = ctx->PP.n_tris_in;
    const uint32_t per_batch = std::max(1u, rxr_isect_batch_rays(n, nseg));
    const size_t n3 = align_up((size_t)n * 12, 256);
    if ((rc = rxr_ensure(ctx, ctx->d_trace_paths, 4 * n3 + (size_t)n * 4)) != RXR_OK) return rc;
    if ((rc = rxr_ensure(ctx, ctx->d_trace_keys, std::max<size_t>((size_t)std::min(per_batch, n) * nseg * 8, 256))) != RXR_OK) return rc;
    uint8_t *pb = (uint8_t *)ctx->d_trace_paths.p;
    const uint8_t *sc = (const uint8_t *)ctx->d_trace_scene.p;
    TraceArgs A{};
    A.tris = (const float *)ctx->d_isect_tris.p;
    A.stride = ctx->isect_stride;
    A.nseg = nseg;
    A.segs = (const uint32_t *)(sc + ctx->trace_off[0]);
    A.tin_prefix = ctx->PP.tin_prefix;
    A.vin_prefix = ctx->PP.vin_prefix;
    A.obj_idx = ctx->PP.obj_idx;
    A.obj_uvs = ctx->PP.obj_uvs;
    A.obj_normals = ctx->PP.obj_normals;
    A.mesh_rec = (const uint32_t *)(sc + ctx->trace_off[1]);
    A.lights = (const rxr_light *)(sc + ctx->trace_off[2]);
    A.srgb = (const float *)(sc + ctx->trace_off[3]);
    A.terrain_rec = (const uint32_t *)(sc + ctx->trace_off[4]);
    A.chunk_texels = (const uint32_t *)ctx->ctex.pool.p;
    A.tex = (const DevTexDesc *)ctx->d_tex.p;
    A.texels = (const uint32_t *)ctx->d_texels.p;
    A.n_lights = ctx->trace_n_lights;
    A.hash_anim = ctx->trace_hash_anim;
    A.sample_mode = ctx->trace_sample_mode;
    A.origins = (float *)pb;
    A.dirs = (float *)(pb + n3);
    A.thr = (float *)(pb + 2 * n3);
    A.ret = (float *)(pb + 3 * n3);
    A.live = (uint32_t *)(pb + 4 * n3);
    A.seed = seed;
    const bool has_tris = ntri && nseg;
    const dim3 all((n + TRACE_WG - 1) / TRACE_WG), wg(TRACE_WG);
    for (uint32_t k = 0; k < n_frames; ++k) {
        A.frame = first_frame + k;
        A.keys = nullptr;
        hipLaunchKernelGGL(k_trace_rays, all, wg, 0, s, cam, A, n);
        HIPCHK(ctx, hipGetLastError());
        for (uint32_t b = 0; b < bounces; ++b) {
            A.bounce = b;
            for (uint32_t r0 = 0; r0 < n; r0 += per_batch) {
                const uint32_t nr = std::min(per_batch, n - r0);
                A.keys = has_tris ? (const unsigned long long *)ctx->d_trace_keys.p : nullptr;
                if (has_tris && (rc = rxr_isect_closest(ctx, A.segs, nseg, A.origins, A.dirs, r0, nr, (unsigned long long *)ctx->d_trace_keys.p, s)) != RXR_OK)
                    return rc;
                hipLaunchKernelGGL(k_trace_shade, dim3((nr + TRACE_WG - 1) / TRACE_WG), wg, 0, s, A, r0, nr);
                HIPCHK(ctx, hipGetLastError());
            }
        }
        const float t = 1.0f / ((float)A.frame + 1.0f);
        hipLaunchKernelGGL(k_trace_accumulate, all, wg, 0, s, A.ret, (float4 *)dev_accum, n, t);
        HIPCHK(ctx, hipGetLastError());
    }
    if ((rc = rxr_query_end(ctx, ctx->lane[Q_ISECT], s)) != RXR_OK) return rc;
    return rxr_query_end(ctx, ctx->lane[Q_TRACE], s);
}

// the checks rxr_trace and rxr_trace_to share; fills `cam`
int trace_check(rxr_ctx *ctx, const char *who, uint32_t camera_kind, const float *camera, uint32_t width, uint32_t height, uint32_t n_frames,
                uint32_t bounces, const float *accum, TraceCamera &cam) {
    const std::string w = who;
    if (!camera || !accum) return rxr_fail(ctx, RXR_ERR_INVALID, w + ": NULL camera or accumulation buffer");
    if (!width || !height || !n_frames) return rxr_fail(ctx, RXR_ERR_INVALID, w + ": width, height and n_frames must be at least 1");
    if (width > (1u << 24) || height > (1u << 24) || (uint64_t)width * height > (1ull << 28))
        return rxr_fail(ctx, RXR_ERR_INVALID, w + ": at most 2^24 pixels a side and 2^28 in all");
    if (camera_kind > RXR_TRACE_CAMERA_ISO) return rxr_fail(ctx, RXR_ERR_INVALID, w + ": unknown camera kind");
    if (bounces > RXR_TRACE_MAX_BOUNCES) return rxr_fail(ctx, RXR_ERR_UNSUPPORTED, w + ": more than RXR_TRACE_MAX_BOUNCES bounces");
    cam.kind = camera_kind;
    cam.width = width;
    cam.height = height;
    memcpy(cam.pos, camera, 12);
    memcpy(cam.forward, camera + 3, 12);
    memcpy(cam.right, camera + 6, 12);
    memcpy(cam.up, camera + 9, 12);
    cam.half_width = camera[12];
    cam.half_height = camera[13];
    return RXR_OK;
}
int trace_ready(rxr_ctx *ctx, const char *who) {
    if (!ctx->meshes_valid || !ctx->trace_set)
        return rxr_fail(ctx, RXR_ERR_INVALID, std::string(who) + ": no rxr_set_trace_scene since the last rxr_set_meshes / rxr_set_textures");
    return RXR_OK;
}

}  // namespace

extern "C" {

int rxr_check_trace_scene(const uint32_t *material_kinds, const float *material_values, uint32_t n_meshes, const rxr_light *lights,
                          uint32_t n_lights, uint32_t sample_mode, char *message, uint32_t message_capacity) {
    std::string err;
    const int rc = check_scene(material_kinds, material_values, n_meshes, lights, n_lights, sample_mode, err);
    rxr_copy_message(err, message, message_capacity);
    return rc;
}

int rxr_set_trace_scene(rxr_ctx *ctx, const uint32_t *material_kinds, const float *material_values, uint32_t n_meshes,
                        const rxr_light *lights, uint32_t n_lights, uint32_t sample_mode, uint64_t animation_frame,
                        const int32_t *chunk_origin_size, uint32_t n_chunks) {
    if (!ctx) return RXR_ERR_INVALID;
    if (ctx->group)
        return rxr_as_member0(ctx, [&](rxr_ctx *m) { return rxr_set_trace_scene(m, material_kinds, material_values, n_meshes, lights, n_lights, sample_mode, animation_frame, chunk_origin_size, n_chunks); });
    std::string err;
    int rc = check_scene(material_kinds, material_values, n_meshes, lights, n_lights, sample_mode, err);
    if (rc != RXR_OK) return rxr_fail(ctx, rc, "rxr_set_trace_scene: " + err);
    if (!ctx->meshes_valid) return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_set_trace_scene: the last rxr_set_meshes failed: no meshes are registered");
    if (n_meshes != ctx->meshes.size()) return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_set_trace_scene: n_meshes is not the count of the last rxr_set_meshes");
    if (n_chunks && !chunk_origin_size) return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_set_trace_scene: chunk_origin_size is NULL with n_chunks > 0");
    // the blob: segments, mesh records, lights, sRGB table
    std::vector<uint32_t> segs, recs((size_t)MESH_WORDS * n_meshes, 0u), terrain;
    uint32_t nseg = 0;
    for (uint32_t m = 0; m < n_meshes; ++m) {
        const HostMesh &M = ctx->meshes[m];
        const bool traced = traced_list(M.list);
        uint32_t *R = recs.data() + (size_t)MESH_WORDS * m;
        R[MR_ROLE] = material_kinds ? material_kinds[2 * m] : RXR_TRACE_NO_MATERIAL;
        R[MR_MODIFIER] = material_kinds ? material_kinds[2 * m + 1] : 0u;
        if (material_values) memcpy(&R[MR_VALUE], &material_values[m], 4);
        R[MR_REPEAT] = M.repeat_mode;
        R[MR_KIND] = TEXEL_ZERO;
        if (traced && M.dev.n_tris) {
            const std::string who = "rxr_set_trace_scene: mesh " + std::to_string(m);
            switch (M.source.kind) {
                case RXR_SOURCE_PIXEL:
                    R[MR_KIND] = TEXEL_PIXEL;
                    R[MR_PIXEL] = pack_px(M.source.pixel);
                    break;
                case RXR_SOURCE_STATIC_TILE:
                case RXR_SOURCE_DYNAMIC_TILE: {
                    const std::vector<TileRange> &tiles = M.source.kind == RXR_SOURCE_STATIC_TILE ? ctx->tiles_static : ctx->tiles_dynamic;
                    if (M.source.index >= tiles.size()) return rxr_fail(ctx, RXR_ERR_INVALID, who + ": its tile does not exist (the reference panics)");
                    const TileRange &tr = tiles[M.source.index];
                    if (!tr.n) return rxr_fail(ctx, RXR_ERR_INVALID, who + ": its tile has no texture (`% 0` panics)");
                    R[MR_KIND] = TEXEL_TEXTURE;
                    R[MR_TEX] = tr.first + (uint32_t)(animation_frame % tr.n);
                    break;
                }
                case RXR_SOURCE_TERRAIN: {
                    if (M.chunk < 0) break;   // (no chunk: Vec4::zero)
                    const ChunkTextures &T = ctx->ctex;
                    if (!T.set || (size_t)M.chunk >= T.terrain.size())
                        return rxr_fail(ctx, RXR_ERR_UNSUPPORTED, who + ": PixelSource::Terrain, and no resident chunk texture is registered for its chunk (rxr_set_chunk_textures)");
                    if ((uint32_t)M.chunk >= n_chunks) return rxr_fail(ctx, RXR_ERR_INVALID, who + ": PixelSource::Terrain, and chunk_origin_size does not reach its chunk");
                    const int32_t slot = T.terrain[M.chunk];
                    if (slot < 0) break;      // (terrain_texture is None: [0, 0, 0, 0], chunk.rs:150)
                    const int32_t *C = chunk_origin_size + 3 * (size_t)M.chunk;
                    if (C[2] < 1) return rxr_fail(ctx, RXR_ERR_INVALID, who + ": its chunk's size is below 1 (`texture.width as i32 / self.size` panics at 0)");
                    const ChunkTextures::Slot &S = T.slots[slot];
                    R[MR_KIND] = TEXEL_TERRAIN;
                    R[MR_TEX] = (uint32_t)(terrain.size() / TERRAIN_WORDS);
                    const uint32_t rec[TERRAIN_WORDS] = {S.offset, S.w, S.h, (uint32_t)C[0], (uint32_t)C[1], (uint32_t)((int32_t)S.w / C[2])};
                    terrain.insert(terrain.end(), rec, rec + TERRAIN_WORDS);
                    break;
                }
                case RXR_HOST_SOURCE_ENTITY_TILE:
                case RXR_HOST_SOURCE_ITEM_TILE: return rxr_fail(ctx, RXR_ERR_INVALID, who + ": a host-side source kind (the host resolves it, include/rxr.h)");
                default: break;   // Vec4::zero
            }
        }
        if (!M.dev.n_tris) continue;   // (no hit: nothing to fold, and no reason to end a run)
        const uint32_t rule = traced ? SEG_TRACED : SEG_IGNORED;
        if (nseg && segs[RXR_ISECT_SEG_WORDS * (nseg - 1) + 4] == rule) {
            segs[RXR_ISECT_SEG_WORDS * (nseg - 1) + 1] = M.dev.tin_base + M.dev.n_tris;
            segs[RXR_ISECT_SEG_WORDS * (nseg - 1) + 3] = m + 1;
            continue;
        }
        const uint32_t seg[RXR_ISECT_SEG_WORDS] = {M.dev.tin_base, M.dev.tin_base + M.dev.n_tris, m, m + 1, rule, 0u};
        segs.insert(segs.end(), seg, seg + RXR_ISECT_SEG_WORDS);
        ++nseg;
    }
    BlobCursor take;
    const size_t off[5] = {take(segs.size() * 4), take(recs.size() * 4), take((size_t)n_lights * sizeof(rxr_light)), take(256 * 4), take(terrain.size() * 4)};
    std::vector<uint8_t> blob(take.o, 0);
    if (!segs.empty()) memcpy(blob.data() + off[0], segs.data(), segs.size() * 4);
    if (!recs.empty()) memcpy(blob.data() + off[1], recs.data(), recs.size() * 4);
    if (n_lights) memcpy(blob.data() + off[2], lights, (size_t)n_lights * sizeof(rxr_light));
    memcpy(blob.data() + off[3], srgb_table(), 256 * 4);
    if (!terrain.empty()) memcpy(blob.data() + off[4], terrain.data(), terrain.size() * 4);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if ((rc = rxr_quiesce(ctx)) != RXR_OK) return rc;   // (a trace queued on the caller's stream reads the old blob)
    if ((rc = rxr_ensure(ctx, ctx->d_trace_scene, blob.size())) != RXR_OK) return rc;
    ctx->trace_set = false;
    HIPCHK(ctx, hipMemcpyAsync(ctx->d_trace_scene.p, blob.data(), blob.size(), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(ctx->trace_off, off, sizeof(off));
    ctx->trace_nseg = nseg;
    ctx->trace_n_lights = n_lights;
    ctx->trace_sample_mode = sample_mode;
    ctx->trace_hash_anim = hash_u32((uint32_t)animation_frame);
    ctx->trace_set = true;
    return RXR_OK;
}

float rxr_trace_rand(uint32_t seed, uint32_t frame, uint32_t pixel, uint32_t slot) { return trace_rand(seed, frame, pixel, slot); }

int rxr_trace_srgb_table(rxr_ctx *ctx, float out[256]) {
    if (!out) return ctx ? rxr_fail(ctx, RXR_ERR_INVALID, "rxr_trace_srgb_table: out is NULL") : RXR_ERR_INVALID;
    memcpy(out, srgb_table(), 256 * 4);
    return RXR_OK;
}

int rxr_trace(rxr_ctx *ctx, uint32_t camera_kind, const float *camera, uint32_t width, uint32_t height, uint32_t first_frame,
              uint32_t n_frames, uint32_t seed, uint32_t bounces, float *accum) {
    if (!ctx) return RXR_ERR_INVALID;
    TraceCamera cam{};
    int rc = trace_check(ctx, "rxr_trace", camera_kind, camera, width, height, n_frames, bounces, accum, cam);
    if (rc != RXR_OK) return rc;
    if (ctx->group)
        return rxr_as_member0(ctx, [&](rxr_ctx *m) { return rxr_trace(m, camera_kind, camera, width, height, first_frame, n_frames, seed, bounces, accum); });
    if ((rc = trace_ready(ctx, "rxr_trace")) != RXR_OK) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    QueryIO io{ctx, ctx->lane[Q_TRACE]};
    const unsigned i_acc = io.inout(accum, (size_t)width * height * 16);
    if ((rc = io.upload()) != RXR_OK) return rc;
    if ((rc = trace_run(ctx, cam, first_frame, n_frames, seed, bounces, io.dev<float>(i_acc), ctx->stream)) != RXR_OK) return rc;
    rc = io.download();
    if (rc == RXR_OK) rxr_query_drained(ctx->lane[Q_ISECT]);   // (its event lies behind on the stream that was just synchronised)
    return rc;
}

int rxr_trace_to(rxr_ctx *ctx, uint32_t camera_kind, const float *camera, uint32_t width, uint32_t height, uint32_t first_frame,
                 uint32_t n_frames, uint32_t seed, uint32_t bounces, float *dev_accum, void *hip_stream) {
    if (!ctx) return RXR_ERR_INVALID;
    TraceCamera cam{};
    int rc = trace_check(ctx, "rxr_trace_to", camera_kind, camera, width, height, n_frames, bounces, dev_accum, cam);
    if (rc != RXR_OK) return rc;
    if (ctx->group) return rxr_fail(ctx, RXR_ERR_UNSUPPORTED, "rxr_trace_to on a multi-device context: device pointers and streams belong to ONE device (use rxr_member)");
    if ((rc = trace_ready(ctx, "rxr_trace_to")) != RXR_OK) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (((uintptr_t)dev_accum & 15u) || !rxr_on_device(ctx, dev_accum, (size_t)width * height * 16))
        return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_trace_to: dev_accum is not 16-byte aligned memory of the context's device");
    return trace_run(ctx, cam, first_frame, n_frames, seed, bounces, dev_accum, hip_stream ? (hipStream_t)hip_stream : ctx->stream);
}

int rxr_accum_to_rgba_to(rxr_ctx *ctx, const float *dev_accum, uint32_t width, uint32_t height, uint8_t *dev_rgba, void *hip_stream) {
    if (!ctx) return RXR_ERR_INVALID;
    if (!dev_accum || !dev_rgba) return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_accum_to_rgba_to: NULL buffer");
    if (!width || !height || (uint64_t)width * height > (1ull << 28)) return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_accum_to_rgba_to: 1 to 2^28 pixels");
    if (ctx->group) return rxr_fail(ctx, RXR_ERR_UNSUPPORTED, "rxr_accum_to_rgba_to on a multi-device context: device pointers and streams belong to ONE device (use rxr_member)");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const uint32_t n = width * height;
    if (((uintptr_t)dev_accum & 15u) || ((uintptr_t)dev_rgba & 3u) || !rxr_on_device(ctx, dev_accum, (size_t)n * 16) || !rxr_on_device(ctx, dev_rgba, (size_t)n * 4))
        return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_accum_to_rgba_to: the buffers are not aligned memory of the context's device");
    hipLaunchKernelGGL(k_accum_to_rgba, dim3((n + TRACE_WG - 1) / TRACE_WG), dim3(TRACE_WG), 0, hip_stream ? (hipStream_t)hip_stream : ctx->stream,
                       (const float4 *)dev_accum, (uint32_t *)dev_rgba, n);
    HIPCHK(ctx, hipGetLastError());
    return RXR_OK;
}

int rxr_accum_to_rgba(rxr_ctx *ctx, const float *accum, uint32_t width, uint32_t height, uint8_t *rgba) {
    if (!ctx) return RXR_ERR_INVALID;
    if (!accum || !rgba) return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_accum_to_rgba: NULL buffer");
    if (!width || !height || (uint64_t)width * height > (1ull << 28)) return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_accum_to_rgba: 1 to 2^28 pixels");
    if (ctx->group) return rxr_as_member0(ctx, [&](rxr_ctx *m) { return rxr_accum_to_rgba(m, accum, width, height, rgba); });
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const uint32_t n = width * height;
    QueryIO io{ctx, ctx->lane[Q_TRACE]};
    const unsigned i_acc = io.in(accum, (size_t)n * 16), i_out = io.out(rgba, (size_t)n * 4);
    int rc = io.upload();
    if (rc != RXR_OK) return rc;
    if ((rc = rxr_query_begin(ctx, ctx->lane[Q_TRACE], ctx->stream)) != RXR_OK) return rc;
    hipLaunchKernelGGL(k_accum_to_rgba, dim3((n + TRACE_WG - 1) / TRACE_WG), dim3(TRACE_WG), 0, ctx->stream, io.dev<float4>(i_acc), io.dev<uint32_t>(i_out), n);
    HIPCHK(ctx, hipGetLastError());
    if ((rc = rxr_query_end(ctx, ctx->lane[Q_TRACE], ctx->stream)) != RXR_OK) return rc;
    return io.download();
}

}  // extern "C"
