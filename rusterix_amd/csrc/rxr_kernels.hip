// rxr_kernels.hip -- hand-written gfx950 (CDNA4) kernels for the Rusterix tile rasterizer hot path.
//
// Compile with -ffp-contract=off and WITHOUT fast-math: the arithmetic below restates the reference's
// f32 expressions operation for operation (Rust never contracts a*b+c); the only fused operations
// are the ones the reference itself fuses (vec4_to_pixel's mul_add, vek's Mat*Vec), written fmaf.
// hipcc's default IEEE-correct division / sqrt expansions are relied on (no -ffast-math, no
// __fdividef, no rsq shortcuts).
//
// Pipeline per frame (all on one stream):
//   k_setup3d  one thread per 3D triangle: de-indexes the batch arrays into TriSetup / TriShade
//              records (per-triangle constants of the reference's per-fragment formulas), computes
//              the triangle's clamped pixel box (rasterizer.rs:998-1017) and counts it into the
//              16x16-pixel bins it touches (or appends it to the large-triangle list).
//   k_scan     exclusive scan of the bin counts.
//   k_fill     writes triangle ids into the bin lists.
//   k_raster   one 256-thread workgroup per 16x16 tile, one pixel per lane:
//              visibility (edge functions, barycentrics, depth) over the tile's triangles, then ONE
//              shading evaluation of the winning fragment, then the 2D pass, then one store.
//
// Why visibility-then-shade equals the reference's immediate shading: d3_rasterize writes a
// fragment iff `z < z_buffer` (strict) and its encoded alpha is 255 (rasterizer.rs:1060, 1408), and
// a fragment's colour/alpha depend only on (triangle, pixel).  Processing triangles in submission
// order, the surviving fragment of a pixel is therefore the one with the smallest z among the
// alpha-255 fragments, ties broken by the smaller submission index -- an order-independent argmin,
// so the bins need not be sorted and overdraw is never shaded.
// RXR_JIT: this file compiled at RUN time by hiprtc (rxr_jit.hip) for one set of Rusteria programs -- only the raster kernel of
// the program levels, with the interpreter replaced by the straight-line code generated from the set's jump code.  hiprtc brings
// its own runtime declarations and no host headers; the pre-pass kernels and the launch functions are left out.
#ifndef RXR_JIT
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>

#include "rxr_debug.h"
#include "rxr_launch.h"
#include "rxr_route.h"
#endif

#include "rxr_device.h"
#include "rxr_exact_math.h"
#include "rxr_project.h"
#include "rxr_vm.h"

// occupancy of k_raster_vm / k_raster_vm_s / k_raster_vm_sv: 6 waves per SIMD = 80 VGPRs AND at most 26.6 KB of LDS per workgroup,
// which is why the interpreter's LDS value stack holds 2 entries per lane (rxr_vm.h, RXR_VM_LDS_STACK; the top of the stack lives
// in registers, so expressions up to depth 3 never touch scratch memory).  1 M triangles with the configuration-C5 program, raster
// kernel: 3 entries + 5 waves (96 VGPRs) 1178 us, 2 entries + 6 waves 1085 us, 1 entry + 7 waves (72 VGPRs, spills) 1337 us.
// (Before the interpreter's dispatch became a tree -- rxr_vm.h -- its state needed the registers and 6 waves lost to 5.)
#ifndef RXR_VM_WAVES_PER_SIMD
#define RXR_VM_WAVES_PER_SIMD 6
#endif
#ifndef RXR_VEK_FUSED_MATVEC
#define RXR_VEK_FUSED_MATVEC 1
#endif

// -DRXR_PHASE_TIMING=1 (tuning builds only): per-phase wave-cycle totals of the raster kernel, read with
// rxr_debug_phase_read; see tools/phase_timing.py
#ifndef RXR_PHASE_TIMING
#define RXR_PHASE_TIMING 0
#endif
#if RXR_PHASE_TIMING
__device__ unsigned long long g_phase[1024][16];  // spread over 1024 slots: same-address atomics would serialise
// slots: 0 prologue (+ opacity pass), 1 list staging / walk, 2 shade begin, 3 lights, 4 shade end, 5 2D pass, 6 store,
// 7 row mode (rows_round), 8 = number of waves, 9 rows_resolve, 10 per-pixel walk of a binned round
struct PhaseClock {
    unsigned long long t, acc[12];
};
#define PHASE_DECL PhaseClock ph_clock = {__builtin_readcyclecounter(), {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}}; PhaseClock *const ph = &ph_clock
#define PHASE_PARAM , PhaseClock *ph
#define PHASE_ARG , ph
#define PHASE_MARK(k)                                          \
    do {                                                       \
        unsigned long long now_ = __builtin_readcyclecounter(); \
        ph->acc[k] += now_ - ph->t;                            \
        ph->t = now_;                                          \
    } while (0)
#define PHASE_FLUSH                                                              \
    do {                                                                         \
        if ((threadIdx.x & 63u) == 0) {                                          \
            unsigned slot_ = ((blockIdx.y * gridDim.x + blockIdx.x) * 4u + (threadIdx.x >> 6)) & 1023u;                   \
            for (int k_ = 0; k_ < 12; ++k_) if (k_ != 8) atomicAdd(&g_phase[slot_][k_], ph->acc[k_]);   \
            atomicAdd(&g_phase[slot_][8], 1ull);                                        \
        }                                                                        \
    } while (0)
#else
#define PHASE_DECL
#define PHASE_PARAM
#define PHASE_ARG
#define PHASE_MARK(k)
#define PHASE_FLUSH
#endif

namespace {

struct f3 {
    float x, y, z;
};
// A record of a read-only table at a WAVE-UNIFORM index, fetched through the constant address space: scalar loads (s_load, scalar
// cache) instead of vector loads.  Behind any earlier store of the kernel the compiler can no longer prove that a plain global
// load is unclobbered and issues it as a VECTOR load plus v_readfirstlane -- for the lights that was an L2 round trip per light and
// wave on the critical path of the light loop (seen in the ISA: global_load_dwordx4 ... s_waitcnt vmcnt ... v_readfirstlane).
// Only fields that are used are loaded.  The tables (lights, linedefs) are written by the upload and never by a kernel.
template <class T>
__device__ __forceinline__ T uniform_record(const T *table, uint32_t i) {
    // word by word: a struct has no copy constructor from another address space; the loads are merged again (s_load_dwordx16 ...)
    static_assert(sizeof(T) % 4 == 0 && alignof(T) >= 4, "records of 32-bit fields");
    typedef const uint32_t __attribute__((address_space(4))) *word_ptr;
    const word_ptr src = (word_ptr)(table + i);
    T out;
    uint32_t *dst = reinterpret_cast<uint32_t *>(&out);
#pragma unroll
    for (uint32_t k = 0; k < sizeof(T) / 4; ++k) dst[k] = src[k];
    return out;
}
// the first 32 bytes of a record in ONE scalar load (the word-by-word form above lets the compiler fetch the fields where they are first used:
// several dependent scalar-cache round trips when the uses sit behind one another's branches)
template <class T>
__device__ __forceinline__ T uniform_record_x8(const T *table, uint32_t i) {
    static_assert(sizeof(T) >= 32 && sizeof(T) % 4 == 0, "the first eight 32-bit fields of a record");
    typedef uint32_t u32x8 __attribute__((ext_vector_type(8)));
    typedef const u32x8 __attribute__((address_space(4))) *vec_ptr;
    const u32x8 v = *(vec_ptr)(table + i);
    T out;
    uint32_t *dst = reinterpret_cast<uint32_t *>(&out);
#pragma unroll
    for (uint32_t k = 0; k < 8; ++k) dst[k] = v[k];
    return out;
}

__device__ __forceinline__ f3 mk3(float x, float y, float z) { return f3{x, y, z}; }
__device__ __forceinline__ f3 add3(f3 a, f3 b) { return f3{a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ f3 sub3(f3 a, f3 b) { return f3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ f3 mul3(f3 a, f3 b) { return f3{a.x * b.x, a.y * b.y, a.z * b.z}; }
__device__ __forceinline__ f3 scale3(f3 a, float s) { return f3{a.x * s, a.y * s, a.z * s}; }
__device__ __forceinline__ f3 div3(f3 a, float s) { return f3{a.x / s, a.y / s, a.z / s}; }
__device__ __forceinline__ f3 neg3(f3 a) { return f3{-a.x, -a.y, -a.z}; }
// vek: dot = left-to-right sum of products; magnitude = sqrt(dot); normalized = v / magnitude
__device__ __forceinline__ float dot3(f3 a, f3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ float mag3(f3 a) { return sqrtf(dot3(a, a)); }
__device__ __forceinline__ f3 norm3(f3 a) { return div3(a, mag3(a)); }
// |a| within 1 ulp (v_sqrt_f32), for BOUNDS only: the light culling's sphere radii, whose test carries a relative margin of 1e-3
__device__ __forceinline__ float mag3_bound(f3 a) { return __builtin_amdgcn_sqrtf(dot3(a, a)); }
// same values through the shared-reciprocal sequences of rxr_exact_math.h (bit-identical; cheaper
// unless a component is exactly zero, which sends the wave down the plain path)
__device__ __forceinline__ f3 norm3_fast(f3 a, float &mag) {
    f3 o;
    rxm::normalize3(a.x, a.y, a.z, o.x, o.y, o.z, mag);
    return o;
}
__device__ __forceinline__ f3 norm3_fast(f3 a) {
    float m;
    return norm3_fast(a, m);
}
// relaxed-light mode (RXR_LIGHT_MATH, shade3d_lights): measured 2 ulp per component and for the magnitude against the exact form,
// asserted within 4 and 3 (tests/test_gpu_exact_math_ref.py, profiles/exact_math/README.md)
__device__ __forceinline__ f3 norm3_relaxed(f3 a, float &mag) {
    f3 o;
    rxm::normalize3_relaxed(a.x, a.y, a.z, o.x, o.y, o.z, mag);
    return o;
}
// the variant for surface normals: components that are exactly zero stay on the short path
__device__ __forceinline__ f3 norm3_z(f3 a) {
    f3 o;
    rxm::normalize3_z(a.x, a.y, a.z, o.x, o.y, o.z);
    return o;
}

// Rust f32::clamp keeps NaN
__device__ __forceinline__ float rclamp(float x, float lo, float hi) { return x < lo ? lo : (x > hi ? hi : x); }

__device__ __forceinline__ float madd(float a, float b, float c) {
#if RXR_VEK_FUSED_MATVEC
    return fmaf(a, b, c);
#else
    return a * b + c;
#endif
}

// vek column-major Mat4 * Vec4 (m[c*4+r])
__device__ __forceinline__ void mat4_mul(const float *m, float x, float y, float z, float w, float &ox, float &oy,
                                         float &oz, float &ow) {
    ox = madd(m[12], w, madd(m[8], z, madd(m[4], y, m[0] * x)));
    oy = madd(m[13], w, madd(m[9], z, madd(m[5], y, m[1] * x)));
    oz = madd(m[14], w, madd(m[10], z, madd(m[6], y, m[2] * x)));
    ow = madd(m[15], w, madd(m[11], z, madd(m[7], y, m[3] * x)));
}

// `x as u8` / `as u32` with Rust semantics (saturate, NaN -> 0): the saturating hardware conversion (rxm::sat_u32) and an
// integer minimum -- two instructions where the compare-and-select form needs five
__device__ __forceinline__ uint32_t sat_u8(float x) { return min(rxm::sat_u32(x), 255u); }
// byte / 255.0 -- the correctly rounded quotient of the reference (NOT byte * (1/255): T5 keeps the two apart) -- through the short
// division chain of rxr_exact_math.h: the operands are statically inside its window, +0 included (selftest kind "static")
__device__ __forceinline__ float byte_over_255(uint32_t b) { return rxm::div1_known((float)b, 255.0f, true); }
__device__ __forceinline__ uint32_t sat_u32(float x) { return rxm::sat_u32(x); }
// `x as usize` followed by a clamp to [0, hi] (hi < 2^31)
__device__ __forceinline__ uint32_t sat_index(float x, uint32_t hi) { return rxr_sat_index(x, hi); }

// lib.rs:64-68
__device__ __forceinline__ uint32_t f32_to_u8_saturated(float x) {
    float y = fmaf(fminf(fmaxf(x, 0.0f), 1.0f), 255.0f, 0.5f);
    return (uint32_t)(int)y & 0xFFu;  // y in [0.5, 255.5]
}

// rasterizer.rs:19-33
__device__ __forceinline__ float srgb_to_linear_fast(float x) {
    float x2 = x * x;
    return (0.6975f * x2 + 0.3025f) * x;
}
__device__ __forceinline__ float linear_to_srgb_fast(float x) {
    float s = rxm::sqrt_exact(x);
    return 1.055f * s - 0.055f * s * s;
}

// ---- texture sampling (texture.rs:203-232, 307-323, 414-460) -------------------------------------
__device__ __forceinline__ uint32_t sample_nearest(const DevTexDesc &d, const uint32_t *texels, float u, float v) {
    uint32_t tx = sat_index(roundf(u * ((float)d.w - 1.0f)), d.w - 1u);
    uint32_t ty = sat_index(roundf(v * ((float)d.h - 1.0f)), d.h - 1u);
    return texels[d.offset + ty * d.w + tx];
}

__device__ __forceinline__ uint32_t sample_linear(const DevTexDesc &d, const uint32_t *texels, float u, float v) {
    float x = u * ((float)d.w - 1.0f);
    float y = v * ((float)d.h - 1.0f);
    float fx = floorf(x), fy = floorf(y);
    // `floor() as usize`: u,v are in [0,1] or NaN after the repeat handling, so x0 <= w-1
    uint32_t x0 = sat_index(fx, d.w - 1u);
    uint32_t y0 = sat_index(fy, d.h - 1u);
    uint32_t x1 = min(x0 + 1u, d.w - 1u);
    uint32_t y1 = min(y0 + 1u, d.h - 1u);
    float dx = x - fx, dy = y - fy;
    uint32_t c00 = texels[d.offset + y0 * d.w + x0];
    uint32_t c10 = texels[d.offset + y0 * d.w + x1];
    uint32_t c01 = texels[d.offset + y1 * d.w + x0];
    uint32_t c11 = texels[d.offset + y1 * d.w + x1];
    uint32_t out = 0;
    auto channel = [&](int i) {
        float v00 = (float)((c00 >> (8 * i)) & 0xFFu);
        float v10 = (float)((c10 >> (8 * i)) & 0xFFu);
        float v01 = (float)((c01 >> (8 * i)) & 0xFFu);
        float v11 = (float)((c11 >> (8 * i)) & 0xFFu);
        float a = v00 + dx * (v10 - v00);
        float b = v01 + dx * (v11 - v01);
        float c = a + dy * (b - a);
        out |= sat_u8(roundf(c)) << (8 * i);
    };
#pragma unroll
    for (int i = 0; i < 3; ++i) channel(i);
    // alpha: four texels of 255 interpolate to exactly 255 for finite weights (255 + dx * 0), so a wave whose lanes all sample
    // textures without a single non-opaque texel (DevTexDesc.all_opaque, set at upload) and whose weights are all numbers skips
    // the fourth channel -- a quarter of the interpolation arithmetic of the 1 M-triangle grid's fragments
    if (__ballot(!(d.all_opaque & 1u) || !(dx == dx) || !(dy == dy)) == 0ull) out |= 0xFF000000u;
    else channel(3);
    return out;
}

__device__ __forceinline__ uint32_t sample_texture(const DevTexDesc &d, const uint32_t *texels, float u, float v,
                                                   uint32_t sample_mode, uint32_t repeat_mode) {
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

// ---- lights (map/light.rs:491-677) ---------------------------------------------------------------
__device__ __forceinline__ float smoothstep_rs(float e0, float e1, float x) {
    float t = rclamp((x - e0) / (e1 - e0), 0.0f, 1.0f);
    return t * t * (3.0f - 2.0f * t);
}

__device__ __forceinline__ f3 apply_flicker(const rxr_light &l, float intensity, uint32_t hash) {
    float ff;
    if (l.flicker > 0.0f) {
        uint32_t combined = hash + (sat_u32(l.position[0]) + sat_u32(l.position[1]) + sat_u32(l.position[2])) * 100u;
        float fv = rclamp((float)combined / 4294967296.0f /* u32::MAX as f32 */, 0.0f, 1.0f);
        ff = 1.0f - fv * l.flicker;
    } else {
        ff = 1.0f;
    }
    return mk3(l.color[0] * intensity * ff, l.color[1] * intensity * ff, l.color[2] * intensity * ff);
}

// CompiledLight::color_at; returns false for None
__device__ __forceinline__ bool light_color_at(const rxr_light &l, f3 point, uint32_t hash, bool d2, f3 &out) {
    if (!l.emitting) return false;
    f3 lp = mk3(l.position[0], l.position[1], l.position[2]);
    switch (l.light_type) {
        case RXR_LIGHT_POINT: {
            float distance = mag3(sub3(point, lp));
            if (distance >= l.end_distance) return false;
            if (distance <= l.start_distance) {
                out = apply_flicker(l, l.intensity, hash);
                return true;
            }
            float att = smoothstep_rs(l.end_distance, l.start_distance, distance);
            out = apply_flicker(l, l.intensity * att, hash);
            return true;
        }
        case RXR_LIGHT_AMBIENT:
        case RXR_LIGHT_AMBIENT_DAYLIGHT:
            out = apply_flicker(l, l.intensity, hash);
            return true;
        case RXR_LIGHT_SPOT: {
            float distance = mag3(sub3(point, lp));
            if (distance >= l.end_distance) return false;
            float att = (distance <= l.start_distance)
                            ? 1.0f
                            : 1.0f - ((distance - l.start_distance) / (l.end_distance - l.start_distance));
            f3 dtp = norm3(sub3(point, lp));
            float angle = acosf(dot3(mk3(l.direction[0], l.direction[1], l.direction[2]), dtp));
            if (angle > l.cone_angle) return false;
            out = apply_flicker(l, l.intensity * att, hash);
            return true;
        }
        case RXR_LIGHT_AREA: {
            f3 to_point = sub3(point, lp);
            float distance = mag3(to_point);
            if (distance >= l.end_distance) return false;
            if (distance < 0.1f) {
                out = mk3(l.color[0], l.color[1], l.color[2]);
                return true;
            }
            float datt = (distance <= l.start_distance) ? 1.0f : smoothstep_rs(l.end_distance, l.start_distance, distance);
            float area = l.width * l.height;
            f3 direction = norm3(to_point);
            float att;
            if (l.from_linedef) {
                att = datt * area * l.intensity;
            } else if (d2) {
                float dxn = fabsf(to_point.x / (l.width * 0.5f));
                float dyn = fabsf(to_point.y / (l.height * 0.5f));
                float ax = fmaxf(1.0f - dxn, 0.0f);
                float ay = fmaxf(1.0f - dyn, 0.0f);
                att = ax * ay * datt * l.intensity;
            } else {
                float aa = fmaxf(dot3(mk3(l.normal[0], l.normal[1], l.normal[2]), direction), 0.0f);
                att = aa * datt * area * l.intensity;
            }
            out = mk3(l.color[0] * att, l.color[1] * att, l.color[2] * att);
            return true;
        }
        default: {  // Daylight
            f3 to_point = sub3(point, lp);
            float distance = mag3(to_point);
            if (distance >= l.end_distance) return false;
            f3 direction = norm3(to_point);
            float aa = fmaxf(dot3(mk3(l.normal[0], l.normal[1], l.normal[2]), direction), 0.0f);
            float datt = (distance <= l.start_distance) ? 1.0f : smoothstep_rs(l.end_distance, l.start_distance, distance);
            float att = aa * datt * l.intensity;
            out = mk3(l.color[0] * att, l.color[1] * att, l.color[2] * att);
            return true;
        }
    }
}

// rasterizer.rs:1875-1951 with emissive == 0 at every call site
// (n_dot_l = max(dot(n, l), 0): the point-light path of the caller has the same float at hand as its Lambert term)
template <bool RL = false>
__device__ __forceinline__ f3 shade_fast_brdf(f3 base, float roughness, float metallic, f3 n, f3 v, f3 l, f3 radiance, float n_dot_l) {
    if (n_dot_l <= 0.0f) return mk3(0.0f, 0.0f, 0.0f);
    // Vec3::lerp(0.04, base, metallic) = mul_add(clamp01(t), b - a, a)
    float tm = rclamp(metallic, 0.0f, 1.0f);
    f3 f0 = mk3(fmaf(tm, base.x - 0.04f, 0.04f), fmaf(tm, base.y - 0.04f, 0.04f), fmaf(tm, base.z - 0.04f, 0.04f));
    f3 kd = scale3(base, 1.0f - metallic);
    kd = scale3(kd, 1.0f - fmaxf(f0.x, fmaxf(f0.y, f0.z)));
    float a = fmaxf(roughness * roughness, 1e-4f);
    float shininess = rclamp(2.0f / a - 2.0f, 1.0f, 2048.0f);
    f3 h;
    float n_dot_h, spec_b;
    if constexpr (RL) {
        float hm;
        h = norm3_relaxed(add3(l, v), hm);
        n_dot_h = fmaxf(dot3(n, h), 0.0f);
        // v_log_f32 / v_exp_f32 directly: where log2f / exp2f would rescale (a denormal n.h, a result below 2^-126) both forms give
        // a specular factor below 2^-126
        spec_b = (n_dot_h <= 0.0f) ? 0.0f : __builtin_amdgcn_exp2f(shininess * __builtin_amdgcn_logf(n_dot_h));
    } else {
        h = norm3_fast(add3(l, v));
        n_dot_h = fmaxf(dot3(n, h), 0.0f);
        spec_b = (n_dot_h <= 0.0f) ? 0.0f : rxm::pow_exp2_log2(n_dot_h, shininess);
    }
    float n_dot_v = fmaxf(dot3(n, v), 0.0f);
    float om = 1.0f - rclamp(n_dot_v, 0.0f, 1.0f);
    float x5 = om * om * om * om * om;
    f3 f = add3(f0, scale3(sub3(mk3(1.0f, 1.0f, 1.0f), f0), x5));
    f3 diffuse = scale3(kd, n_dot_l);
    f3 specular = scale3(scale3(f, spec_b), n_dot_l);
    return mul3(add3(diffuse, specular), radiance);  // + emissive (0)
}

// MapMini::get_occlusion / Chunk::get_occlusion (map/mini.rs:58-66, chunk.rs:154-161)
__device__ __forceinline__ float get_occlusion(const rxr_occluder *occ, uint32_t first, uint32_t count, float x, float y) {
    for (uint32_t i = 0; i < count; ++i) {
        const rxr_occluder &o = occ[first + i];
        if (x >= o.min[0] && x <= o.max[0] && y >= o.min[1] && y <= o.max[1]) return o.occlusion;
    }
    return 1.0f;
}

// MapMini::is_visible (map/mini.rs:68-95)
__device__ __forceinline__ bool mapmini_is_visible(const rxr_linedef *ld, uint32_t n, float ax, float ay, float bx, float by) {
    for (uint32_t i = 0; i < n; ++i) {
        const rxr_linedef seg = uniform_record(ld, i);
        float b1x = seg.start[0], b1y = seg.start[1], b2x = seg.end[0], b2y = seg.end[1];
        float d = (bx - ax) * (b2y - b1y) - (by - ay) * (b2x - b1x);
        if (d == 0.0f) continue;
        float u = ((b1x - ax) * (b2y - b1y) - (b1y - ay) * (b2x - b1x)) / d;
        float v = ((b1x - ax) * (by - ay) - (b1y - ay) * (bx - ax)) / d;
        if ((u >= 0.0f && u <= 1.0f) && (v >= 0.0f && v <= 1.0f)) return false;
    }
    return true;
}

__device__ __forceinline__ uint32_t pack4(uint32_t r, uint32_t g, uint32_t b, uint32_t a) {
    return r | (g << 8) | (b << 16) | (a << 24);
}

// GridShader::shade_pixel (shader/grid.rs:36-108) at pixel (px, py): uv = (x / W, y / H), screen = (W, H) as the tile loop
// passes them (rasterizer.rs:292-308).  vek's Vec2 arithmetic is component-wise; `round` is half away from zero, `min` drops NaN.
__device__ __forceinline__ float grid_mul_dist(float delta, float value) {  // |value - delta * round(value / delta)|
    return fabsf(value - delta * roundf(value / delta));
}
__device__ __forceinline__ uint32_t grid_shade(const RasterParams &P, uint32_t px, uint32_t py) {
    const float grid = P.bg_grid[0], sub_div = P.bg_grid[1];
    const float pos_x = ((float)px / P.fwidth) * P.fwidth, pos_y = ((float)py / P.fheight) * P.fheight;
    const float origin_x = P.fwidth / 2.0f + P.bg_grid[2], origin_y = P.fheight / 2.0f + P.bg_grid[3];
    // align_pixel(origin, 1): odd thickness
    const float ao_x = roundf(origin_x - 0.5f) + 0.5f, ao_y = roundf(origin_y - 0.5f) + 0.5f;
    const float rel_x = pos_x - ao_x, rel_y = pos_y - ao_y;
    const float dist_x = grid_mul_dist(grid, rel_x), dist_y = grid_mul_dist(grid, rel_y);
    const uint32_t line = pack4(f32_to_u8_saturated(0.15f), f32_to_u8_saturated(0.15f), f32_to_u8_saturated(0.15f), f32_to_u8_saturated(1.0f));
    const uint32_t sub_line = pack4(f32_to_u8_saturated(0.11f), f32_to_u8_saturated(0.11f), f32_to_u8_saturated(0.11f), f32_to_u8_saturated(1.0f));
    const uint32_t bg = pack4(f32_to_u8_saturated(0.05f), f32_to_u8_saturated(0.05f), f32_to_u8_saturated(0.05f), f32_to_u8_saturated(1.0f));
    if (fminf(dist_x, dist_y) <= 1.0f * 0.5f) return line;
    const float dtf_x = fabsf(rel_x - grid * floorf(rel_x / grid)), dtf_y = fabsf(rel_y - grid * floorf(rel_y / grid));
    const float sub_size = grid / roundf(sub_div);
    float sd_x = grid_mul_dist(sub_size, dtf_x), sd_y = grid_mul_dist(sub_size, dtf_y);
    const float rc_x = roundf(dist_x / sub_size), rc_y = roundf(dist_y / sub_size);
    const float extra = grid - sub_size * sub_div;
    if (rc_x == sub_div) sd_x = sd_x + extra;
    if (rc_y == sub_div) sd_y = sd_y + extra;
    if (fminf(sd_x, sd_y) <= 1.0f * 0.5f) return sub_line;
    return bg;
}

// perspective-correct uv of the fragment (rasterizer.rs:1062-1076)
__device__ __forceinline__ void fragment_uv(const TriShade &S, float alpha, float beta, float gamma, float &u, float &v) {
    float iu = S.u0w * alpha + S.u1w * beta + S.u2w * gamma;
    float iv = S.v0w * alpha + S.v1w * beta + S.v2w * gamma;
    float irw = S.iw0 * alpha + S.iw1 * beta + S.iw2 * gamma;
    rxm::div2(iu, iv, irw, u, v);
}

// texel base of a texture: the resident pool, or this frame's chunk textures in the frame blob
__device__ __forceinline__ const uint32_t *texel_base(const RasterParams &P, const DevTexDesc &d) {
    // both bases as scalars, then a select: written as `c ? P.frame_texels : P.texels` the compiler selects between the two ADDRESSES
    // inside the parameter block and loads the pointer per lane -- one more dependent round trip in front of every texel
    // (as integers, and back through the global address space: a pointer that has been through the asm is a FLAT pointer to the
    // compiler, and flat loads count against the LDS counter as well)
    unsigned long long ft = (unsigned long long)P.frame_texels, rt = (unsigned long long)P.texels;
    asm volatile("" : "+v"(ft), "+v"(rt));  // ("v": the out-of-line interpreter sites receive P through vector registers)
    typedef const uint32_t __attribute__((address_space(1))) *global_words;
    return (const uint32_t *)(global_words)((d.all_opaque & 2u) ? ft : rt);
}

// Chunk::sample_terrain_texture(world_pos, Vec2::one()) (chunk.rs:133-151) with Texture::get_pixel (texture.rs:527-538)
__device__ __forceinline__ uint32_t terrain_texel(const RasterParams &P, const DevBatch &B, float wx, float wy) {
    const ChunkRange cr = P.chunks[B.chunk];
    const DevTexDesc d = P.tex[B.tex];
    float local_x = (wx / 1.0f) - (float)cr.origin_x;
    float local_y = (wy / 1.0f) - (float)cr.origin_y;
    float pixel_x = local_x * (float)cr.pixels_per_tile;
    float pixel_y = local_y * (float)cr.pixels_per_tile;
    uint32_t px = sat_u32(rclamp(floorf(pixel_x), 0.0f, (float)d.w - 1.0f));
    uint32_t py = sat_u32(rclamp(floorf(pixel_y), 0.0f, (float)d.h - 1.0f));
    px = min(px, d.w - 1u);
    py = min(py, d.h - 1u);
    return texel_base(P, d)[d.offset + py * d.w + px];
}

// Rasterizer.brush_preview over a terrain texel (rasterizer.rs:1193-1212, :1601-1622): a white disc around the brush position,
// 20 % .. 80 % opaque, blended into RGB with `as u8` truncation; `world` is the fragment's world position
__device__ __forceinline__ float brush_blend(const RasterParams &P, f3 world, bool &inside) {
    const float dist = mag3(sub3(world, mk3(P.brush_pos[0], P.brush_pos[1], P.brush_pos[2])));
    inside = dist < P.brush_radius;
    const float normalized = dist / P.brush_radius;
    const float falloff = rclamp(P.brush_falloff, 0.001f, 1.0f);
    const float fade = rclamp((1.0f - normalized) / falloff, 0.0f, 1.0f);
    return 0.2f + 0.6f * fade;
}
__device__ __forceinline__ uint32_t brush_over_texel(const RasterParams &P, uint32_t texel, f3 world) {
    bool inside;
    const float blend = brush_blend(P, world, inside);
    if (!inside) return texel;
    uint32_t out = texel & 0xFF000000u;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float c = (float)((texel >> (8 * i)) & 0xFFu);
        out |= sat_u8(fminf(c * (1.0f - blend) + 255.0f * blend, 255.0f)) << (8 * i);
    }
    return out;
}

// what the feature level LV of the raster code below carries (the table of rxr_device.h)
template <Level LV> inline constexpr LevelFeatures feat = level_features(LV);

// the texel switch of the raster loops (rasterizer.rs:1101-1222, :672-758); (wx, wy) is the position terrain batches sample at;
// `world3`: the fragment's world position in the two 3D loops (terrain brush preview), nullptr in the 2D loop
// UNIFORM: `B` is the same batch for every lane (the 2D pass walks one primitive at a time) -- its texture descriptor then
// comes through the scalar cache like the batch header itself (uniform_record)
template <Level LV, bool UNIFORM = false>
__device__ __forceinline__ uint32_t batch_texel(const RasterParams &P, const DevBatch &B, float u, float v, float wx, float wy, const f3 *world3 = nullptr) {
    if constexpr (!UNIFORM && !feat<LV>.chunk) {
        // tex, pixel and repeat_mode are neighbours in the header: one 16-byte load instead of one word now and another, behind
        // the descriptor's round trip, when the sampler wants the repeat mode
        static_assert(__builtin_offsetof(DevBatch, tex) == 16 && __builtin_offsetof(DevBatch, pixel) == 20 && __builtin_offsetof(DevBatch, repeat_mode) == 24, "one 16-byte load");
        const uint4 hw = *reinterpret_cast<const uint4 *>(&B.tex);
        int32_t tex = (int32_t)hw.x;
        uint32_t pixel = hw.y, repeat = hw.z;
        asm volatile("" : "+v"(tex), "+v"(pixel), "+v"(repeat));
        if (tex < 0) return pixel;
        const uint4 raw = *reinterpret_cast<const uint4 *>(&P.tex[tex]);
        DevTexDesc d{raw.x, raw.y, raw.z, raw.w};
        asm volatile("" : "+v"(d.offset), "+v"(d.w), "+v"(d.h), "+v"(d.all_opaque));
        return sample_texture(d, texel_base(P, d), u, v, P.sample_mode, repeat);
    }
    if (B.tex < 0) return B.pixel;
    if constexpr (feat<LV>.chunk) {
        if (B.flags & DB_TERRAIN) {
            uint32_t t = terrain_texel(P, B, wx, wy);
            if (P.has_brush && world3) t = brush_over_texel(P, t, *world3);
            return t;
        }
    }
    if constexpr (UNIFORM) {
        const DevTexDesc d = uniform_record(P.tex, (uint32_t)B.tex);
        return sample_texture(d, texel_base(P, d), u, v, P.sample_mode, B.repeat_mode);
    } else {
        // the descriptor in ONE 16-byte load: left to itself the compiler fetches its four words where they are first used --
        // all_opaque, then w, then h and offset, three dependent round trips between the batch header and the texel
        const uint4 raw = *reinterpret_cast<const uint4 *>(&P.tex[B.tex]);
        DevTexDesc d{raw.x, raw.y, raw.z, raw.w};
        asm volatile("" : "+v"(d.offset), "+v"(d.w), "+v"(d.h), "+v"(d.all_opaque));
        static_assert(sizeof(DevTexDesc) == 16, "one 16-byte load");
        return sample_texture(d, texel_base(P, d), u, v, P.sample_mode, B.repeat_mode);
    }
}

// ---- the covered-fragment block of d3_rasterize after the depth test (rasterizer.rs:1062-1404) ----
// Split in three so that the light loop runs in wave-uniform control flow (see shade3d_lights).
struct Frag {
    f3 world, normal, view_dir, base, lit;
    float opacity;
    uint32_t alpha_bits;  // the texel's alpha byte where it stands (bits 24..31): at levels without chunk paths and programs it IS the encoded
                          // alpha -- trunc(fma(clamp(RN(a / 255), 0, 1), 255, 0.5)) = a for every byte a -- and `opacity` is never formed
    float rough, metal;  // mat_roughness / mat_metallic (:1321-1322): 0.5 / 0 unless a program ran
    f3 emis;             // mat_emissive (:1323): what THIS fragment's program assigned (levels with programs; frames in which a
                         // fragment could see another fragment's emissive are refused by rxr_upload_frame), else 0
};

// screen_to_world (rasterizer.rs:1707-1727) in the reference's own sequence: two quotients, the inverse projection, the perspective
// divide, the inverse view.  fx, fy are pixel centres (0.5 .. 2^15) and the frame size is validated by rxr_upload_frame
// (1 .. 32768): always inside the division window
__device__ __forceinline__ f3 screen_to_world_exact(const RasterParams &P, float fx, float fy, float z) {
    float vx, vy, vz, vw, wx, wy, wz, ww;
    const float x_ndc = 2.0f * rxm::div1_known(fx, P.fwidth, true) - 1.0f;
    const float y_ndc = 1.0f - 2.0f * rxm::div1_known(fy, P.fheight, true);
    mat4_mul(P.inv_proj, x_ndc, y_ndc, z, 1.0f, vx, vy, vz, vw);
    rxm::div3_self(vx, vy, vz, vw, vx, vy, vz, vw);
    mat4_mul(P.inv_view, vx, vy, vz, vw, wx, wy, wz, ww);
    return mk3(wx, wy, wz);
}

// everything before the light loop: uv, world position, normal, texel, ambient terms (:1062-1370)
// RL (relaxed light mode, frames with a 3D light loop only): the view direction and the surface normal feed nothing but the lit
// colour, so they are normalised with one v_rsq_f32 each (within 2 ulp per component) and the reference's second normalisation of
// the already-unit normal (:1320) is skipped.  The one DECISION they take part in -- flip the normal toward the camera when
// n.v < 0 (:1096) -- is only taken from the relaxed values when every fragment of the wave has |n.v| >= 1e-4, a hundred times
// their error; otherwise, and for magnitudes outside the window, the wave takes the exact sequences.
template <Level LV, bool RL = false>
__device__ __forceinline__ void shade3d_begin(const RasterParams &P, const TriShade &S, uint32_t batch_id, float alpha, float beta,
                                              float z, float fx, float fy, Frag &F, bool have_flags = false, uint32_t known_flags = 0u) {
    const DevBatch &B = P.batches3d[batch_id];
    // (have_flags, wave-uniform: the caller read the flags from the winner's staged record -- no round trip to the header for them)
    const uint32_t b_flags = have_flags ? known_flags : B.flags;
    float gamma = 1.0f - alpha - beta;
    float u, v;
    fragment_uv(S, alpha, beta, gamma, u, v);

    // screen_to_world (rasterizer.rs:1707-1727).  Relaxed mode, neither chunk paths nor programs, no occluder anywhere: the world position feeds only
    // the light loop and the view direction -- continuous uses -- so its three divisions (pixel / frame size, the perspective divide) become
    // products: with 2 / width and -2 / height as the host rounded them (no reciprocal of a wave-uniform operand here) and with v_rcp_f32 of
    // w (within 2 ulp).  The two matrix products keep the reference's own operation order: w is a difference of two nearly equal
    // terms, and only the same roundings in the same order land on the reference's value (one product with a combined matrix, its
    // constant column innermost, left 21 831 pixels of the 4K bench frame a step off where this leaves about a hundred).  With an occluder
    // in the frame its boxes are compared with the position (get_occlusion): the exact quotients then, as for a w outside the window.
    bool relaxed_world = RL && !feat<LV>.chunk && !feat<LV>.programs && !P.any_occluders;  // wave-uniform
    f3 world;
    if (relaxed_world) {
        float vx, vy, vz, vw, wx, wy, wz, ww;
        mat4_mul(P.inv_proj, fmaf(fx, P.ndc_sx, -1.0f), fmaf(fy, P.ndc_sy, 1.0f), z, 1.0f, vx, vy, vz, vw);
        relaxed_world = rxm::wave_all(rxm::in_window(vw));
        if (relaxed_world) {
            const float rw = __builtin_amdgcn_rcpf(vw);
            mat4_mul(P.inv_view, vx * rw, vy * rw, vz * rw, 1.0f, wx, wy, wz, ww);
            world = mk3(wx, wy, wz);
        }
    }
    if (!relaxed_world) world = screen_to_world_exact(P, fx, fy, z);
    f3 cam = mk3(P.cam[0], P.cam[1], P.cam[2]);
    f3 view_dir, normal;
    bool relaxed_normals = false;  // wave-uniform
    if constexpr (RL && !feat<LV>.programs) {
        const bool has_n = (b_flags & DB_HAS_NORMALS) != 0u;
        const f3 vd = sub3(cam, world);
        f3 ni = mk3(0.0f, 0.0f, 0.0f);
        if (has_n) {
            f3 n0 = mk3(S.n0[0], S.n0[1], S.n0[2]), n1 = mk3(S.n1[0], S.n1[1], S.n1[2]), n2 = mk3(S.n2[0], S.n2[1], S.n2[2]);
            ni = add3(add3(scale3(n0, alpha), scale3(n1, beta)), scale3(n2, gamma));
        }
        const float vm2 = fmaf(vd.z, vd.z, fmaf(vd.y, vd.y, vd.x * vd.x)), nm2 = fmaf(ni.z, ni.z, fmaf(ni.y, ni.y, ni.x * ni.x));
        const float vinv = __builtin_amdgcn_rsqf(vm2), ninv = __builtin_amdgcn_rsqf(nm2);
        const float dnv = fmaf(ni.z, vd.z, fmaf(ni.y, vd.y, ni.x * vd.x)) * (vinv * ninv);
        // with the relaxed world position the view vector itself is off by up to an ulp of |world| -- an angle of ulp * |world| / |v|,
        // which matters for a camera far from the origin looking at something close: the guard grows with that ratio (25x margin)
        float guard = P.rl_flip_guard;
        if (relaxed_world) guard = fmaf(1e-5f * vinv, __builtin_fabsf(world.x) + __builtin_fabsf(world.y) + __builtin_fabsf(world.z), guard);
        relaxed_normals = rxm::wave_all(rxm::sq_in_window(vm2) && (!has_n || (rxm::sq_in_window(nm2) && __builtin_fabsf(dnv) >= guard)));
        if (relaxed_normals) {
            view_dir = scale3(vd, vinv);
            // (no normals: the reference normalises the zero vector, 0 / 0)
            normal = has_n ? scale3(ni, dnv < 0.0f ? -ninv : ninv) : mk3(__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""));
        }
    }
    if (!relaxed_normals) {
        if (relaxed_world) world = screen_to_world_exact(P, fx, fy, z);  // (rare: the exact sequences want the reference's world position)
        view_dir = norm3_fast(sub3(cam, world));
        if (b_flags & DB_HAS_NORMALS) {  // :1083-1099
            f3 n0 = mk3(S.n0[0], S.n0[1], S.n0[2]), n1 = mk3(S.n1[0], S.n1[1], S.n1[2]), n2 = mk3(S.n2[0], S.n2[1], S.n2[2]);
            normal = norm3_z(add3(add3(scale3(n0, alpha), scale3(n1, beta)), scale3(n2, gamma)));
            if (dot3(normal, view_dir) < 0.0f) normal = neg3(normal);
        } else {
            normal = mk3(0.0f, 0.0f, 0.0f);
        }
    }

    uint32_t texel;
    bool desc_in_record = false;  // wave-uniform
    if constexpr (!feat<LV>.chunk || !feat<LV>.programs) desc_in_record = rxm::wave_all((S.pad[1] & TS_DESC_VALID) != 0u);  // (terrain batches leave the words zero: make_setup)
    if (desc_in_record) {  // (make_setup: the descriptor as the record carries it -- the same sampler on the same words)
        const uint32_t p0 = S.pad[0], p1 = S.pad[1];
        const DevTexDesc d{p0, p1 & 0x1FFFu, (p1 >> 13) & 0x1FFFu, (p1 >> 28) & 3u};
        texel = sample_texture(d, texel_base(P, d), u, v, P.sample_mode, (p1 >> 26) & 3u);
    } else texel = batch_texel<LV>(P, B, u, v, world.x, world.z, &world);
    const float INV_255 = 1.0f / 255.0f;  // lib.rs:52
    f3 base = mk3(srgb_to_linear_fast((float)(texel & 0xFFu) * INV_255), srgb_to_linear_fast((float)((texel >> 8) & 0xFFu) * INV_255),
                  srgb_to_linear_fast((float)((texel >> 16) & 0xFFu) * INV_255));
    F.opacity = rxm::div1_known((float)(texel >> 24), 255.0f, true);  // :1313; byte / 255 is inside the division window
    F.alpha_bits = texel & 0xFF000000u;  // (shade3d_end, levels without chunk paths and programs: nothing else reads or writes the opacity there)
    if (feat<LV>.chunk && B.baked_plus1) {  // chunk.shader_textures: the baked texel replaces colour and alpha, no program runs (:1239-1267)
        const DevTexDesc &baked = P.tex[B.baked_plus1 - 1u];
        uint32_t bt = sample_texture(baked, texel_base(P, baked), u, v, P.sample_mode, B.repeat_mode);
        base = mk3(srgb_to_linear_fast((float)(bt & 0xFFu) * INV_255), srgb_to_linear_fast((float)((bt >> 8) & 0xFFu) * INV_255),
                   srgb_to_linear_fast((float)((bt >> 16) & 0xFFu) * INV_255));
        F.opacity = (float)(bt >> 24) * INV_255;  // execution.opacity.x = color.w of pixel_to_vec4 (:1262)
    }
    float rough = 0.5f, metal = 0.0f;  // :1315-1316 (no-shader branch)
    if constexpr (feat<LV>.programs) {
        if (B.program_plus1) {  // :1283-1304
            rxvm::IO io;
            rxvm::io_defaults(io);
            io.color = rxvm::mk(base.x, base.y, base.z);
            io.opacity.x = F.opacity;
            io.normal = rxvm::mk(normal.x, normal.y, normal.z);
            io.roughness.x = 0.5f;
            io.metallic.x = 0.0f;
            io.uv.x = u / 4.0f;
            io.uv.y = v / 4.0f;
            io.hitpoint = rxvm::mk(world.x, world.y, world.z);
            io.time = rxvm::splat(P.time);
            // (calling the out-of-line interpreter from the opaque pass too was slower: 304 vs 236 us on the probe)
            if constexpr (feat<LV>.inline_site) rxvm::shade_inline<feat<LV>.ssp>(P, B.program_plus1 - 1u, io, rxvm::stack_block());
            else rxvm::shade_call<feat<LV>.ssp>(P, B.program_plus1 - 1u, io);  // VmOol / VmSOol: from the visibility loop's alpha test
            base = mk3(io.color.x, io.color.y, io.color.z);  // :1319-1323
            normal = mk3(io.normal.x, io.normal.y, io.normal.z);
            rough = rclamp(io.roughness.x, 0.0f, 1.0f);
            metal = rclamp(io.metallic.x, 0.0f, 1.0f);
            F.opacity = io.opacity.x;  // :1403
            F.emis = mk3(io.emissive.x, io.emissive.y, io.emissive.z);  // :1323
        }
    }

    if (!relaxed_normals) normal = norm3_z(normal);  // :1320

    f3 lit = mk3(0.0f, 0.0f, 0.0f);
    float occlusion;
    // the batch's ambient colour and its chunk are neighbours in the header: one 16-byte load here instead of the chunk now and the
    // colour in a round trip of its own at the end of this function, right in front of the light loop
    static_assert(__builtin_offsetof(DevBatch, ambient) == 32 && __builtin_offsetof(DevBatch, chunk) == 44, "one 16-byte load");
    const uint4 amb_chunk = *reinterpret_cast<const uint4 *>(&B.ambient[0]);
    float amb0 = __uint_as_float(amb_chunk.x), amb1 = __uint_as_float(amb_chunk.y), amb2 = __uint_as_float(amb_chunk.z);
    int32_t b_chunk = (int32_t)amb_chunk.w;
    asm volatile("" : "+v"(amb0), "+v"(amb1), "+v"(amb2), "+v"(b_chunk));
    if (b_chunk >= 0) {
        ChunkRange cr = P.chunks[b_chunk];
        occlusion = get_occlusion(P.occluders, cr.occ_first, cr.occ_count, world.x, world.z);
    } else {
        occlusion = get_occlusion(P.occluders, 0, P.n_occluders, world.x, world.z);
    }
    float hemi = 0.5f * (normal.y + 1.0f);
    f3 kd = scale3(scale3(base, 1.0f - metal), 1.0f - 0.04f);
    if (occlusion > 0.0f) {  // :1334-1365
        if (P.flags & RXR_FLAG_HAS_AMBIENT) {
            lit = add3(lit, scale3(mul3(mk3(P.ambient[0], P.ambient[1], P.ambient[2]), kd), hemi));
        }
        if ((P.flags & RXR_FLAG_HAS_SUN) && P.day_factor > 0.0f) {
            f3 ldir = norm3(neg3(mk3(P.sun_dir[0], P.sun_dir[1], P.sun_dir[2])));
            float df = fmaxf(P.day_factor, 0.0f);
            lit = add3(lit, shade_fast_brdf(base, rough, metal, normal, view_dir, ldir, mk3(df, df, df), fmaxf(dot3(normal, ldir), 0.0f)));
        }
        lit = scale3(lit, occlusion);
    }
    lit = add3(lit, scale3(mul3(mk3(amb0, amb1, amb2), kd), hemi));  // :1368-1370
    F.world = world;
    F.normal = normal;
    F.view_dir = view_dir;
    F.base = base;
    F.lit = lit;
    F.rough = rough;
    F.metal = metal;
}

// The direct-light loop (:1373-1391).  Must be called by EVERY lane of the wave (`hit` marks the lanes
// that own a fragment).  Lights are first culled per WAVE, one light per lane: a light whose range
// sphere cannot reach the bounding sphere of the wave's fragments is one for which every lane's
// `distance >= end_distance` test (light.rs:539, 561, 586, 636) would return None, so skipping it
// changes nothing; the surviving lights are then evaluated in their original order.
// RL: the relaxed arithmetic of RXR_LIGHT_MATH=relaxed for POINT lights (every quantity is continuous in the fragment's position
// there: the range test, the smoothstep and the Lambert / specular cut-offs all meet their neighbours at zero, so an error of a
// few ulp moves a channel by at most one step); spot, area and daylight lights have hard cut-offs and stay exact in both modes.
// Three A-B variants of the relaxed point-light term were tried against what stands below and are retired: the light's
// constants read from its rxr_light record in the loop (now its LightFast record), the light direction formed and normalised
// first (now folded into the dot products), and exp2(6 log2 x) at levels without programs (now three multiplies).
// PREFIX: relaxed kernels walk the leading fast lights in a loop of their own (below; not k_raster_pair_rl and the *_cut_rl kernels,
// which sit at their 64 registers with scratch already and answered with 16 and 8 more bytes of it).
template <Level LV, bool RL = false, bool PREFIX = RL>
__device__ __forceinline__ void shade3d_lights(const RasterParams &P, bool hit, Frag &F) {
    static_assert(RL || !PREFIX, "the prefix loop is the relaxed term");
    const unsigned long long hitmask = __ballot(hit);
    if (hitmask == 0ull) return;
    const int lane = (int)(threadIdx.x & 63u);
    const int src = __ffsll((long long)hitmask) - 1;
    // (the centre through v_readlane_b32 -- `src` is a scalar -- and the radius through DPP operands: no LDS round trip in front of the loop)
    const f3 c = mk3(__int_as_float(__builtin_amdgcn_readlane(__float_as_int(F.world.x), src)),
                     __int_as_float(__builtin_amdgcn_readlane(__float_as_int(F.world.y), src)),
                     __int_as_float(__builtin_amdgcn_readlane(__float_as_int(F.world.z), src)));
    const float r = hit ? mag3_bound(sub3(F.world, c)) : 0.0f;
    // NaN / inf world positions are not bounded by the sphere: no culling for this wave then
    const bool can_cull = __ballot(hit && !(r < __builtin_huge_valf())) == 0ull;  // (INFINITY, without <cmath>: hiprtc)
    const float rmax = rxm::wave_max_nonneg(r);  // (a magnitude, +0 for the lanes without a fragment; meaningless and unused when !can_cull)
    const float rough = feat<LV>.programs ? F.rough : 0.5f, metal = feat<LV>.programs ? F.metal : 0.0f;
    // relaxed mode: the light-independent factors of shade_fast_brdf (:1875-1951) once per fragment -- diffuse weight kd, Fresnel
    // term f, shininess -- by the reference's own operations
    f3 rl_kd = mk3(0.0f, 0.0f, 0.0f), rl_f = rl_kd;
    float rl_shininess = 1.0f;
    if constexpr (RL && !feat<LV>.programs) {
        // levels without programs: metal = 0 and the base colour is a texel's (finite), so f0 = lerp(0.04, base, 0) is 0.04
        // in every channel -- the same floats as the general form below without its multiplications by zero
        rl_kd = scale3(F.base, 1.0f - 0.04f);
        rl_shininess = 6.0f;  // clamp(2 / 0.25 - 2, 1, 2048)
        const float om = 1.0f - rclamp(fmaxf(dot3(F.normal, F.view_dir), 0.0f), 0.0f, 1.0f);
        const float fs = 0.04f + (1.0f - 0.04f) * (om * om * om * om * om);
        rl_f = mk3(fs, fs, fs);
    } else if constexpr (RL) {
        const float tm = rclamp(metal, 0.0f, 1.0f);
        const f3 f0 = mk3(fmaf(tm, F.base.x - 0.04f, 0.04f), fmaf(tm, F.base.y - 0.04f, 0.04f), fmaf(tm, F.base.z - 0.04f, 0.04f));
        rl_kd = scale3(scale3(F.base, 1.0f - metal), 1.0f - fmaxf(f0.x, fmaxf(f0.y, f0.z)));
        rl_shininess = rclamp(2.0f / fmaxf(rough * rough, 1e-4f) - 2.0f, 1.0f, 2048.0f);
        const float om = 1.0f - rclamp(fmaxf(dot3(F.normal, F.view_dir), 0.0f), 0.0f, 1.0f);
        rl_f = add3(f0, scale3(sub3(mk3(1.0f, 1.0f, 1.0f), f0), om * om * om * om * om));
    }

    for (uint32_t base_i = 0; base_i < P.n_lights; base_i += 64u) {
        const uint32_t mine = base_i + (uint32_t)lane;
        bool cand = mine < P.n_lights;
        // smoothstep(end, start, d) divides by (start - end), the same for every fragment: the lane that owns the light in
        // this step keeps the denominator's refined reciprocal (rxr_exact_math.h) and whether it is inside the window
        float ss_rcp = 0.0f;
        bool ss_ok = false;
        unsigned long long ss_ok_mask = 0ull;
        // lights of this step that have a LightFast record (relaxed mode): one bit per light, tested by the scalar unit in the loop
        unsigned long long fast_mask = 0ull;
        if constexpr (RL) {
            // Everything the step needs of a light -- position, range, whether its type is culled at all, whether it has a fast
            // record -- comes from its LightFast record in ONE round of loads (the general form below reads start / end, the fast flag,
            // the type and then position / range in four dependent round trips, each behind the previous one's branch); the
            // smoothstep's reciprocal is only wanted by lights WITHOUT a fast record, a uniform branch no lit room takes.
            bool fast = false;
            if (cand) {
                // (two 16-byte loads, each feeding a word that is needed whatever the light is: issued together, one round trip)
                const float4 *lf4 = reinterpret_cast<const float4 *>(&P.lights_fast[mine]);
                const float4 head = lf4[0], tail = lf4[2];
                f3 lpos = mk3(head.x, head.y, head.z);
                float endd = tail.x;
                asm volatile("" : "+v"(lpos.x), "+v"(lpos.y), "+v"(lpos.z), "+v"(endd));  // (keeps the compiler from sinking the loads' other halves behind the branch below)
                const uint32_t kind = __float_as_uint(tail.y);
                fast = __float_as_uint(head.w) != 0u;
                if (can_cull && kind) {
                    float dcl = mag3_bound(sub3(c, lpos));
                    // every fragment p of the wave has |p - L| >= dcl - rmax; the margin covers rounding
                    float margin = 1e-3f * (dcl + rmax + fabsf(endd)) + 1e-6f;
                    if (dcl - rmax > endd + margin) cand = false;
                }
            }
            fast_mask = __ballot(cand && fast);
            if (__ballot(cand && !fast)) {
                if (cand && !fast) {
                    const float ssd = P.lights[mine].start_distance - P.lights[mine].end_distance;
                    ss_ok = rxm::in_window(ssd);
                    ss_rcp = rxm::rcp_refined(ssd);
                }
                ss_ok_mask = __ballot(ss_ok);
            }
        } else {
            if (cand) {
                const float ssd = P.lights[mine].start_distance - P.lights[mine].end_distance;
                ss_ok = rxm::in_window(ssd);
                ss_rcp = rxm::rcp_refined(ssd);
            }
            ss_ok_mask = __ballot(ss_ok);
            if (cand && can_cull) {
                const rxr_light &L = P.lights[mine];
                if (L.light_type == RXR_LIGHT_POINT || L.light_type == RXR_LIGHT_SPOT || L.light_type == RXR_LIGHT_AREA ||
                    L.light_type == RXR_LIGHT_DAYLIGHT) {
                    float dcl = mag3_bound(sub3(c, mk3(L.position[0], L.position[1], L.position[2])));
                    // every fragment p of the wave has |p - L| >= dcl - rmax; the margin covers rounding
                    float margin = 1e-3f * (dcl + rmax + fabsf(L.end_distance)) + 1e-6f;
                    if (dcl - rmax > L.end_distance + margin) cand = false;
                }
            }
        }
        unsigned long long todo = __ballot(cand);
        if constexpr (PREFIX) {
            // The leading run of lights with a LightFast record in a loop of its own, whose body is the fast term of the loop below and
            // nothing else (the same operations in the same order, so the same floats).  What the loop below pays around that term per
            // light and wave is paid here once per step: the table's base stays in SGPRs instead of being re-read from the kernarg
            // segment in front of every record (one scalar round trip per light, not two dependent ones); exec is never narrowed to
            // `hit`; and with no second path to join, F.lit is updated in place (no copies at the latch): 44 VALU instructions
            // per light and wave against 47, no s_and_saveexec.  Every lane takes part: a wave-uniform `todo` cannot come out of a
            // region entered under `hit` as a scalar, so a lane without a fragment computes a term nobody reads (its F is zeros,
            // its colour the miss colour) and only the window test is masked with `hitmask`.
            // The run ends at the first light without a record or whose squared distance leaves the window for a fragment: that
            // light is still in `todo`, and it and everything behind it go through the loop below, unchanged.
            // RXR_LIGHT_PREFIX=0 (RPF_LIGHT_PREFIX clear) leaves every light to the loop below: the parent's frame by the parent's code.
            // Tried on top and dropped (profiles/light_prefix/): the next light's record fetched under this light's arithmetic --
            // the bench frame 1.4 us SLOWER than without (eight more live SGPRs, five s_mov and a select per light).
            const unsigned long long slow = todo & ~fast_mask;
            unsigned long long pre = slow ? (todo & ((slow & (0ull - slow)) - 1ull)) : todo;
            if (!(P.flags & RPF_LIGHT_PREFIX)) pre = 0ull;
            if (pre) {
                const LightFast *tbl = P.lights_fast + base_i;
                LightFast LF = uniform_record_x8(tbl, (uint32_t)(__ffsll((long long)pre) - 1));
                for (;;) {
                    // (the record stays in the scalar registers it was loaded into: the arithmetic reads it from there, as the loop below does)
                    asm volatile("" : "+s"(LF.pos[0]), "+s"(LF.pos[1]), "+s"(LF.pos[2]), "+s"(LF.ss_r), "+s"(LF.cfi[0]), "+s"(LF.cfi[1]), "+s"(LF.cfi[2]), "+s"(LF.c0));
                    pre &= pre - 1ull;
                    const f3 d = sub3(mk3(LF.pos[0], LF.pos[1], LF.pos[2]), F.world);
                    const float m2 = fmaf(d.z, d.z, fmaf(d.y, d.y, d.x * d.x));
                    if (__ballot(!rxm::sq_in_window(m2)) & hitmask) break;  // (wave_all over the lanes that own a fragment)
                    const float inv = __builtin_amdgcn_rsqf(m2);
                    const float t = __builtin_amdgcn_fmed3f(fmaf(m2 * inv, LF.ss_r, LF.c0), 0.0f, 1.0f);
                    const float ss = t * t * fmaf(-2.0f, t, 3.0f);
                    const float ndl = __builtin_amdgcn_fmed3f(fmaf(F.normal.z, d.z, fmaf(F.normal.y, d.y, F.normal.x * d.x)) * inv, 0.0f, 1.0f);
                    const f3 hu = mk3(fmaf(d.x, inv, F.view_dir.x), fmaf(d.y, inv, F.view_dir.y), fmaf(d.z, inv, F.view_dir.z));
                    const float hh = fmaf(hu.z, hu.z, fmaf(hu.y, hu.y, hu.x * hu.x));
                    const float ndh = __builtin_amdgcn_fmed3f(fmaf(F.normal.z, hu.z, fmaf(F.normal.y, hu.y, F.normal.x * hu.x)) * __builtin_amdgcn_rsqf(hh), 0.0f, 1.0f);
                    float spec;
                    if constexpr (!feat<LV>.programs) {
                        const float ndh2 = ndh * ndh;
                        spec = ndh2 * ndh2 * ndh2;
                    } else {
                        spec = __builtin_amdgcn_exp2f(rl_shininess * __builtin_amdgcn_logf(ndh));
                    }
                    const float s = ss * ndl * ndl;
                    F.lit.x = fmaf(fmaf(rl_f.x, spec, rl_kd.x), LF.cfi[0] * s, F.lit.x);
                    F.lit.y = fmaf(fmaf(rl_f.y, spec, rl_kd.y), LF.cfi[1] * s, F.lit.y);
                    F.lit.z = fmaf(fmaf(rl_f.z, spec, rl_kd.z), LF.cfi[2] * s, F.lit.z);
                    todo &= todo - 1ull;  // (this light was the lowest of `todo`)
                    if (!pre) break;
                    LF = uniform_record_x8(tbl, (uint32_t)(__ffsll((long long)pre) - 1));
                }
            }
        }
        while (todo) {
            const int li_lane = __ffsll((long long)todo) - 1;
            const uint32_t li = base_i + (uint32_t)li_lane;
            todo &= todo - 1ull;
            // (read where the exact kernels have always read it; the relaxed kernels want it only behind their fast path)
            float ss_r = 0.0f;
            bool ss_fast = false;
            if constexpr (!RL) {
                ss_r = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ss_rcp), li_lane));
                ss_fast = (ss_ok_mask >> li_lane) & 1ull;
            }
            if (!hit) continue;
            if constexpr (RL) {
                // The whole point-light term in relaxed arithmetic: fused multiply-adds, one v_rsq_f32 per normalisation, the half
                // vector never normalised (n.h = n.(l + v) * rsq(|l + v|^2)), and the scalar factors gathered before they meet the
                // colour:  lit += (kd + f * spec) * (colour * flicker) * (intensity * (n.l)^2).  Every operand stays within a few ulp
                // of the reference's; a fragment outside the range, behind the light (n.l = 0) or without a specular lobe contributes
                // exactly what it contributes there: nothing.  Magnitudes outside the window (zero, denormal, infinite, NaN) leave
                // through the exact path below.
                // Every fragment-independent factor is read from the light's LightFast record -- made by the host with the frame,
                // fetched through the scalar cache: no VALU instruction on a wave-uniform operand is left in the loop.
                // t = clamp((distance - end) / (start - end)) as ONE fused multiply-add, distance * ss_r + (-end * ss_r); colour,
                // intensity and flicker arrive as one product.  The range test and the full-intensity test ARE the clamp of the
                // smoothstep: beyond the end distance t = 0 and the term is exactly +0 added to lit; inside the start distance t = 1
                // and the smoothstep is exactly 1.  No compare, no select, no divergent branch (the wave-level culling has already
                // dropped the lights that reach no fragment of the wave).  The clamps are output modifiers of the multiplies.
                if ((fast_mask >> li_lane) & 1ull) {
                    const LightFast LF = uniform_record_x8(P.lights_fast, li);  // one s_load_dwordx8
                    const f3 d = sub3(mk3(LF.pos[0], LF.pos[1], LF.pos[2]), F.world);
                    const float m2 = fmaf(d.z, d.z, fmaf(d.y, d.y, d.x * d.x));
                    if (rxm::wave_all(rxm::sq_in_window(m2))) {
                        const float inv = __builtin_amdgcn_rsqf(m2);
                        const float t = __builtin_amdgcn_fmed3f(fmaf(m2 * inv, LF.ss_r, LF.c0), 0.0f, 1.0f);
                        const float ss = t * t * fmaf(-2.0f, t, 3.0f);
                        // max(n.l, 0) and max(n.h, 0) as clamps to [0, 1] (both are cosines: at most 1 + 2 ulp); l = d / |d| is never
                        // formed: n.l = (n.d) / |d| and l + v = d / |d| + v as one fused multiply-add per component
                        const float ndl = __builtin_amdgcn_fmed3f(fmaf(F.normal.z, d.z, fmaf(F.normal.y, d.y, F.normal.x * d.x)) * inv, 0.0f, 1.0f);
                        const f3 hu = mk3(fmaf(d.x, inv, F.view_dir.x), fmaf(d.y, inv, F.view_dir.y), fmaf(d.z, inv, F.view_dir.z));
                        const float hh = fmaf(hu.z, hu.z, fmaf(hu.y, hu.y, hu.x * hu.x));  // 0 (l = -v: n.h = NaN -> 0 below) or >= 1e-15
                        const float ndh = __builtin_amdgcn_fmed3f(fmaf(F.normal.z, hu.z, fmaf(F.normal.y, hu.y, F.normal.x * hu.x)) * __builtin_amdgcn_rsqf(hh), 0.0f, 1.0f);
                        // At levels without programs nothing sets roughness: rough = 0.5, shininess = 2 / 0.25 - 2 = 6 exactly, and the
                        // reference's powf(n.h, 6) is three multiplies (each within half an ulp: closer to powf than exp2(6 log2 x),
                        // whose v_log_f32 error the exponent multiplies by six) instead of two quarter-rate transcendentals
                        float spec;
                        if constexpr (!feat<LV>.programs) {
                            const float ndh2 = ndh * ndh;
                            spec = ndh2 * ndh2 * ndh2;
                        } else {
                            spec = __builtin_amdgcn_exp2f(rl_shininess * __builtin_amdgcn_logf(ndh));  // (0 for n.h = 0)
                        }
                        const float s = ss * ndl * ndl;
                        F.lit.x = fmaf(fmaf(rl_f.x, spec, rl_kd.x), LF.cfi[0] * s, F.lit.x);
                        F.lit.y = fmaf(fmaf(rl_f.y, spec, rl_kd.y), LF.cfi[1] * s, F.lit.y);
                        F.lit.z = fmaf(fmaf(rl_f.z, spec, rl_kd.z), LF.cfi[2] * s, F.lit.z);
                        continue;
                    }
                }
            }
            if constexpr (RL) {
                ss_r = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ss_rcp), li_lane));
                ss_fast = (ss_ok_mask >> li_lane) & 1ull;
            }
            const rxr_light L = uniform_record(P.lights, li);
            const f3 lp = mk3(L.position[0], L.position[1], L.position[2]);
            f3 incoming, ldir;
            if (L.light_type == RXR_LIGHT_POINT) {
                // calculate_point_light (light.rs:535-552) sharing d = lp - world with the caller's
                // (lp - world).normalized(): |world - lp| and |lp - world| are the same float
                if (!L.emitting) continue;
                f3 d = sub3(lp, F.world);
                float distance;
                ldir = norm3_fast(d, distance);
                if (distance >= L.end_distance) continue;
                float intensity = L.intensity;
                if (!(distance <= L.start_distance)) {
                    // smoothstep_rs(end, start, distance) with the shared reciprocal
                    const float sn = distance - L.end_distance, sd = L.start_distance - L.end_distance;
                    float q;
                    if (ss_fast && rxm::wave_all(rxm::in_window(sn))) q = rxm::div_chain(sn, sd, ss_r);
                    else q = sn / sd;
                    const float t = rclamp(q, 0.0f, 1.0f);
                    intensity = L.intensity * (t * t * (3.0f - 2.0f * t));
                }
                incoming = apply_flicker(L, intensity, P.hash_anim);
            } else {
                if (!light_color_at(L, F.world, P.hash_anim, false, incoming)) continue;
                ldir = norm3_fast(sub3(lp, F.world));
            }
            const float n_dot_l = fmaxf(dot3(F.normal, ldir), 0.0f);  // the Lambert term of radiance_at (light.rs:529-532) and of the BRDF
            f3 radiance;
            if (L.light_type == RXR_LIGHT_AMBIENT || L.light_type == RXR_LIGHT_AMBIENT_DAYLIGHT || L.light_type == RXR_LIGHT_DAYLIGHT) {
                radiance = incoming;
            } else {
                radiance = scale3(incoming, n_dot_l);
            }
            // (relaxed kernels: the general path is the rare one -- its light-independent factors (f0, kd, the Fresnel term) must not
            // be hoisted in front of the loop, where every wave would pay for them: the empty asm ties them to this iteration)
            float rough_g = rough, metal_g = metal;
            if constexpr (RL) asm volatile("" : "+v"(rough_g), "+v"(metal_g));
            F.lit = add3(F.lit, shade_fast_brdf<RL>(F.base, rough_g, metal_g, F.normal, F.view_dir, ldir, radiance, n_dot_l));  // (continuous for every light type)
        }
    }
}

// encode (:1394-1404).  `lit += mat_emissive` (:1394): at levels without programs none runs and emissive is 0 -- adding it cannot
// change the encoded byte (x + 0 == x except -0 + 0 == +0, and both encode to 0)
template <Level LV, bool RL = false>
__device__ __forceinline__ uint32_t shade3d_end(const Frag &F) {
    f3 lit = F.lit;
    if constexpr (feat<LV>.programs) lit = add3(lit, F.emis);
    // (a baked texture or a program may replace the opacity: encoded from the float there; else the texel's own byte, see Frag)
    uint32_t alpha;
    if constexpr (feat<LV>.chunk || feat<LV>.programs) alpha = f32_to_u8_saturated(F.opacity) << 24;
    else alpha = F.alpha_bits;
    if constexpr (RL) {  // linear_to_srgb_fast (:26-33) with v_sqrt_f32 (1 ulp) for the correctly rounded root
        const float sx = __builtin_amdgcn_sqrtf(lit.x), sy = __builtin_amdgcn_sqrtf(lit.y), sz = __builtin_amdgcn_sqrtf(lit.z);
        return pack4(f32_to_u8_saturated(1.055f * sx - 0.055f * sx * sx), f32_to_u8_saturated(1.055f * sy - 0.055f * sy * sy),
                     f32_to_u8_saturated(1.055f * sz - 0.055f * sz * sz), 0u) | alpha;
    }
    return pack4(f32_to_u8_saturated(linear_to_srgb_fast(lit.x)), f32_to_u8_saturated(linear_to_srgb_fast(lit.y)),
                 f32_to_u8_saturated(linear_to_srgb_fast(lit.z)), 0u) | alpha;
}

// the covered-fragment block of d3_rasterize_opacity (rasterizer.rs:1497-1682, no shader)
template <Level LV>
__device__ __forceinline__ uint32_t shade3d_opacity(const RasterParams &P, const TriShade &S, uint32_t batch_id, float alpha, float beta,
                                                    float z, float fx, float fy) {
    const DevBatch &B = P.batches3d[batch_id];
    float gamma = 1.0f - alpha - beta;
    float u, v;
    fragment_uv(S, alpha, beta, gamma, u, v);
    // screen_to_world (:1515, :1707-1727): needed by terrain texels and by programs
    float wx = 0.0f, wy = 0.0f, wz = 0.0f;
    if ((feat<LV>.chunk && (B.flags & DB_TERRAIN)) || (feat<LV>.programs && B.program_plus1)) {
        float x_ndc = 2.0f * (fx / P.fwidth) - 1.0f;
        float y_ndc = 1.0f - 2.0f * (fy / P.fheight);
        float vx, vy, vz, vw, ww;
        mat4_mul(P.inv_proj, x_ndc, y_ndc, z, 1.0f, vx, vy, vz, vw);
        vx = vx / vw;
        vy = vy / vw;
        vz = vz / vw;
        vw = vw / vw;
        mat4_mul(P.inv_view, vx, vy, vz, vw, wx, wy, wz, ww);
    }
    const f3 world3 = mk3(wx, wy, wz);
    uint32_t texel = batch_texel<LV>(P, B, u, v, wx, wz, &world3);
    const float INV_255 = 1.0f / 255.0f;
    float r = srgb_to_linear_fast((float)(texel & 0xFFu) * INV_255);
    float g = srgb_to_linear_fast((float)((texel >> 8) & 0xFFu) * INV_255);
    float b = srgb_to_linear_fast((float)((texel >> 16) & 0xFFu) * INV_255);
    float opacity = byte_over_255(texel >> 24);
    if constexpr (feat<LV>.programs) {
        if (B.program_plus1) {  // :1642-1667
            rxvm::IO io;
            rxvm::io_defaults(io);
            io.color = rxvm::mk(r, g, b);
            io.opacity.x = opacity;
            io.uv.x = u / 4.0f;
            io.uv.y = v / 4.0f;
            io.hitpoint = rxvm::mk(wx, wy, wz);
            io.time = rxvm::splat(P.time);
            io.roughness.x = 0.5f;
            io.metallic.x = 0.0f;
            rxvm::shade_call<feat<LV>.ssp>(P, B.program_plus1 - 1u, io);
            r = io.color.x;
            g = io.color.y;
            b = io.color.z;
            opacity = io.opacity.x;
        }
    }
    return pack4(f32_to_u8_saturated(linear_to_srgb_fast(r)), f32_to_u8_saturated(linear_to_srgb_fast(g)),
                 f32_to_u8_saturated(linear_to_srgb_fast(b)), f32_to_u8_saturated(opacity));
}

// one 2D fragment (rasterizer.rs:656-895); returns the new pixel
template <Level LV>
__device__ __forceinline__ uint32_t fragment2d(const RasterParams &P, const Prim2D &T, const DevBatch &B, uint32_t px, uint32_t py,
                                               float fx, float fy, uint32_t dst) {
    // barycentric_weights_2d (rasterizer.rs:1731-1750)
    float acx = T.v2x - T.v0x, acy = T.v2y - T.v0y;
    float abx = T.v1x - T.v0x, aby = T.v1y - T.v0y;
    float apx = fx - T.v0x, apy = fy - T.v0y;
    float pcx = T.v2x - fx, pcy = T.v2y - fy;
    float pbx = T.v1x - fx, pby = T.v1y - fy;
    float area = acx * aby - acy * abx;
    float w0 = (pcx * pby - pcy * pbx) / area;
    float w1 = (acx * apy - acy * apx) / area;
    float w2 = 1.0f - w0 - w1;
    float u = T.u0 * w0 + T.u1 * w1 + T.u2 * w2;
    float v = T.v0 * w0 + T.v1 * w1 + T.v2 * w2;

    // :664-670
    float gx = ((float)px - P.fwidth / 2.0f) - (P.translationd2[0] - P.fwidth / 2.0f);
    float gy = ((float)py - P.fheight / 2.0f) - (P.translationd2[1] - P.fheight / 2.0f);
    float wx = gx / P.scaled2, wy = gy / P.scaled2;

    uint32_t texel = batch_texel<LV, true>(P, B, u, v, wx, wy);  // 2D terrain: chunk.sample_terrain_texture(world, ..), :749-751
    if constexpr (feat<LV>.programs) {
        if (B.program_plus1 && P.programs[B.program_plus1 - 1u].shade_entry != 0xFFFFFFFFu) {  // :760-797
            const float INV_255 = 1.0f / 255.0f;  // pixel_to_vec4, lib.rs:52-62
            rxvm::IO io;
            rxvm::io_defaults(io);
            io.uv.x = u / 4.0f;
            io.uv.y = v / 4.0f;
            io.color = rxvm::mk((float)(texel & 0xFFu) * INV_255, (float)((texel >> 8) & 0xFFu) * INV_255, (float)((texel >> 16) & 0xFFu) * INV_255);
            io.hitpoint.x = wx;
            io.hitpoint.y = wy;
            io.time = rxvm::splat(P.time);
            io.roughness.x = 0.5f;
            io.metallic.x = 0.0f;
            rxvm::shade_call<feat<LV>.ssp>(P, B.program_plus1 - 1u, io);
            texel = pack4(f32_to_u8_saturated(io.color.x), f32_to_u8_saturated(io.color.y), f32_to_u8_saturated(io.color.z), 255u);
        }
    }
    uint32_t tr = texel & 0xFFu, tg = (texel >> 8) & 0xFFu, tb = (texel >> 16) & 0xFFu, ta = texel >> 24;

    // :799-873 -- note the reference's precedence: (receives_light && any lights) || ambient
    if (((B.flags & DB_RECEIVES_LIGHT) && P.any_lights) || (P.flags & RXR_FLAG_HAS_AMBIENT)) {
        float acc0 = 0.0f, acc1 = 0.0f, acc2 = 0.0f;
        uint32_t occ_first = 0, occ_count = P.n_occluders;
        if (B.chunk >= 0) {
            ChunkRange cr = P.chunks[B.chunk];
            occ_first = cr.occ_first;
            occ_count = cr.occ_count;
        }
        if (P.flags & RXR_FLAG_HAS_AMBIENT) {
            float occlusion = get_occlusion(P.occluders, occ_first, occ_count, wx, wy);
            acc0 += P.ambient[0] * occlusion;
            acc1 += P.ambient[1] * occlusion;
            acc2 += P.ambient[2] * occlusion;
        }
        for (uint32_t li = 0; li < P.n_lights; ++li) {
            const rxr_light L = uniform_record(P.lights, li);
            f3 lc;
            if (!light_color_at(L, mk3(wx, 0.0f, wy), P.hash_anim, true, lc)) continue;
            bool visible = true;
            if (L.light_type == RXR_LIGHT_AMBIENT_DAYLIGHT) {
                float occlusion = get_occlusion(P.occluders, occ_first, occ_count, wx, wy);
                lc = scale3(lc, occlusion);
            }
            if (L.light_type != RXR_LIGHT_AMBIENT && L.light_type != RXR_LIGHT_AMBIENT_DAYLIGHT &&
                !mapmini_is_visible(P.linedefs, P.n_linedefs, wx, wy, L.position[0], L.position[2]))
                visible = false;
            if (visible) {
                acc0 += lc.x;
                acc1 += lc.y;
                acc2 += lc.z;
            }
        }
        acc0 = rclamp(acc0, 0.0f, 1.0f);
        acc1 = rclamp(acc1, 0.0f, 1.0f);
        acc2 = rclamp(acc2, 0.0f, 1.0f);
        tr = sat_u8(rclamp((byte_over_255(tr) * acc0) * 255.0f, 0.0f, 255.0f));
        tg = sat_u8(rclamp((byte_over_255(tg) * acc1) * 255.0f, 0.0f, 255.0f));
        tb = sat_u8(rclamp((byte_over_255(tb) * acc2) * 255.0f, 0.0f, 255.0f));
    }

    if (ta == 255u) return pack4(tr, tg, tb, ta);  // :878-879
    float src_alpha = byte_over_255(ta);
    float dst_alpha = 1.0f - src_alpha;
    uint32_t dr = dst & 0xFFu, dg = (dst >> 8) & 0xFFu, db = (dst >> 16) & 0xFFu, da = dst >> 24;
    uint32_t orr = sat_u8(((float)tr * src_alpha) + ((float)dr * dst_alpha));
    uint32_t og = sat_u8(((float)tg * src_alpha) + ((float)dg * dst_alpha));
    uint32_t ob = sat_u8(((float)tb * src_alpha) + ((float)db * dst_alpha));
    uint32_t oa = (P.flags & RXR_FLAG_PRESERVE_TRANSPARENCY) ? max(da, ta) : 255u;
    return pack4(orr, og, ob, oa);
}

// A pixel no 3D fragment reached, with a brush preview (rasterizer.rs:420-461): screen_ray (:1841-1869) through the pixel's
// CORNER ((tile.x + tx) as f32, no + 0.5, :422-423), intersected with the plane y = 0, white blended over black.
__device__ __forceinline__ uint32_t miss_brush_preview(const RasterParams &P, uint32_t px, uint32_t py) {
    const float ndc_x = 2.0f * ((float)px / P.fwidth) - 1.0f;
    const float ndc_y = 1.0f - 2.0f * ((float)py / P.fheight);
    float nx, ny, nz, nw, fx_, fy_, fz_, fw_;
    mat4_mul(P.inv_proj, ndc_x, ndc_y, -1.0f, 1.0f, nx, ny, nz, nw);
    mat4_mul(P.inv_proj, ndc_x, ndc_y, 1.0f, 1.0f, fx_, fy_, fz_, fw_);
    nx = nx / nw; ny = ny / nw; nz = nz / nw; nw = nw / nw;
    fx_ = fx_ / fw_; fy_ = fy_ / fw_; fz_ = fz_ / fw_; fw_ = fw_ / fw_;
    float ox, oy, oz, ow, tx, ty, tz, tw;
    mat4_mul(P.inv_view, nx, ny, nz, nw, ox, oy, oz, ow);
    mat4_mul(P.inv_view, fx_, fy_, fz_, fw_, tx, ty, tz, tw);
    const f3 origin = mk3(ox, oy, oz);
    const f3 dir = norm3(sub3(mk3(tx, ty, tz), origin));
    float c = 0.0f;
    if (fabsf(dir.y) > 1e-5f) {
        const float t = -origin.y / dir.y;
        if (t > 0.0f) {
            bool inside;
            const float blend = brush_blend(P, add3(origin, scale3(dir, t)), inside);
            if (inside) c = fminf(0.0f * (1.0f - blend) + blend, 1.0f);
        }
    }
    const uint32_t g = f32_to_u8_saturated(c);
    return pack4(g, g, g, f32_to_u8_saturated(1.0f));
}

// bins (launch-local tile rows l0..l1, tile columns bx0..bx1) touched by a clamped pixel box
__device__ __forceinline__ bool bin_range(const RasterParams &P, uint32_t min_x, uint32_t max_x, uint32_t min_y, uint32_t max_y,
                                          uint32_t &bx0, uint32_t &bx1, uint32_t &l0, uint32_t &l1) {
    if (!(min_x < max_x && min_y < max_y) || P.tiles_y == 0) return false;
    bx0 = min_x / RXR_TILE_W;
    bx1 = (max_x - 1) / RXR_TILE_W;
    uint32_t g0 = min_y / RXR_TILE_H, g1 = (max_y - 1) / RXR_TILE_H;  // frame tile rows
    if (g1 < P.tile_y0) return false;
    l0 = g0 <= P.tile_y0 ? 0u : (g0 - P.tile_y0 + P.tile_stride - 1u) / P.tile_stride;
    l1 = (g1 - P.tile_y0) / P.tile_stride;
    if (l1 >= P.tiles_y) l1 = P.tiles_y - 1u;
    return l0 <= l1;
}

// Per-triangle set-up shared by k_setup3d and the fused small-scene path of k_raster: de-indexes the
// batch arrays into the TriSetup / TriShade records (per-triangle constants of the reference's
// per-fragment formulas, rasterizer.rs:989-995, 1054-1072, 1754-1767) and computes the clamped pixel
// box (:998-1017, tile = whole width x row band).  Returns false when no pixel can be produced
// (invisible edge, skipped batch, empty box); then only S.bx / S.by (an empty pixel box) are meaningful.
__device__ __forceinline__ bool make_setup(const RasterParams &P, uint32_t t, TriSetup &S, TriShade &H) {
    // triangle -> batch: looked up (small frames: the table written at upload) or searched (largest b with base[b] <= t)
    uint32_t lo = 0, hi = P.n_batches3d;
    const bool have_info = P.tri_info != nullptr;  // uniform
    uint2 info = make_uint2(0u, 0u);
    if (have_info) {
        info = P.tri_info[t];
        lo = info.x;
    } else {
        while (hi - lo > 1) {
            uint32_t mid = (lo + hi) >> 1;
            if (P.batch_tri_base[mid] <= t) lo = mid;
            else hi = mid;
        }
    }
    if (P.mesh_live && t - P.batch_tri_base[lo] >= P.mesh_live[lo]) {  // an unused slot of a device-projected mesh: nothing to read
        S.bx = S.by = 0u;
        return false;
    }
    // (with the table the index triple and the edge record do not wait for the batch header: two levels of loads instead of seven)
    const bool own_edges = P.pm_meshes != nullptr;  // uniform: a device-projected frame whose Edges records are built here (below)
    const bool host_edgeless = P.edge_vis3d != nullptr;  // uniform: a host-projected frame handed over without its Edges records (ABI 5)
    rxr_edges E;
    if (!own_edges && !host_edgeless) E = P.edges[t];
    const uint32_t ix0 = P.idx[3 * (size_t)t + 0], ix1 = P.idx[3 * (size_t)t + 1], ix2 = P.idx[3 * (size_t)t + 2];
    const DevBatch B = P.batches3d[lo];
    const uint32_t vbase = have_info ? info.y : B.vert_base;
    if (own_edges) {
        // k_proj_edges, fused: the slot is in use (mesh_live above), its edge_visibility is the original triangle's or, for an
        // appended fan, true; the record is Edges::new of the projected vertices under the mesh's cull mode (edges_from_vertices,
        // rxr_project.h -- the same function k_proj_edges calls).  40 B per slot are neither written nor read back.
        const DevMesh &M = P.pm_meshes[lo];
        const uint32_t local = t - P.batch_tri_base[lo];
        const bool evis = local < M.n_tris ? P.pm_edge_vis[M.tin_base + local] != 0 : true;
        E = edges_from_vertices(M.cull_mode, evis, P.pv[ix0 + vbase], P.pv[ix1 + vbase], P.pv[ix2 + vbase]);
    } else if (host_edgeless) {
        // Edges::new of the projected vertices under the batch's cull mode: what the host computed and did not send (40 bytes per triangle
        // that are a function of the vertices it sent).  `visible` arrives as a word per triangle.
        E = edges_from_vertices(B.mode, P.edge_vis3d[t] != 0u, P.pv[ix0 + vbase], P.pv[ix1 + vbase], P.pv[ix2 + vbase]);
    }

    // triangles that can never produce a pixel (culled / clipped away: edges.visible == false, :989-992; skipped batch;
    // batch box off screen) are known before any vertex is read: they only get an empty pixel box
    bool skip = (B.flags & DB_SKIP) != 0;
    if (P.dev_bbox) {
        // device-projection path: the batch-level box reject (rasterizer.rs:978-983, whole screen) on the
        // box accumulated by rxr_project.hip; Rect {x, y, width = max - min, height} as batch3d.rs:762-767
        const DevBBox bb = P.dev_bbox[lo];
        auto dec = [](uint32_t e) { return __uint_as_float((e & 0x80000000u) ? (e ^ 0x80000000u) : ~e); };
        float bx = dec(bb.min_x), by = dec(bb.min_y), bw = dec(bb.max_x) - bx, bh = dec(bb.max_y) - by;
        bool keep = bx < (float)P.width && (bx + bw) > 0.0f && by < (float)P.height && (by + bh) > 0.0f;
        skip = skip || !keep;
    }
    if (!E.visible || skip) {
        S.bx = S.by = 0u;
        return false;
    }

    // the fetch; the arithmetic is rxr_tri_records (rxr_device.h), which the host runs as well for the frames whose records it builds
    const uint32_t i0 = ix0 + vbase, i1 = ix1 + vbase, i2 = ix2 + vbase;
    const float4 v0 = P.pv[i0], v1 = P.pv[i1], v2 = P.pv[i2];
    const float2 uv0 = P.uv[i0], uv1 = P.uv[i1], uv2 = P.uv[i2];
    TriRecordIn in;
    in.v[0][0] = v0.x; in.v[0][1] = v0.y; in.v[0][2] = v0.z; in.v[0][3] = v0.w;
    in.v[1][0] = v1.x; in.v[1][1] = v1.y; in.v[1][2] = v1.z; in.v[1][3] = v1.w;
    in.v[2][0] = v2.x; in.v[2][1] = v2.y; in.v[2][2] = v2.z; in.v[2][3] = v2.w;
    in.uv[0][0] = uv0.x; in.uv[0][1] = uv0.y; in.uv[1][0] = uv1.x; in.uv[1][1] = uv1.y; in.uv[2][0] = uv2.x; in.uv[2][1] = uv2.y;
    if (B.flags & DB_HAS_NORMALS) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            in.n[0][k] = P.nrm[3 * (size_t)i0 + k];
            in.n[1][k] = P.nrm[3 * (size_t)i1 + k];
            in.n[2][k] = P.nrm[3 * (size_t)i2 + k];
        }
    } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) in.n[0][k] = in.n[1][k] = in.n[2][k] = 0.0f;
    }
    in.E = E;
    in.batch = lo;
    in.bflags = B.flags;
    in.profile_id = B.profile_id;
    in.repeat_mode = B.repeat_mode;
    in.tex = B.tex;
    in.desc = DevTexDesc{};
    if (B.tex >= 0 && !(B.flags & DB_TERRAIN) && B.repeat_mode < 4u) in.desc = P.tex[B.tex];
    in.sample_mode = P.sample_mode;
    in.width = P.width;
    in.row0 = P.row0;
    in.row1 = P.row1;
    // the clip rectangle of the pixel box (rxr_tri_records): the pixels of the tiles that pass the reference's batch box test
    in.has_clip = 0u;
    in.clip[0] = in.clip[1] = in.clip[2] = in.clip[3] = 0u;
    if (P.batch_clip3d) {   // uniform: host-projected, some batch is risky or the frame takes row spans
        const uint4 c = P.batch_clip3d[lo];
        in.has_clip = 1u;
        in.clip[0] = c.x; in.clip[1] = c.y; in.clip[2] = c.z; in.clip[3] = c.w;
    } else if (P.dev_bbox) {   // device-projected: the box is here
        const DevBBox bb = P.dev_bbox[lo];
        auto dec = [](uint32_t e) { return __uint_as_float((e & 0x80000000u) ? (e ^ 0x80000000u) : ~e); };
        const float bx = dec(bb.min_x), by = dec(bb.min_y), bw = dec(bb.max_x) - bx, bh = dec(bb.max_y) - by;
        if (P.row_spans || rxr_box_is_risky(bx, by, bw, bh)) {   // (row_spans: k_spans_from_meshes made them from these boxes, the same way)
            in.has_clip = 1u;
            rxr_ref_tile_span_quick(bx, bw, P.width, P.ref_tile, 0.0f, in.clip[0], in.clip[1]);
            rxr_ref_tile_span_quick(by, bh, P.height, P.ref_tile, 0.0f, in.clip[2], in.clip[3]);
        }
    }
    return rxr_tri_records(in, S, H);
}

}  // namespace

// =================================================================================================
// k_setup3d: triangle set-up + bin counting.  One thread per triangle.
// Replaces the per-tile re-derivation of per-triangle constants in rasterizer.rs:989-1017, 1054-1072.
// =================================================================================================
// Run-length aggregated "counter[bin] += 1": neighbouring triangles of a mesh (consecutive ids = consecutive lanes) fall
// into the same few bins, and atomics on one address serialise in L2 -- so a run of adjacent lanes with the same bin
// issues ONE atomic (by its first lane) for the whole run.  O(1) per call whatever the bins are; lanes whose neighbours
// target other bins simply form runs of one.  Must be called by ALL lanes of the wave (`active` marks the ones that have
// a bin); with RETURN each active lane gets a distinct slot (old value + its position in the run).
template <bool RETURN>
__device__ __forceinline__ uint32_t wave_bin_increment(uint32_t *counter, uint32_t bin, bool active) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t prev_bin = (uint32_t)__shfl_up((int)bin, 1, 64);
    const bool prev_active = __shfl_up((int)active, 1, 64) != 0;
    const bool head = !active || lane == 0u || !prev_active || bin != prev_bin;
    const unsigned long long heads = __ballot(head);
    // first lane of my run: the highest head at or below me
    const unsigned long long below = heads & (lane == 63u ? ~0ull : ((2ull << lane) - 1ull));
    const uint32_t first = 63u - (uint32_t)__clzll((long long)below);
    uint32_t base = 0;
    if (active && head) {
        const unsigned long long above = lane == 63u ? 0ull : (heads >> (lane + 1u));
        const uint32_t run = above ? (uint32_t)__ffsll((long long)above) : 64u - lane;
        base = atomicAdd(&counter[bin], run);
    }
    if (!RETURN) return 0u;
    base = (uint32_t)__shfl((int)base, (int)first, 64);
    return base + (lane - first);
}
// the same in two halves, so that a caller can have several atomics in flight before it waits for the first answer:
// `issue` returns the run head's raw answer (only meaningful on head lanes) and the lane of this lane's head
__device__ __forceinline__ uint32_t wave_bin_issue(uint32_t *counter, uint32_t bin, bool active, uint32_t &first) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t prev_bin = (uint32_t)__shfl_up((int)bin, 1, 64);
    const bool prev_active = __shfl_up((int)active, 1, 64) != 0;
    const bool head = !active || lane == 0u || !prev_active || bin != prev_bin;
    const unsigned long long heads = __ballot(head);
    const unsigned long long below = heads & (lane == 63u ? ~0ull : ((2ull << lane) - 1ull));
    first = 63u - (uint32_t)__clzll((long long)below);
    uint32_t base = 0;
    if (active && head) {
        const unsigned long long above = lane == 63u ? 0ull : (heads >> (lane + 1u));
        const uint32_t run = above ? (uint32_t)__ffsll((long long)above) : 64u - lane;
        base = atomicAdd(&counter[bin], run);
    }
    return base;
}
__device__ __forceinline__ uint32_t wave_bin_finish(uint32_t raw, uint32_t first) {
    return (uint32_t)__shfl((int)raw, (int)first, 64) + ((threadIdx.x & 63u) - first);
}

#ifndef RXR_JIT  // ---- the pre-pass kernels (not part of a run-time compiled program kernel) --------------------------------
// The records leave through LDS: a thread's own 96 + 80 bytes are eleven 16-byte stores at a stride of 96 / 80 bytes across the
// wave (every store instruction touches 64 cache lines, a sixth of each); transposed, the workgroup's 256 records are one
// contiguous 24 KB / 20 KB block that consecutive lanes write 16 bytes at a time.
// device-projected frames: true (uniformly) for a workgroup whose 256 slots all lie behind the live triangles of one mesh.  The
// pools are capacity based (3 slots per input triangle): an unclipped scene leaves two thirds of them unused, and k_setup3d /
// k_fill used to walk them all (1 M-triangle grid: 161 us instead of 87).  Such a workgroup writes and reads nothing; the bin
// lists never name its slots.  Not in small-scene mode, where the raster kernel scans the records themselves.
__device__ __forceinline__ bool dead_slots_block(const RasterParams &P, uint32_t t0) {
    if (!P.mesh_live || P.fused_small) return false;
    const uint32_t t1 = min(t0 + 255u, P.n_tris3d - 1u);
    uint32_t b[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const uint32_t t = k ? t1 : t0;
        uint32_t lo = 0, hi = P.n_batches3d;
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (P.batch_tri_base[mid] <= t) lo = mid;
            else hi = mid;
        }
        b[k] = lo;
    }
    return b[0] == b[1] && t0 - P.batch_tri_base[b[0]] >= P.mesh_live[b[0]];
}

extern "C" __global__ void __launch_bounds__(256) k_setup3d(RasterParams P) {
    const uint32_t t0 = blockIdx.x * blockDim.x;
    if (dead_slots_block(P, t0)) {
        // (k_blockscan reads the boxes of listed groups only: these four groups just say that they are empty)
        if (P.blockscan_cap && (threadIdx.x & 63u) == 0u && (blockIdx.x * 4u + (threadIdx.x >> 6)) * RXR_BLOCKSCAN_GROUP < P.n_tris3d)
            P.group_rng[blockIdx.x * 4u + (threadIdx.x >> 6)] = make_uint2(0xFFFFu, 0xFFFFu);
        return;
    }
    uint32_t t = t0 + threadIdx.x;
    bool live = false;
    TriSetup S = {};
    TriShade H = {};
    if (t < P.n_tris3d) {
        live = make_setup(P, t, S, H);
        P.tri_box[t] = make_uint2(S.bx, S.by);
    }
    {
        // (a triangle that can never be a candidate -- culled, clipped away, empty box -- has bx = by = 0: the lists skip it and
        // the implicit-list path rejects its empty box; its other fields are whatever make_setup got to, zero at the least)
        __shared__ uint4 xpose[256 * 6];
        const uint32_t tid = threadIdx.x;
        const uint32_t n_here = min(256u, P.n_tris3d - t0);   // the grid covers n_tris3d: t0 < n_tris3d
        // a workgroup without a single live triangle (the unused output slots behind a device-projected mesh: two thirds of
        // the slots of an unclipped scene) only marks its records as empty
        if (!__syncthreads_or(live ? 1 : 0)) {
            if (t < P.n_tris3d) *reinterpret_cast<uint2 *>(&P.tri_setup[t].bx) = make_uint2(0u, 0u);
            if (P.blockscan_cap && (threadIdx.x & 63u) == 0u && (blockIdx.x * 4u + (threadIdx.x >> 6)) * RXR_BLOCKSCAN_GROUP < P.n_tris3d)
                P.group_rng[blockIdx.x * 4u + (threadIdx.x >> 6)] = make_uint2(0xFFFFu, 0xFFFFu);  // (empty groups)
            return;   // (nothing to bin either)
        }
        uint4 rec[6];
        __builtin_memcpy(rec, &S, sizeof(S));
#pragma unroll
        for (int i = 0; i < 6; ++i) xpose[tid * 6u + i] = rec[i];
        __syncthreads();
        uint4 *dst = reinterpret_cast<uint4 *>(P.tri_setup + t0);
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            const uint32_t k = (uint32_t)i * 256u + tid;
            if (k < n_here * 6u) dst[k] = xpose[k];
        }
        __syncthreads();
        __builtin_memcpy(rec, &H, sizeof(H));
#pragma unroll
        for (int i = 0; i < 5; ++i) xpose[tid * 5u + i] = rec[i];
        __syncthreads();
        dst = reinterpret_cast<uint4 *>(P.tri_shade + t0);
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            const uint32_t k = (uint32_t)i * 256u + tid;
            if (k < n_here * 5u) dst[k] = xpose[k];
        }
    }
    if (P.blockscan_cap) {  // uniform: k_blockscan bins this launch -- every wave leaves it the union of its 64 triangles' bin ranges
        uint32_t gx0 = 0xFFFFu, gx1 = 0u, gy0 = 0xFFFFu, gy1 = 0u;  // (empty: x0 > x1)
        if (live) {
            uint32_t bx0, bx1, l0, l1;
            if (bin_range(P, S.bx & 0xFFFFu, S.bx >> 16, S.by & 0xFFFFu, S.by >> 16, bx0, bx1, l0, l1)) {
                gx0 = bx0;
                gx1 = bx1;
                gy0 = l0;
                gy1 = l1;
            }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            gx0 = min(gx0, (uint32_t)__shfl_xor((int)gx0, d, 64));
            gx1 = max(gx1, (uint32_t)__shfl_xor((int)gx1, d, 64));
            gy0 = min(gy0, (uint32_t)__shfl_xor((int)gy0, d, 64));
            gy1 = max(gy1, (uint32_t)__shfl_xor((int)gy1, d, 64));
        }
        const uint32_t lane = threadIdx.x & 63u, g = blockIdx.x * 4u + (threadIdx.x >> 6);  // group = wave
        if (g * RXR_BLOCKSCAN_GROUP >= P.n_tris3d) return;  // (wave-uniform: a wave behind the last triangle)
        if (lane == 0u) P.group_rng[g] = gx0 <= gx1 ? make_uint2(gx0 | (gx1 << 16), gy0 | (gy1 << 16)) : make_uint2(0xFFFFu, 0xFFFFu);
        if (P.blockscan_scatter && gx0 <= gx1) {  // uniform: the group appends itself to the list of every block of 4 x 4 bins its range meets
            const uint32_t bx_lo = gx0 / 4u, by_lo = gy0 / 4u, w = gx1 / 4u - bx_lo + 1u, nbk = w * (gy1 / 4u - by_lo + 1u);
            if (nbk > RXR_BLOCKSCAN_GROUP_BLOCKS) {
                // a group all over the screen (triangles next to the camera): on the list every block looks through
                // (counted in the launch's clean counter set, word CNT_TICKET: k_scan does not run in this mode)
                if (lane == 0u) P.blk_grp[P.blk_wide_base + atomicAdd(&P.counters[CNT_TICKET], 1u)] = g;
            } else if (lane < nbk) {  // one lane per block
                const uint32_t b = (by_lo + lane / w) * ((P.tiles_x + 3u) / 4u) + bx_lo + lane % w;
                const uint32_t pos = atomicAdd(&P.blk_cnt[b], 1u);
                if (pos < RXR_BLOCKSCAN_BLOCK_GROUPS) P.blk_grp[(size_t)b * RXR_BLOCKSCAN_BLOCK_GROUPS + pos] = g;  // (else k_blockscan sees the count)
            }
        }
        return;
    }
    if (P.fused_small) return;  // small scenes are not binned (see scan_implicit); uniform
    uint32_t bx0 = 0, bx1 = 0, by0 = 0, by1 = 0, nb = 0;
    if (live) {
        const uint32_t min_x = S.bx & 0xFFFFu, max_x = S.bx >> 16, min_y = S.by & 0xFFFFu, max_y = S.by >> 16;
        if (bin_range(P, min_x, max_x, min_y, max_y, bx0, bx1, by0, by1)) nb = (bx1 - bx0 + 1) * (by1 - by0 + 1);
    }
    if (nb > RXR_LARGE_BINS) {
        uint32_t slot = atomicAdd(&P.counters[CNT_LARGE], 1u);
        if (slot < P.n_tris3d) P.large_list[slot] = t;  // (always true while the counter invariant holds)
        nb = 0;
    }
    // step k of every lane's own (bx, by) walk, the whole wave in lockstep
    const uint32_t w = bx1 - bx0 + 1;
    for (uint32_t k = 0; __ballot(k < nb); ++k) {
        const bool active = k < nb;
        const uint32_t bin = active ? (by0 + k / w) * P.tiles_x + (bx0 + k % w) : 0u;
        wave_bin_increment<false>(P.bin_count, bin, active);
    }
}

// =================================================================================================
// k_scan: exclusive scan of bin_count.  One 256-thread workgroup per chunk of 2048 bins writes
// chunk-local offsets; the workgroup that finishes last (ticket counter) scans the chunk totals,
// publishes the totals to the host-visible status words and clears the other counter set.
// =================================================================================================
extern "C" __global__ void __launch_bounds__(256) k_scan(ScanArgs A) {
    __shared__ uint32_t wave_tot[4];
    __shared__ uint32_t s_last;
    const uint32_t n = A.n;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    constexpr uint32_t PER = RXR_SCAN_CHUNK / 256u;
    const uint32_t i0 = blockIdx.x * RXR_SCAN_CHUNK + tid * PER;
    uint32_t v[PER];
    uint32_t sum = 0;
#pragma unroll
    for (uint32_t k = 0; k < PER; ++k) {
        uint32_t i = i0 + k;
        v[k] = (i < n) ? A.count[i] : 0u;
        sum += v[k];
    }
    uint32_t inc = sum;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        uint32_t o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    if (lane == 63) wave_tot[wave] = inc;
    __syncthreads();
    uint32_t wave_off = 0, total = 0;
#pragma unroll
    for (uint32_t w = 0; w < 4; ++w) {
        uint32_t wt = wave_tot[w];
        if (w < wave) wave_off += wt;
        total += wt;
    }
    uint32_t run = wave_off + (inc - sum);
#pragma unroll
    for (uint32_t k = 0; k < PER; ++k) {
        uint32_t i = i0 + k;
        if (i < n) {
            A.offset[i] = run;
            A.cursor[i] = 0u;
        }
        run += v[k];
    }
    if (tid == 0) {
        __hip_atomic_store(&A.chunk_tot[blockIdx.x], total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __threadfence();
        uint32_t ticket = atomicAdd(&A.counters[CNT_TICKET], 1u);
        s_last = (ticket == gridDim.x - 1u) ? 1u : 0u;
    }
    __syncthreads();
    if (!s_last || wave != 0) return;
    // last workgroup, wave 0: scan the chunk totals
    __threadfence();
    uint32_t carry = 0;
    for (uint32_t base = 0; base < gridDim.x; base += 64u) {
        uint32_t c = base + lane;
        uint32_t t = (c < gridDim.x) ? __hip_atomic_load(&A.chunk_tot[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
        uint32_t ic = t;
#pragma unroll
        for (uint32_t d = 1; d < 64; d <<= 1) {
            uint32_t o = __shfl_up(ic, d, 64);
            if (lane >= d) ic += o;
        }
        if (c < gridDim.x) A.chunk_base[c] = carry + ic - t;
        carry += __shfl(ic, 63, 64);
    }
    if (lane == 0) {
        const uint32_t overflow = carry > A.list_capacity ? 1u : 0u;
        A.counters[CNT_ENTRIES] = carry;
        A.counters[CNT_OVERFLOW] = overflow;
        // host words: the entry count of this launch; the overflow flag and the largest overflowing count are STICKY (only
        // ever set / raised here, cleared by rxr_synchronize once the streams have drained), so that an asynchronous caller
        // learns about ANY overflowed launch, not only the last one
        A.host_status[CNT_ENTRIES] = carry;
        if (overflow) {
            A.host_status[CNT_OVERFLOW] = 1u;
            if (carry > A.host_status[CNT_LARGE]) A.host_status[CNT_LARGE] = carry;  // (HS_MAX_ENTRIES, rxr_ctx.h)
        }
    }
    if (lane < CNT_WORDS) A.counters_next[lane] = 0u;
}

// =================================================================================================
// k_fill: scatter triangle ids into the bin lists (order inside a bin is irrelevant, see header)
// =================================================================================================
#ifndef RXR_FILL_DEPTH
#define RXR_FILL_DEPTH 8
#endif
// step k of every lane's own (bx, by) walk, the whole wave in lockstep, U steps in flight
template <uint32_t U>
__device__ __forceinline__ void fill_lockstep(const RasterParams &P, uint32_t t, uint32_t nb, uint32_t max_nb, uint32_t w, uint32_t bx0, uint32_t by0) {
    for (uint32_t k0 = 0; k0 < max_nb; k0 += U) {
        uint32_t raw[U], first[U], cb[U], bo[U];
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) {
            const uint32_t k = k0 + u;
            const bool active = k < nb;
            raw[u] = first[u] = cb[u] = bo[u] = 0u;
            if (U == 1u || k < max_nb) {  // wave-uniform
                const uint32_t bin = active ? (by0 + k / w) * P.tiles_x + (bx0 + k % w) : 0u;
                raw[u] = wave_bin_issue(P.bin_cursor, bin, active, first[u]);
                if (active) {
                    cb[u] = P.chunk_base[bin / RXR_SCAN_CHUNK];
                    bo[u] = P.bin_offset[bin];
                }
            }
        }
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) {
            const uint32_t k = k0 + u;
            if (U == 1u || k < max_nb) {  // wave-uniform
                const uint32_t pos = cb[u] + bo[u] + wave_bin_finish(raw[u], first[u]);
                if (k < nb && pos < P.list_capacity) P.bin_list[pos] = t;
            }
        }
    }
}
extern "C" __global__ void __launch_bounds__(256) k_fill(RasterParams P) {
    // Every (triangle, bin) pair needs one atomic WITH a return value (its slot in the bin), i.e. one memory round trip.
    // Walking "step k of every lane's own bin loop" serialises max(bins per triangle) round trips per wave -- 48 for a mesh
    // of mid-sized triangles (teapot at 1080p: k_fill 19 us for 2256 triangles).  Instead the wave flattens its pairs: an
    // exclusive prefix sum of the lanes' bin counts, then pair i belongs to lane (i mod 64), which finds the owning
    // triangle by a binary search over the prefix with shuffles -- ceil(pairs / 64) round trips, all lanes busy.
    if (dead_slots_block(P, blockIdx.x * blockDim.x)) return;  // (k_setup3d left these slots' boxes unwritten)
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t bx0 = 0, bx1 = 0, by0 = 0, by1 = 0, nb = 0;
    if (t < P.n_tris3d) {
        const uint2 box = P.tri_box[t];
        uint32_t bxw = box.x, byw = box.y;
        uint32_t min_x = bxw & 0xFFFFu, max_x = bxw >> 16, min_y = byw & 0xFFFFu, max_y = byw >> 16;
        if (bin_range(P, min_x, max_x, min_y, max_y, bx0, bx1, by0, by1)) nb = (bx1 - bx0 + 1) * (by1 - by0 + 1);
        if (nb > RXR_LARGE_BINS) nb = 0;  // on the large list
    }
    const uint32_t w = bx1 - bx0 + 1;
    uint32_t inc = nb;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    const uint32_t start = inc - nb;                       // exclusive prefix: this lane's first pair
    const uint32_t total = (uint32_t)__shfl((int)inc, 63, 64);
    // Dense meshes of small triangles (few bins each, neighbours in the SAME bins) are better served by the lock-step walk
    // with its run-length aggregated atomics: one atomic per run of adjacent lanes with the same bin instead of one per
    // pair on the same address.  The flattened walk is taken when it saves at least a quarter of the round trips.
    uint32_t max_nb = nb;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) max_nb = max(max_nb, (uint32_t)__shfl_xor((int)max_nb, d, 64));
    // Either way several steps are issued before the first answer is awaited: a step is one returning atomic plus two offset
    // loads, i.e. a memory round trip, and a wave of mid-sized triangles has dozens of steps (teapot at 1080p: pre-pass
    // 49.1 -> 40.6 us with eight in flight).  Waves of small triangles (at most four steps: the 1 M-triangle grid) keep the
    // plain loop, which the unrolled form made 3 % slower.
    if (max_nb <= 8u || 4u * ((total + 63u) / 64u) > 3u * max_nb) {
        if (max_nb <= 4u) fill_lockstep<1>(P, t, nb, max_nb, w, bx0, by0);
        else fill_lockstep<RXR_FILL_DEPTH>(P, t, nb, max_nb, w, bx0, by0);
        return;
    }
    constexpr uint32_t U = RXR_FILL_DEPTH;
    for (uint32_t base = 0; base < total; base += 64u * U) {    // wave-uniform trip count
        uint32_t slot[U], cb[U], bo[U], owner_t[U];
        bool act[U];
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) {
            const uint32_t i = base + 64u * u + lane;
            act[u] = i < total;
            slot[u] = cb[u] = bo[u] = owner_t[u] = 0u;
            if (base + 64u * u < total) {  // wave-uniform
                // owner: the largest lane j with start[j] <= i (lanes without bins share their successor's start and are skipped
                // because the search prefers the larger j)
                uint32_t lo = 0, hi = 64;
#pragma unroll
                for (int step = 0; step < 6; ++step) {
                    const uint32_t mid = (lo + hi) >> 1;
                    const uint32_t s_mid = (uint32_t)__shfl((int)start, (int)mid, 64);
                    if (s_mid <= i) lo = mid;
                    else hi = mid;
                }
                const uint32_t k = i - (uint32_t)__shfl((int)start, (int)lo, 64);
                const uint32_t o_w = (uint32_t)__shfl((int)w, (int)lo, 64), o_bx0 = (uint32_t)__shfl((int)bx0, (int)lo, 64);
                const uint32_t o_by0 = (uint32_t)__shfl((int)by0, (int)lo, 64);
                owner_t[u] = (uint32_t)__shfl((int)t, (int)lo, 64);
                if (act[u]) {
                    const uint32_t bin = (o_by0 + k / o_w) * P.tiles_x + (o_bx0 + k % o_w);
                    slot[u] = atomicAdd(&P.bin_cursor[bin], 1u);
                    cb[u] = P.chunk_base[bin / RXR_SCAN_CHUNK];
                    bo[u] = P.bin_offset[bin];
                }
            }
        }
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) {
            const uint32_t pos = cb[u] + bo[u] + slot[u];
            if (act[u] && pos < P.list_capacity) P.bin_list[pos] = owner_t[u];
        }
    }
}

// =================================================================================================
// k_blockscan: the bin lists of a mid-sized scene in one launch (rxr_device.h RXR_BLOCKSCAN_*).  One workgroup per block of
// 4 x 4 bins.  Phase 1: the four waves walk ALL triangles' pixel boxes (8 bytes each, dense array written by k_setup3d), 64 per
// step, turn each into its bin range (bin_range: the same function the general pipeline's k_fill enumerates) and keep the ones
// whose range meets the block -- id and packed range -- in LDS (one LDS atomic per wave and step).  Phase 2: every wave takes
// four of the block's bins and deals the kept triangles into the bin's slots with ballot + popcount.  It leaves what k_scan /
// k_fill leave: bin_count, bin_offset (+ a zero chunk base) and the list entries -- in an order that does not matter (the
// visibility pass is an arg-min).  No global atomic, no scan, no second pass over the triangles; large triangles need no list
// of their own (every block sees every triangle).
// =================================================================================================
extern "C" __global__ void __launch_bounds__(256) k_blockscan(RasterParams P) {
    __shared__ uint32_t kept_id[RXR_BLOCKSCAN_BLOCK_TRIS];
    __shared__ uint8_t kept_rng[RXR_BLOCKSCAN_BLOCK_TRIS];  // the bin range clipped to the block, two bits per bound: x0 | x1 << 2 | y0 << 4 | y1 << 6
    __shared__ uint32_t kept_n;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t blocks_x = (P.tiles_x + 3u) / 4u;
    const uint32_t bbx = blockIdx.x % blocks_x, bby = blockIdx.x / blocks_x;
    const uint32_t x_lo = bbx * 4u, x_hi = min(x_lo + 3u, P.tiles_x - 1u), y_lo = bby * 4u, y_hi = min(y_lo + 3u, P.tiles_y - 1u);
    __shared__ uint32_t grp[RXR_BLOCKSCAN_BLOCK_GROUPS];
    __shared__ uint32_t grp_n;
    if (tid == 0) kept_n = grp_n = 0u;
    __syncthreads();
    const unsigned long long below = (1ull << lane) - 1ull;
    // phase 0: the groups (256 consecutive triangles, k_setup3d's workgroups) whose union of bin ranges meets this block
    const uint32_t n_groups = (P.n_tris3d + RXR_BLOCKSCAN_GROUP - 1u) / RXR_BLOCKSCAN_GROUP;
    if (P.blockscan_scatter) {  // uniform: the groups have listed themselves (k_setup3d); the count goes back zeroed
        const uint32_t cnt = P.blk_cnt[blockIdx.x];
        if (tid < min(cnt, (uint32_t)RXR_BLOCKSCAN_BLOCK_GROUPS)) grp[tid] = P.blk_grp[(size_t)blockIdx.x * RXR_BLOCKSCAN_BLOCK_GROUPS + tid];
        __syncthreads();
        if (tid == 0) {
            grp_n = cnt;
            if (cnt) P.blk_cnt[blockIdx.x] = 0u;
        }
        __syncthreads();
        const uint32_t n_wide = P.counters[CNT_TICKET];
        for (uint32_t w0 = 0; w0 < n_wide; w0 += 256u) {  // uniform trip count
            bool hit = false;
            uint32_t g = 0;
            if (w0 + tid < n_wide) {
                g = P.blk_grp[P.blk_wide_base + w0 + tid];
                const uint2 r = P.group_rng[g];
                hit = (r.x & 0xFFFFu) <= x_hi && (r.x >> 16) >= x_lo && (r.y & 0xFFFFu) <= y_hi && (r.y >> 16) >= y_lo;
            }
            const unsigned long long m = __ballot(hit);
            if (m) {  // wave-uniform
                uint32_t base = 0;
                if (lane == 0) base = atomicAdd(&grp_n, (uint32_t)__popcll(m));
                base = (uint32_t)__shfl((int)base, 0, 64);
                const uint32_t pos = base + (uint32_t)__popcll(m & below);
                if (hit && pos < RXR_BLOCKSCAN_BLOCK_GROUPS) grp[pos] = g;
            }
        }
        if (blockIdx.x == 0 && tid < CNT_WORDS) P.counters_next[tid] = 0u;  // (the set of the previous launch, as k_scan does)
    } else
    for (uint32_t g0 = 0; g0 < n_groups; g0 += 256u) {  // uniform trip count
        const uint32_t g = g0 + tid;
        bool hit = false;
        if (g < n_groups) {
            const uint2 r = P.group_rng[g];
            hit = (r.x & 0xFFFFu) <= x_hi && (r.x >> 16) >= x_lo && (r.y & 0xFFFFu) <= y_hi && (r.y >> 16) >= y_lo;  // (an empty group: first bin 65535)
        }
        const unsigned long long m = __ballot(hit);
        if (m) {  // wave-uniform
            uint32_t base = 0;
            if (lane == 0) base = atomicAdd(&grp_n, (uint32_t)__popcll(m));
            base = (uint32_t)__shfl((int)base, 0, 64);
            const uint32_t pos = base + (uint32_t)__popcll(m & below);
            if (hit && pos < RXR_BLOCKSCAN_BLOCK_GROUPS) grp[pos] = g;
        }
    }
    __syncthreads();
    const uint32_t n_grp_all = grp_n;
    const uint32_t n_grp = min(n_grp_all, (uint32_t)RXR_BLOCKSCAN_BLOCK_GROUPS);
    // phase 1: those groups' triangles whose own range meets the block (a group per wave and step)
    for (uint32_t gi0 = 0; gi0 < n_grp; gi0 += 4u) {  // uniform trip count
        const uint32_t gi = gi0 + wave;
        const uint32_t t = gi < n_grp ? grp[gi] * RXR_BLOCKSCAN_GROUP + lane : 0xFFFFFFFFu;
        bool hit = false;
        uint32_t rng = 0u;
        if (t < P.n_tris3d) {
            const uint2 box = P.tri_box[t];
            uint32_t bx0, bx1, l0, l1;
            if (bin_range(P, box.x & 0xFFFFu, box.x >> 16, box.y & 0xFFFFu, box.y >> 16, bx0, bx1, l0, l1)) {
                hit = bx0 <= x_hi && bx1 >= x_lo && l0 <= y_hi && l1 >= y_lo;
                rng = (max(bx0, x_lo) - x_lo) | ((min(bx1, x_hi) - x_lo) << 2) | ((max(l0, y_lo) - y_lo) << 4) | ((min(l1, y_hi) - y_lo) << 6);
            }
        }
        const unsigned long long m = __ballot(hit);
        if (m) {  // wave-uniform
            uint32_t base = 0;
            if (lane == 0) base = atomicAdd(&kept_n, (uint32_t)__popcll(m));
            base = (uint32_t)__shfl((int)base, 0, 64);
            const uint32_t pos = base + (uint32_t)__popcll(m & below);
            if (hit && pos < RXR_BLOCKSCAN_BLOCK_TRIS) {
                kept_id[pos] = t;
                kept_rng[pos] = (uint8_t)rng;
            }
        }
    }
    __syncthreads();
    const uint32_t n_kept_all = kept_n;
    const uint32_t n_kept = min(n_kept_all, (uint32_t)RXR_BLOCKSCAN_BLOCK_TRIS);
    bool overflow = n_kept_all > RXR_BLOCKSCAN_BLOCK_TRIS || n_grp_all > RXR_BLOCKSCAN_BLOCK_GROUPS;
    uint32_t worst = 0;
    for (uint32_t j = wave; j < 16u; j += 4u) {
        const uint32_t bx = x_lo + (j & 3u), by = y_lo + (j >> 2);
        if (bx > x_hi || by > y_hi) continue;  // wave-uniform
        const uint32_t bin = by * P.tiles_x + bx;
        const uint32_t first = bin * P.blockscan_cap;
        uint32_t cnt = 0;
        for (uint32_t k0 = 0; k0 < n_kept; k0 += 64u) {
            const uint32_t k = k0 + lane;
            bool in = false;
            uint32_t id = 0;
            if (k < n_kept) {
                const uint32_t r = kept_rng[k];
                in = (j & 3u) >= (r & 3u) && (j & 3u) <= ((r >> 2) & 3u) && (j >> 2) >= ((r >> 4) & 3u) && (j >> 2) <= (r >> 6);
                id = kept_id[k];
            }
            const unsigned long long m = __ballot(in);
            const uint32_t pos = cnt + (uint32_t)__popcll(m & below);
            if (in && pos < P.blockscan_cap && first + pos < P.list_capacity) P.bin_list[first + pos] = id;
            cnt += (uint32_t)__popcll(m);
        }
        if (cnt > P.blockscan_cap) overflow = true;
        worst = max(worst, cnt);
        if (lane == 0) {
            P.bin_count[bin] = min(cnt, P.blockscan_cap);
            P.bin_offset[bin] = first;  // (chunk bases are zero in this mode)
            if (bin % RXR_SCAN_CHUNK == 0u) P.chunk_base[bin / RXR_SCAN_CHUNK] = 0u;
        }
    }
    if (overflow && lane == 0) P.host_status[CNT_OVERFLOW] = 1u;  // sticky; rxr_synchronize renders the frame again through the general pipeline
    (void)worst;
}

// =================================================================================================
// 2D binning (only when the frame has more than RXR_STAGE_TRIS 2D primitives): count / fill of the
// primitives' pixel boxes, same scheme as the 3D bins; the lists are sorted per tile in k_raster.
// =================================================================================================
namespace {
__device__ __forceinline__ bool prim2d_box_bins(const RasterParams &P, uint2 box, uint32_t &bx0, uint32_t &bx1, uint32_t &l0, uint32_t &l1);
__device__ __forceinline__ bool prim2d_bins(const RasterParams &P, const Prim2D &R, uint32_t &bx0, uint32_t &bx1, uint32_t &l0, uint32_t &l1) {
    return prim2d_box_bins(P, make_uint2(R.bx, R.by), bx0, bx1, l0, l1);
}
// (the same from the primitive's packed pixel box alone)
__device__ __forceinline__ bool prim2d_box_bins(const RasterParams &P, uint2 box, uint32_t &bx0, uint32_t &bx1, uint32_t &l0, uint32_t &l1) {
    uint32_t min_x = box.x & 0xFFFFu, max_x = box.x >> 16, min_y = box.y & 0xFFFFu, max_y = box.y >> 16;
    // clamp the box to the rows of this launch (bands / stripes)
    if (min_y < P.row0) min_y = P.row0;
    if (max_y > P.row1) max_y = P.row1;
    return bin_range(P, min_x, max_x, min_y, max_y, bx0, bx1, l0, l1);
}
}  // namespace

// k_blockscan2d: the 2D bin lists without atomics, a scan or a second pass, and IN SUBMISSION ORDER -- what the ordered blending of
// d2_rasterize needs (rasterizer.rs:876-895) and what the general pipeline restores with a bitonic sort in every tile.  One workgroup
// per block of 4 x 4 bins walks all primitives in index order, 256 per step; the step's hits get consecutive places in LDS (wave
// counts through LDS, ballot + popcount inside a wave), so the kept list -- and every bin's list dealt from it -- is sorted.
// Leaves bin2d_count / bin2d_offset (+ a zero chunk base) like k_scan / k_bin2d_fill; overflow of the block (RXR_BLOCKSCAN_BLOCK_TRIS)
// or of a bin's slots raises the 2D overflow word and the frame is rendered again through the general pipeline.
extern "C" __global__ void __launch_bounds__(256) k_blockscan2d(RasterParams P) {
    __shared__ uint32_t kept_id[RXR_BLOCKSCAN_BLOCK_TRIS];
    __shared__ uint8_t kept_rng[RXR_BLOCKSCAN_BLOCK_TRIS];  // bin range clipped to the block: x0 | x1 << 2 | y0 << 4 | y1 << 6
    __shared__ uint32_t wave_cnt[4];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t blocks_x = (P.tiles_x + 3u) / 4u;
    const uint32_t bbx = blockIdx.x % blocks_x, bby = blockIdx.x / blocks_x;
    const uint32_t x_lo = bbx * 4u, x_hi = min(x_lo + 3u, P.tiles_x - 1u), y_lo = bby * 4u, y_hi = min(y_lo + 3u, P.tiles_y - 1u);
    const unsigned long long below = (1ull << lane) - 1ull;
    uint32_t running = 0;  // uniform: primitives kept so far
    // (a step's pixel box is requested one step ahead: the two barriers of a step would otherwise expose every load's latency)
    uint2 box_next = tid < P.n_prims2d ? *reinterpret_cast<const uint2 *>(&P.prim2d[tid].bx) : make_uint2(0u, 0u);
    for (uint32_t t0 = 0; t0 < P.n_prims2d; t0 += 256u) {  // uniform trip count
        const uint32_t t = t0 + tid;
        const uint2 box = box_next;
        if (t + 256u < P.n_prims2d) box_next = *reinterpret_cast<const uint2 *>(&P.prim2d[t + 256u].bx);
        bool hit = false;
        uint32_t rng = 0u;
        if (t < P.n_prims2d) {
            uint32_t bx0, bx1, l0, l1;
            if (prim2d_box_bins(P, box, bx0, bx1, l0, l1)) {
                hit = bx0 <= x_hi && bx1 >= x_lo && l0 <= y_hi && l1 >= y_lo;
                rng = (max(bx0, x_lo) - x_lo) | ((min(bx1, x_hi) - x_lo) << 2) | ((max(l0, y_lo) - y_lo) << 4) | ((min(l1, y_hi) - y_lo) << 6);
            }
        }
        const unsigned long long m = __ballot(hit);
        if (lane == 0) wave_cnt[wave] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t off = running, total = 0;
#pragma unroll
        for (uint32_t w = 0; w < 4u; ++w) {
            const uint32_t c = wave_cnt[w];
            if (w < wave) off += c;
            total += c;
        }
        const uint32_t pos = off + (uint32_t)__popcll(m & below);
        if (hit && pos < RXR_BLOCKSCAN_BLOCK_TRIS) {
            kept_id[pos] = t;
            kept_rng[pos] = (uint8_t)rng;
        }
        running += total;
        __syncthreads();  // (wave_cnt is rewritten by the next step; the last one publishes the kept list)
    }
    const uint32_t n_kept = min(running, (uint32_t)RXR_BLOCKSCAN_BLOCK_TRIS);
    bool overflow = running > RXR_BLOCKSCAN_BLOCK_TRIS;
    for (uint32_t j = wave; j < 16u; j += 4u) {
        const uint32_t bx = x_lo + (j & 3u), by = y_lo + (j >> 2);
        if (bx > x_hi || by > y_hi) continue;  // wave-uniform
        const uint32_t bin = by * P.tiles_x + bx;
        const uint32_t first = bin * P.blockscan2d_cap;
        uint32_t cnt = 0;
        for (uint32_t k0 = 0; k0 < n_kept; k0 += 64u) {
            const uint32_t k = k0 + lane;
            bool in = false;
            uint32_t id = 0;
            if (k < n_kept) {
                const uint32_t r = kept_rng[k];
                in = (j & 3u) >= (r & 3u) && (j & 3u) <= ((r >> 2) & 3u) && (j >> 2) >= ((r >> 4) & 3u) && (j >> 2) <= (r >> 6);
                id = kept_id[k];
            }
            const unsigned long long m = __ballot(in);
            const uint32_t pos = cnt + (uint32_t)__popcll(m & below);
            if (in && pos < P.blockscan2d_cap && first + pos < P.list2d_capacity) P.bin2d_list[first + pos] = id;
            cnt += (uint32_t)__popcll(m);
        }
        if (cnt > P.blockscan2d_cap) overflow = true;
        if (lane == 0) {
            P.bin2d_count[bin] = min(cnt, P.blockscan2d_cap);
            P.bin2d_offset[bin] = first;
            if (bin % RXR_SCAN_CHUNK == 0u) P.chunk2d_base[bin / RXR_SCAN_CHUNK] = 0u;
        }
    }
    if (overflow && lane == 0) P.host_status2d[CNT_OVERFLOW] = 1u;
}

extern "C" __global__ void __launch_bounds__(256) k_bin2d_count(RasterParams P) {
    uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= P.n_prims2d) return;
    uint32_t bx0, bx1, by0, by1;
    if (!prim2d_bins(P, P.prim2d[t], bx0, bx1, by0, by1)) return;
    uint32_t nb = (bx1 - bx0 + 1) * (by1 - by0 + 1);
    if (nb > RXR_LARGE_BINS) {
        uint32_t slot = atomicAdd(&P.counters2d[CNT_LARGE], 1u);
        if (slot < P.n_prims2d) P.large2d_list[slot] = t;
    } else {
        for (uint32_t by = by0; by <= by1; ++by)
            for (uint32_t bx = bx0; bx <= bx1; ++bx) atomicAdd(&P.bin2d_count[by * P.tiles_x + bx], 1u);
    }
}

extern "C" __global__ void __launch_bounds__(256) k_bin2d_fill(RasterParams P) {
    uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= P.n_prims2d) return;
    uint32_t bx0, bx1, by0, by1;
    if (!prim2d_bins(P, P.prim2d[t], bx0, bx1, by0, by1)) return;
    uint32_t nb = (bx1 - bx0 + 1) * (by1 - by0 + 1);
    if (nb > RXR_LARGE_BINS) return;
    for (uint32_t by = by0; by <= by1; ++by)
        for (uint32_t bx = bx0; bx <= bx1; ++bx) {
            uint32_t bin = by * P.tiles_x + bx;
            uint32_t pos = P.chunk2d_base[bin / RXR_SCAN_CHUNK] + P.bin2d_offset[bin] + atomicAdd(&P.bin2d_cursor[bin], 1u);
            if (pos < P.list2d_capacity) P.bin2d_list[pos] = t;
        }
}

#endif  // !RXR_JIT
// =================================================================================================
// k_raster: the tile kernel.  One workgroup per 16x16 tile, one pixel per lane.
// Replaces the rayon tile closure, rasterizer.rs:275-556, and the tile->framebuffer copy, :559-579.
// =================================================================================================
namespace {

struct Vis {
    float zmin;
    int best;        // global triangle id of the winner, -1 = none
    float alpha, beta;
    uint32_t slot;   // staged slot of the winner (fused small-scene path: its TriShade lives in LDS)
    uint32_t batch;  // batch of the winner
    // opacity pass, levels with the chunk paths only: the "staircase" of prefix minima.  surface_id (rasterizer.rs:1682) is read by the
    // opaque batches of chunk k when only the opacity batches of chunks <= k have run (:314-357), so a candidate with
    // submission index t must see the opacity winner among fragments with index < t.  A fragment is a prefix minimum iff
    // no fragment with a smaller index has z <= its z; the set is kept here (index ascending = z descending).  Of one
    // batch's prefix minima only the last one (largest index) can ever be the answer for a candidate of ANOTHER batch, and it
    // dominates whatever the others dominate, so each batch holds at most one of the 3 slots.
    float fz[3];
    int fid[3];
    int fprof[3];    // profile id of the fragment's batch, -1 for None
    int fbatch[3];
};

__device__ __forceinline__ void front_init(Vis &v) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        v.fz[i] = 0.0f;
        v.fid[i] = -1;
        v.fprof[i] = -1;
        v.fbatch[i] = -1;
    }
}
// inserts fragment (z, id, prof) arriving in arbitrary order.  `batch` is the fragment's opacity GROUP (DevBatch.flags >> 16,
// rxr_upload_frame): a maximal run of opacity batches in submission order with no profiled opaque batch between them.  Only
// opaque candidates with a profile id ever look the staircase up, and none of them has an index inside a group's index range --
// so, exactly as for the prefix minima of one batch, of a group's prefix minima only the last one can be an answer.
__device__ __forceinline__ void front_insert(Vis &v, float z, int id, int prof, int batch, uint32_t *overflow_flag) {
    if (!(z < 1.0f)) return;  // z_buffer_opacity starts at 1.0 (:283): never written
    bool dominated = false;
#pragma unroll
    for (int i = 0; i < 3; ++i)
        if (v.fid[i] >= 0 && v.fid[i] < id && v.fz[i] <= z) dominated = true;
    if (dominated) return;
#pragma unroll
    for (int i = 0; i < 3; ++i)
        if (v.fid[i] >= 0 && id < v.fid[i] && z <= v.fz[i]) v.fid[i] = -1;  // no longer a prefix minimum
    // same group already present: both are prefix minima, keep the later one (its batch may differ: the profile goes with it)
    bool done = false;
#pragma unroll
    for (int i = 0; i < 3; ++i)
        if (v.fid[i] >= 0 && v.fbatch[i] == batch) {
            if (id > v.fid[i]) {
                v.fz[i] = z;
                v.fid[i] = id;
                v.fprof[i] = prof;
            }
            done = true;
        }
    if (done) return;
    // take a free slot; if all three are taken drop the entry with the smallest index (only happens when four or more
    // opacity GROUPS nest as prefix minima in one pixel).  The drop is reported: rxr_synchronize returns RXR_ERR_UNSUPPORTED
    // for the frame (pinned host word; the store is this rare path's only cost)
    int slot = v.fid[0] < 0 ? 0 : (v.fid[1] < 0 ? 1 : (v.fid[2] < 0 ? 2 : -1));
    if (slot < 0) {
        *overflow_flag = 1u;
        slot = (v.fid[0] < v.fid[1]) ? (v.fid[0] < v.fid[2] ? 0 : 2) : (v.fid[1] < v.fid[2] ? 1 : 2);
        // (selects, not v.fid[slot]: a run-time index would put the whole staircase -- and with it the opacity winner that every
        // pixel reads in the resolve step -- into scratch memory)
        const int fid_slot = slot == 0 ? v.fid[0] : (slot == 1 ? v.fid[1] : v.fid[2]);
        if (id < fid_slot) return;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i)
        if (i == slot) {
            v.fz[i] = z;
            v.fid[i] = id;
            v.fprof[i] = prof;
            v.fbatch[i] = batch;
        }
}
// surface_id as the candidate with submission index t sees it: the prefix minimum with the largest index < t
__device__ __forceinline__ int front_lookup(const Vis &v, int t) {
    int best_id = -1, prof = -1;
#pragma unroll
    for (int i = 0; i < 3; ++i)
        if (v.fid[i] >= 0 && v.fid[i] < t && v.fid[i] > best_id) {
            best_id = v.fid[i];
            prof = v.fprof[i];
        }
    return prof;
}

// barycentric_weights_3d (rasterizer.rs:1754-1773) and the fragment's depth (:1054-1058) for the pixel centre (fx, fy): the three
// correctly rounded divisions of the reference -- alpha and beta by the triangle's `area`, 1 / one_over_z -- through the
// shared-reciprocal sequences of rxr_exact_math.h (the same floats as `/`; a wave with an operand outside the window, e.g. a
// barycentric that is exactly zero, takes the plain operators).  Must be called in wave-uniform-or-divergent control flow
// alike: the window vote counts active lanes only.
// PRE: (pre_acx, pre_acy, pre_r) = (v2x - v0x, v2y - v0y, rxm::denominator_part(area)) -- what the expressions need of the TRIANGLE
// alone -- computed once per candidate of a row-mode round by the thread that prepares it (rows_round) instead of by every pixel
// item: the same operations on the same operands, so the same floats.
template <bool PRE = false>
__device__ __forceinline__ void bary_depth(float v0x, float v0y, float v1x, float v1y, float v2x, float v2y, float area, float iz0, float iz1, float iz2,
                                           float fx, float fy, float &alpha, float &beta, float &z, float pre_acx = 0.0f, float pre_acy = 0.0f,
                                           float pre_r = 0.0f) {
    const float pcx = v2x - fx, pcy = v2y - fy;
    const float pbx = v1x - fx, pby = v1y - fy;
    const float apx = fx - v0x, apy = fy - v0y;
    const float acx = PRE ? pre_acx : v2x - v0x, acy = PRE ? pre_acy : v2y - v0y;
    const float na = pcx * pby - pcy * pbx, nb = acx * apy - acy * apx;
    if constexpr (PRE) rxm::div2_pre(na, nb, area, pre_r, alpha, beta);
    else rxm::div2(na, nb, area, alpha, beta);
    const float gamma = 1.0f - alpha - beta;
    const float one_over_z = iz0 * alpha + iz1 * beta + iz2 * gamma;
    z = rxm::div1_known(1.0f, one_over_z, rxm::in_window(one_over_z));
}

// one candidate triangle against this lane's pixel (rasterizer.rs:1020-1060 + the :1408 alpha rule)
// the encoded alpha of an opaque-pass fragment whose alpha does not follow from (texture, uv) alone -- a program
// that may write `opacity` (:1403-1408), a terrain texel, a baked shader texture: the whole front half of the
// fragment block has to run to know whether the fragment is written at all
template <Level LV>
__device__ __forceinline__ bool fragment_alpha_is_255_body(const RasterParams &P, const TriShade *shade, uint32_t batch, float alpha, float beta,
                                                           float z, float fx, float fy) {
    const TriShade H = *shade;
    Frag F;
    shade3d_begin<feat<LV>.out_of_line>(P, H, batch, alpha, beta, z, fx, fy, F);  // (programs: the interpreter out of line)
    return f32_to_u8_saturated(F.opacity) == 255u;
}
// Vm and VmS keep it out of line (the interpreter's registers).  Chunk inlines it: a real call anywhere in a kernel makes the
// compiler reserve the call ABI's registers and wait for all memory traffic around it -- k_raster_chunk ran the bench
// frame at 329 us against k_raster's 197 us with the SAME instruction count until its only call went away.
template <Level LV>
__device__ __noinline__ bool fragment_alpha_is_255_call(const RasterParams &P, const TriShade *shade, uint32_t batch, float alpha, float beta,
                                                        float z, float fx, float fy) {
    return fragment_alpha_is_255_body<LV>(P, shade, batch, alpha, beta, z, fx, fy);
}
template <Level LV>
__device__ __forceinline__ bool fragment_alpha_is_255_full(const RasterParams &P, const TriShade *shade, uint32_t batch, float alpha, float beta,
                                                           float z, float fx, float fy) {
    if constexpr (!feat<LV>.vis_programs) return fragment_alpha_is_255_body<Level::Chunk>(P, shade, batch, alpha, beta, z, fx, fy);
    else return fragment_alpha_is_255_call<LV>(P, shade, batch, alpha, beta, z, fx, fy);
}

// ASC: the caller walks its candidates in ascending submission index from a fresh Vis, so a tie in z can never go to the candidate
// (the reference's strict `z < z_buffer`, :1060, in submission order); LEAN: the caller recovers the winner's slot and batch from
// vis.best after its walk (scan_implicit: slot == index, the record is still staged) -- two selects fewer per candidate
template <bool OPACITY, Level LV, bool ASC = false, bool LEAN = false>
__device__ __forceinline__ void visit(const RasterParams &P, const TriSetup &S, const TriShade *shade, uint32_t t, uint32_t slot,
                                      uint32_t px, uint32_t py, float fx, float fy, Vis &vis, int surf_profile, const Vis *opf) {
    uint32_t min_x = S.bx & 0xFFFFu, max_x = S.bx >> 16, min_y = S.by & 0xFFFFu, max_y = S.by >> 16;
    bool in = px >= min_x && px < max_x && py >= min_y && py < max_y;
    if (!in) return;  // small triangles: most waves of the tile have no lane inside the box and skip the edge functions
    // Edges::evaluate (edge.rs:28-36): reject iff a*px + b*py + c < 0 (NaN passes)
    float r0 = S.ea[0] * fx + S.eb[0] * fy + S.ec[0];
    float r1 = S.ea[1] * fx + S.eb[1] * fy + S.ec[1];
    float r2 = S.ea[2] * fx + S.eb[2] * fy + S.ec[2];
    in = !(r0 < 0.0f) && !(r1 < 0.0f) && !(r2 < 0.0f);
    if (!in) return;
    const bool is_opacity = (S.bflags & DB_OPACITY_LIST) != 0;
    if (is_opacity != OPACITY) return;
    if (!OPACITY) {
        // surface_id[idx].is_some() && surface_id[idx] == batch.profile_id  (:1044-1048)
        if constexpr (feat<LV>.chunk) {
            if (S.bflags & DB_HAS_PROFILE) {
                const int sp = front_lookup(*opf, (int)t);
                if (sp >= 0 && (uint32_t)sp == S.profile_id) return;
            }
        } else {
            if (surf_profile >= 0 && (S.bflags & DB_HAS_PROFILE) && (uint32_t)surf_profile == S.profile_id) return;
        }
    }
    // barycentric_weights_3d (:1754-1773)
    float alpha, beta, z;
    bary_depth(S.v0x, S.v0y, S.v1x, S.v1y, S.v2x, S.v2y, S.area, S.iz0, S.iz1, S.iz2, fx, fy, alpha, beta, z);
    const float gamma = 1.0f - alpha - beta;
    if constexpr (OPACITY && feat<LV>.chunk) front_insert(vis, z, (int)t, (S.bflags & DB_HAS_PROFILE) ? (int)S.profile_id : -1, (int)(S.bflags >> DB_GROUP_SHIFT), P.staircase_overflow);
    bool take = z < vis.zmin || (!ASC && z == vis.zmin && vis.best >= 0 && (int)t < vis.best);
    if (take) {
        if (feat<LV>.chunk && !OPACITY && (S.bflags & DB_FULL_ALPHA)) {  // frames with such batches run k_raster_chunk / k_raster_vm (KernelLevel)
            take = fragment_alpha_is_255_full<LV>(P, shade, S.batch, alpha, beta, z, fx, fy);
        } else if (!OPACITY && (S.bflags & DB_ALPHA_TEST)) {
            // the fragment is only written when its encoded alpha is 255 (:1408): sample it now
            const TriShade H = *shade;
            float u, v;
            fragment_uv(H, alpha, beta, gamma, u, v);
            uint32_t texel;
            // (the candidate is the same for every lane, and so is its record: the descriptor it carries -- make_setup -- leads straight to
            // the texels; through the batch header and the descriptor table every cut-out candidate of a tile cost two more round trips)
            if (H.pad[1] & TS_DESC_VALID) {
                const DevTexDesc d{H.pad[0], H.pad[1] & 0x1FFFu, (H.pad[1] >> 13) & 0x1FFFu, (H.pad[1] >> 28) & 3u};
                texel = sample_texture(d, texel_base(P, d), u, v, P.sample_mode, (H.pad[1] >> 26) & 3u);
            } else {
                const DevBatch &B = P.batches3d[S.batch];
                texel = batch_texel<LV>(P, B, u, v, 0.0f, 0.0f);  // never a terrain batch: those carry DB_FULL_ALPHA
            }
            take = (texel >> 24) == 255u;
        }
    }
    // branch-free update: see rows_resolve for what hipcc's if-conversion did to the `if (!closer) return; vis.x = ...;` form
    vis.zmin = take ? z : vis.zmin;
    vis.best = take ? (int)t : vis.best;
    vis.alpha = take ? alpha : vis.alpha;
    vis.beta = take ? beta : vis.beta;
    if constexpr (!LEAN) {
        vis.slot = take ? slot : vis.slot;
        vis.batch = take ? S.batch : vis.batch;
    }
}

// visit() for a candidate the tile-level classification has found to be COVERING and PLAIN (tile_inside_edges below; no opacity list,
// profile, cut-out or program-decided alpha): every pixel of the tile is inside its pixel box and passes its three edge functions, and
// none of the per-batch rules applies -- what is left of visit() is the depth of the fragment and the strict compare.  The same
// expressions in the same order: the same floats.
template <bool ASC, bool LEAN>
__device__ __forceinline__ void visit_cover(const TriSetup &S, uint32_t t, uint32_t slot, float fx, float fy, Vis &vis) {
    float alpha, beta, z;
    bary_depth(S.v0x, S.v0y, S.v1x, S.v1y, S.v2x, S.v2y, S.area, S.iz0, S.iz1, S.iz2, fx, fy, alpha, beta, z);
    const bool take = z < vis.zmin || (!ASC && z == vis.zmin && vis.best >= 0 && (int)t < vis.best);
    vis.zmin = take ? z : vis.zmin;
    vis.best = take ? (int)t : vis.best;
    vis.alpha = take ? alpha : vis.alpha;
    vis.beta = take ? beta : vis.beta;
    if constexpr (!LEAN) {
        vis.slot = take ? slot : vis.slot;
        vis.batch = take ? S.batch : vis.batch;
    }
}

// Exact trivial reject of a triangle for a whole tile (rxr_rect_outside_edges, rxr_device.h: the definition, which the host asks of
// whole tile rows -- rxr_tri_tile_rows).  A name for the call, not a function of its own: one more level of inlining between the kernels
// and the shared definition changed the register allocation of thirteen kernels that have nothing else to do with it.
#define tile_outside_edges(ea, eb, ec, tile_x0, tile_y0px) rxr_rect_outside_edges((ea), (eb), (ec), (tile_x0), (tile_y0px), RXR_TILE_W, RXR_TILE_H)

// The converse: Edges::evaluate accepts EVERY pixel centre of the tile.  Over the tile r = (a*x + b*y) + c is smallest at the corner
// that minimises a*x and b*y separately (the same monotonicity); if that corner's r -- the same expression -- is a number >= 0,
// every other pixel's r is a number at least as large, or NaN (an overflowed product meeting an opposite infinity), and `r < 0`
// rejects neither.  A NaN at the corner itself proves nothing: not covering.
__device__ __forceinline__ bool tile_inside_edges(const float *ea, const float *eb, const float *ec, uint32_t tile_x0, uint32_t tile_y0px,
                                                  uint32_t th = RXR_TILE_H) {
    const float x_lo = (float)tile_x0 + 0.5f, x_hi = (float)(tile_x0 + RXR_TILE_W - 1u) + 0.5f;
    const float y_lo = (float)tile_y0px + 0.5f, y_hi = (float)(tile_y0px + th - 1u) + 0.5f;
    bool inside = true;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float xm = ea[i] >= 0.0f ? x_lo : x_hi;
        const float ym = eb[i] >= 0.0f ? y_lo : y_hi;
        const float r = ea[i] * xm + eb[i] * ym + ec[i];
        inside = inside && (r >= 0.0f);
    }
    return inside;
}
#define RXR_COVER_BIT 0x80000000u
// candidate R of the opaque pass, already known to meet the tile: covering and plain (visit_cover)?
__device__ __forceinline__ bool covers_plainly(const TriSetup &R, uint32_t tile_x0, uint32_t tile_y0px) {
    if (R.bflags & (DB_OPACITY_LIST | DB_HAS_PROFILE | DB_ALPHA_TEST | DB_FULL_ALPHA)) return false;
    const uint32_t min_x = R.bx & 0xFFFFu, max_x = R.bx >> 16, min_y = R.by & 0xFFFFu, max_y = R.by >> 16;
    if (!(min_x <= tile_x0 && max_x >= tile_x0 + RXR_TILE_W && min_y <= tile_y0px && max_y >= tile_y0px + RXR_TILE_H)) return false;
    return tile_inside_edges(R.ea, R.eb, R.ec, tile_x0, tile_y0px);
}

// LDS staging area of one workgroup: candidate triangle records of the current round
struct Stage {
    float4 tri[RXR_STAGE_TRIS * 6];  // TriSetup / Prim2D records, 6 x 16 B each
    uint32_t ids[RXR_STAGE_TRIS];
    uint32_t wave_cnt[RXR_TILE_THREADS / 64];
};
// fused small-scene path only: shading records of the staged triangles
struct StageShade {
    TriShade shade[RXR_STAGE_TRIS];
};

// ---- row-parallel visibility (kernel k_raster_rows: binned scenes, Level::Common) -------------------------
// In the walk above every wave tests every candidate against its 64 pixels; with many small triangles (a mesh, the
// 1 M-triangle box grid: ~20 candidates per tile, each covering ~20 of 256 pixels) more than nine lanes in ten do
// nothing useful.  Row mode turns the loop inside out for such rounds: the work items are the ROWS of the candidates'
// pixel boxes clipped to the tile; item i belongs to the thread i (mod 256), which walks the row's pixels, evaluates
// exactly the expressions of visit() and merges the fragment into a per-tile z-buffer in LDS with one 64-bit atomic
// minimum on the key (z, submission index).  The reference's rule -- the fragment with the smallest z wins, ties go to
// the smaller index (see the file header) -- IS the minimum of that key, so the order in which fragments arrive does
// not matter.  After the last round every pixel's lane reads its key back and re-derives the barycentrics of the
// winner from its record (same expressions, same floats).
template <uint32_t TH>
struct RowLdsT {
    unsigned long long key[RXR_TILE_W * TH];   // TH = 32: the pair kernels' two tiles on top of each other (raster_tile_pair)
    uint32_t row_start[RXR_STAGE_TRIS + 1];  // exclusive prefix of the staged candidates' row counts
    uint32_t red[8];                         // per-wave totals: [0..3] rows | area << 12, [4..7] candidates with rows
    uint32_t raw[RXR_STAGE_TRIS];            // scan_lists_rows: triangle id of every list entry of the round (= of every staged record)
    uint8_t slot[RXR_STAGE_TRIS];            // scan_lists_rows: staged record of candidate k (bytes: 8 workgroups per CU must fit in 160 KB)
    uint8_t chunk_owner[RXR_TILE_THREADS];   // rows_round: first owner of every 64-item chunk of the round's pixel items
    uint32_t cut[4];                         // rows_round<.., SPLIT>: the round's candidates that the caller has to walk (cut-outs, profiled ones), a bit per candidate
};
using RowLds = RowLdsT<RXR_TILE_H>;
// order-preserving map of non-NaN floats to unsigned integers
__device__ __forceinline__ uint32_t z_order_bits(float z) {
    const uint32_t b = __float_as_uint(z);
    return b ^ ((b & 0x80000000u) ? 0xFFFFFFFFu : 0x80000000u);
}
// z_buffer starts at 1.0 and only `z < 1.0` is ever written (:1060): no key at or above this one is a hit
#define RXR_ZKEY_INIT (0xBF800000ull << 32)
// A round goes to the pixel-parallel walk when its candidates' clipped boxes average more than this many pixels (a whole tile is 256: at 256
// no round of candidates without cut-outs does).  128 until the end of round 4, chosen when row mode still ran every box pixel through
// bary_depth; with the fragment compaction row mode also wins on LARGE triangles -- A-B-A-B 128 against 256: the teapot 25.2 -> 24.6 us,
// the reduced box grid 43.8 -> 41.5, the lattice seen from among its boxes (tools/run_configs.py near:0.8 / 2 / 4) 71.8 -> 68.4 / 66.5 ->
// 62.8 / 55.9 -> 52.4, the 1 M-triangle grid unchanged; 64: 475-487 us there against 411-425 (profiles/r04/row_mode_area_threshold_abab.txt)
#ifndef RXR_ROW_MODE_MAX_AREA
#define RXR_ROW_MODE_MAX_AREA 256
#endif
// Fragment compaction (north-star: "wavefront ballot/prefix-sum for fragment compaction").  A candidate covers a third of its
// clipped pixel box on the 1 M-triangle grid (measured on the scene: 34 candidates, 1 880 box pixels and 700 fragments per non-empty
// tile), so with Edges::evaluate and the depth arithmetic in one pass two lanes in three sit out bary_depth -- two exact quotients, a
// reciprocal and the ds_min_u64 -- and every box pixel pays the owner search and the decode of its item.  With the compaction
//   (a) an item is a run of up to FOUR pixels of one row of a candidate's clipped box: one owner search, one decode and one fetch of the
//       edge coefficients per run, and b*y per run instead of per pixel (the same products: the same floats);
//   (b) the items only evaluate the edge functions.  The survivors of each of the four pixel slots are counted with one ballot and take
//       consecutive places (mbcnt prefix) in a ring of 32-bit entries (staged record, x, y, z-buffer cell) that belongs to the WAVE:
//       no atomic, no barrier, the ring's head and fill are wave-uniform;
//   (c) whenever 64 entries are queued the wave runs barycentric_weights_3d, the depth and the ds_min_u64 on them with all lanes (the
//       remainder goes last, once per round).
// The same expressions per fragment, and the arg-min is order-independent: exact by construction.  The rings alias the 2D pass's sort
// buffer, idle during the 3D passes: no LDS is added.  First tried with one-pixel items, a queue shared by the workgroup, an LDS add
// per wave and pass and a barrier in front of the drain: 4 % fewer VALU instructions and 1.5 % SLOWER (profiles/r04).
#define RXR_ROWS_RING 128u  // entries per wave: fewer than 64 left over + at most 64 from one pixel slot
static_assert(RXR_ROWS_RING * 4u * (RXR_TILE_THREADS / 64) <= RXR_SORT2D_MAX * 4u, "the four rings live in the 2D pass's sort buffer");

// One round of row mode over the `n` records staged in st (ids in st.ids).  Returns false (uniformly) without having
// done anything when the round is better served by the pixel-parallel walk.
//
// Pixel items (PIX): the work items are the PIXELS of the candidates' clipped boxes, not their rows.  With a row
// per thread every wave runs its x loop as often as its widest row needs (a tile of the 1 M-triangle grid: ~95 rows of 1..16
// pixels in two of the four waves, the other two idle) -- most lanes wait most of the time.  With a pixel per thread the
// ~380 box pixels of such a tile are two passes of all four waves, each lane evaluating exactly the expressions of visit()
// once.  The owner of item i is found without a search per lane: the prefix sums of the box areas are in LDS, every
// 64-item chunk looks its first owner up once (a parallel binary search, one chunk per thread) and a lane steps forward
// from there (runs of one candidate are ~20 items long).
// INDIRECT: candidate k's record is st.tri[rl.slot[k] * 6] (scan_lists_rows) instead of st.tri[k * 6]
// PIX: pixel items (above); false = one item per row with an x loop, which the interpreter kernels with programs in their visibility
// loop keep (LevelFeatures.pixel_items).  The others take pixel items WITH the compaction since the end of round 4: pixel items alone had
// cost k_raster_vm_sv 3-4 % on the 1 M-triangle grid in round 3 (its register budget is spent on the interpreter); as 4-pixel runs with
// the per-wave rings they save k_raster_vm_p 7 % and k_raster_vm_sv 6 % (scan_lists_rows)
// SPLIT: a round that holds candidates row mode cannot take -- cut-outs, whose fragments need a texel (:1408); candidates with a profile id
// in a frame with an opacity pass (:1044-1048) -- still runs in row mode for all the others; the ones left over are named in rl.cut and
// the caller walks them (scan_lists_rows).  Without SPLIT such a round is refused as a whole (returns false), as until the end of round
// 4 everywhere: two batches with a fence texture among the 96 of the reduced box grid made its raster kernel 2.4 times slower, one in
// eight 3.2 times.
// Returns 0 (refused), 1 (done) or -- SPLIT only -- 2 (done, and rl.cut names candidates that are left to walk).
template <bool INDIRECT, bool PIX, uint32_t TH = RXR_TILE_H, bool COMPACT = false, bool SPLIT = false>
__device__ __forceinline__ uint32_t rows_round(const RasterParams &P, Stage &st, RowLdsT<TH> &rl, uint32_t n, uint32_t tile_x0, uint32_t tile_y0px,
                                               uint32_t *queue = nullptr) {
    static_assert(TH == 16 || TH == 32, "the bit fields of `geo` and the exact short division hold for offsets below 512");
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    // clipped pixel box of staged candidate `tid`
    uint32_t rows = 0, area = 0, geo = 0, items = 0;  // items: COMPACT's runs of up to four pixels
    bool alpha_test = false;
    if (tid < n) {
        const TriSetup &R = *reinterpret_cast<const TriSetup *>(&st.tri[(INDIRECT ? rl.slot[tid] : tid) * 6u]);
        // (a candidate with a profile id in a frame with an opacity pass: its fragments are skipped where the opacity layer carries the same id
        // -- a per-pixel question the drain does not ask; such rounds are left to the walk as well)
        alpha_test = (R.bflags & (DB_ALPHA_TEST | DB_FULL_ALPHA)) != 0 || (P.has_opacity && (R.bflags & DB_HAS_PROFILE));
        if (!(R.bflags & DB_OPACITY_LIST)) {
            const uint32_t x0 = max(R.bx & 0xFFFFu, tile_x0), x1 = min(R.bx >> 16, tile_x0 + RXR_TILE_W);
            const uint32_t y0 = max(R.by & 0xFFFFu, tile_y0px), y1 = min(R.by >> 16, tile_y0px + TH);
            // (SPLIT with the compaction: a plain cut-out -- its fragments need a texel's alpha and nothing else -- stays a row candidate, marked
            // in bit 31 of `geo`: the drain samples for the fragments that would win their pixel.  Half of the reduced box grid's batches
            // fenced: 141 us with every such candidate walked by every pixel)
            const bool cut_in_rows = SPLIT && COMPACT && (R.bflags & DB_ALPHA_TEST) && !(R.bflags & DB_FULL_ALPHA) && !(P.has_opacity && (R.bflags & DB_HAS_PROFILE));
            if (SPLIT && alpha_test && !cut_in_rows) {
                alpha_test = x0 < x1 && y0 < y1;   // (left over for the caller's walk -- if its box meets the tile at all; no row items)
            } else if (x0 < x1 && y0 < y1) {
                if (cut_in_rows) alpha_test = false;
                rows = y1 - y0;
                area = rows * (x1 - x0);
                // decode data of the pixel items: box origin inside the tile, width, and ceil(8192 / width): for offsets
                // below 512 and widths up to 16, (offset * that) >> 13 == offset / width exactly (checked for every pair)
                const uint32_t w = x1 - x0;
                if constexpr (COMPACT) {
                    // (runs per row 1..4, then ceil(8192 / runs) for the same exact short division)
                    const uint32_t segs = (w + 3u) >> 2;
                    items = rows * segs;
                    geo = (x0 - tile_x0) | ((y0 - tile_y0px) << 4) | (w << 9) | (segs << 14) | (((8192u + segs - 1u) / segs) << 17) | (cut_in_rows ? 0x80000000u : 0u);
                } else {
                    geo = (x0 - tile_x0) | ((y0 - tile_y0px) << 4) | (w << 9) | (((8192u + w - 1u) / w) << 14);
                }
                static_assert(RXR_TILE_W == 16 && RXR_TILE_H <= 32, "bit fields of `geo`");
            } else if (cut_in_rows) {
                alpha_test = false;   // (its box misses the tile: nothing to do anywhere)
            }
        } else if (SPLIT) {
            alpha_test = false;   // (a candidate of the opacity lists: nothing for the opaque pass, neither in rows nor in the walk)
        }
    }
    // inclusive scan over the workgroup of the areas (each <= 256, at most 128 candidates: below 2^15), or of
    // (rows | area << 13): rows total <= 2^12, area total <= 2^16
    // (COMPACT: items | area << 14: at most 128 * 64 items, the areas decide between row mode and the walk as before)
    const uint32_t packed = COMPACT ? (items | (area << 14)) : PIX ? area : (rows | (area << 13));
    uint32_t inc = packed;
    if (wave * 64u < n) inc = rxm::wave_inclusive_add(packed);  // (wave-uniform: the waves behind the last candidate have nothing to add)
    const unsigned long long has = __ballot(rows != 0u);
    // cut-out candidates need a texel per fragment (:1408): such rounds are left to the walk, which keeps the sampling code
    // (and its registers) out of the row loop
    const unsigned long long cutout = SPLIT ? __ballot(alpha_test && tid < n) : __ballot(rows != 0u && alpha_test);
    if (lane == 63u) {
        rl.red[wave] = inc;
        rl.red[4u + wave] = (cutout ? 0x10000u : 0u) + ((!SPLIT && cutout) ? 0u : (uint32_t)__popcll(has));  // (bit 16 and up: waves with such candidates)
        if constexpr (SPLIT) {
            if (wave < 2u) {
                rl.cut[2u * wave] = (uint32_t)cutout;
                rl.cut[2u * wave + 1u] = (uint32_t)(cutout >> 32);
            }
        }
    }
    __syncthreads();
    uint32_t before = 0, total = 0, cands = 0;
#pragma unroll
    for (uint32_t w = 0; w < RXR_TILE_THREADS / 64; ++w) {
        const uint32_t v = rl.red[w];
        if (w < wave) before += v;
        total += v;
        cands += rl.red[4u + w];
    }
    const uint32_t rows_total = PIX ? 0u : (total & 0x1FFFu), area_total = COMPACT ? (total >> 14) : PIX ? total : (total >> 13);
    const uint32_t n_items = COMPACT ? (total & 0x3FFFu) : area_total;  // work items of the round
    const bool leftovers = SPLIT && cands >= 0x10000u;
    if constexpr (SPLIT) cands &= 0xFFFFu;
    if (cands == 0u || cands >= 0x10000u || area_total > cands * (uint32_t)RXR_ROW_MODE_MAX_AREA) {
        __syncthreads();  // rl.red is rewritten by the next round
        return 0u;
    }
    if constexpr (PIX) {
    if (tid < n) {
        const uint32_t mine = COMPACT ? items : area;
        const uint32_t start = (COMPACT ? ((before + inc) & 0x3FFFu) : before + inc) - mine;  // exclusive prefix of the item counts
        // (the addresses below are functions of the thread index alone: left to itself the compiler computes them once in front of the
        // loop over the rounds and, at 64 registers, SPILLS them -- two scratch dwords per thread, 93 MB of HBM writes per 8K frame
        // in the counters.  An index it cannot see through is recomputed per round: two instructions each.)
        uint32_t tl = tid;
        if constexpr (COMPACT) asm volatile("" : "+v"(tl));
        rl.row_start[tl] = start;
        rl.raw[tl] = geo;                            // (the list entries' ids have moved to st.ids by now)
        // The round is row mode from here on: nothing reads the staged record's pixel box and flags again, and their words take what
        // bary_depth needs of the triangle alone (its PRE form) -- once per candidate instead of once per pixel item.
        if (area) {
            TriSetup &W = *reinterpret_cast<TriSetup *>(&st.tri[(INDIRECT ? rl.slot[tl] : tl) * 6u]);
            const float acx = W.v2x - W.v0x, acy = W.v2y - W.v0y, r = rxm::denominator_part(W.area);
            W.bx = __float_as_uint(acx);
            W.by = __float_as_uint(acy);
            W.bflags = __float_as_uint(r);
            if constexpr (COMPACT) W.profile_id = st.ids[tl];  // (row mode never reads the profile: no candidate of the round has one that matters) the queue names records
        }
        // first owner of every 64-item chunk (area_total <= 128 * 128: at most 256 chunks): item 64 c belongs to the one candidate
        // WITH pixels whose range [start, start + area) holds it -- that candidate knows, so it writes the chunk's entry itself
        // (usually none or one: ~20 items per candidate) instead of a binary search over the prefix by one thread per chunk behind
        // another barrier.  Candidates without pixels in front of it share its start; the item loop steps over them as before.
        for (uint32_t c = (start + 63u) >> 6; (c << 6) < start + mine; ++c) rl.chunk_owner[c] = (uint8_t)tl;
    }
    if (tid == 0) rl.row_start[n] = n_items;
    __syncthreads();
    if constexpr (COMPACT) {
    // (the drain reads the PRE operands and the triangle id from the staged record)
    uint32_t *const ring = queue + wave * RXR_ROWS_RING;
    uint32_t head = 0, fill = 0;  // wave-uniform
    // (c) entries [head, head + m) of this wave's ring on lanes 0 .. m-1: barycentric_weights_3d, the depth and the merge, as visit()
    // (two diagnostic builds -- this drain without its z-buffer traffic, and no drain at all -- located the kernel's LDS bank conflicts
    // here: profiles/r04/lds_conflict_sources_c5.txt)
    auto drain = [&](uint32_t m) {
        if (lane < m) {
            const uint32_t e = ring[(head + lane) & (RXR_ROWS_RING - 1u)];
            // words 8 .. 23 of the staged record as four 16-byte reads (ds_read_b128: 64 banks, 16 lanes per LDS cycle -- the lanes of a drain
            // hold fragments of several records 24 dwords apart; read field by field (ds_read2_b32, 32 banks) records 4 slots apart collide)
            const float4 *const rec = &st.tri[(e & 0xFFu) * 6u];
            const float4 q2 = rec[2], q3 = rec[3], q4 = rec[4], q5 = rec[5];
            // q2 = (ec2, v0x, v0y, v1x)  q3 = (v1y, v2x, v2y, area)  q4 = (iz0, iz1, iz2, batch)  q5 = (PRE acx, PRE acy, PRE r, triangle id)
            static_assert(__builtin_offsetof(TriSetup, v0x) == 36 && __builtin_offsetof(TriSetup, area) == 60 && __builtin_offsetof(TriSetup, iz0) == 64 &&
                          __builtin_offsetof(TriSetup, bx) == 80 && __builtin_offsetof(TriSetup, profile_id) == 92, "the drain's view of a staged record");
            const float fx = (float)((e >> 8) & (SPLIT ? 0x7Fu : 0xFFu)) + ((float)tile_x0 + 0.5f), fy = (float)((e >> 16) & 0xFFu) + ((float)tile_y0px + 0.5f);  // (exact sums: the item's own fx, fy)
            float alpha, beta, z;
            bary_depth<true>(q2.y, q2.z, q2.w, q3.x, q3.y, q3.z, q3.w, q4.x, q4.y, q4.z, fx, fy, alpha, beta, z, q5.x, q5.y, q5.z);
            if (z < 1.0f) {  // never closer than the cleared buffer; also NaN
                const unsigned long long key = ((unsigned long long)z_order_bits(z + 0.0f) << 32) | __float_as_uint(q5.w);  // -0 -> +0: they compare equal
                unsigned long long *const cell = &rl.key[TH == 16 ? (e >> 24) : ((e >> 16) & 0xFFu) * RXR_TILE_W + ((e >> 8) & (SPLIT ? 0x7Fu : 0xFFu))];
                // (cells only ever decrease: a stale value is merely conservative.  A relaxed workgroup-scope atomic load, so that the
                // read is an LDS instruction)
                bool wins = key < __hip_atomic_load(cell, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                if constexpr (SPLIT) {
                    // a cut-out candidate's fragment is only written when its texel's alpha is 255 (:1408): visit()'s test, for the fragments
                    // that would take their pixel (the same expressions: fragment_uv of the same barycentrics, the same sampler)
                    if (wins && (e & 0x8000u)) {
                        const TriShade H = P.tri_shade[__float_as_uint(q5.w)];
                        float u, v;
                        fragment_uv(H, alpha, beta, 1.0f - alpha - beta, u, v);
                        uint32_t texel;
                        if (H.pad[1] & TS_DESC_VALID) {
                            const DevTexDesc d{H.pad[0], H.pad[1] & 0x1FFFu, (H.pad[1] >> 13) & 0x1FFFu, (H.pad[1] >> 28) & 3u};
                            texel = sample_texture(d, texel_base(P, d), u, v, P.sample_mode, (H.pad[1] >> 26) & 3u);
                        } else {
                            texel = batch_texel<Level::Common>(P, P.batches3d[__float_as_uint(q4.w)], u, v, 0.0f, 0.0f);
                        }
                        wins = (texel >> 24) == 255u;
                    }
                }
                if (wins) atomicMin(cell, key);
            }
        }
    };
    for (uint32_t base = wave * 64u; base < n_items; base += RXR_TILE_THREADS) {  // (wave-uniform bounds: every lane is at the ballots)
        const uint32_t item = base + lane;
        uint32_t entry = 0, valid = 0;
        float fx = 0.0f, a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, t0 = 0.0f, t1 = 0.0f, t2 = 0.0f, c0 = 0.0f, c1 = 0.0f, c2 = 0.0f;
        if (item < n_items) {
            uint32_t k = rl.chunk_owner[item >> 6];
            while (rl.row_start[k + 1u] <= item) ++k;  // candidates without pixels share their successor's start; row_start[n] = n_items > item
            const uint32_t g = rl.raw[k];
            const uint32_t local = item - rl.row_start[k], segs = (g >> 14) & 7u;
            const uint32_t ry = (local * ((g >> 17) & 0x3FFFu)) >> 13, sx = local - ry * segs;
            const uint32_t lx = (g & 15u) + 4u * sx, ly = ((g >> 4) & 31u) + ry;
            valid = min(((g >> 9) & 31u) - 4u * sx, 4u);
            const uint32_t sl = INDIRECT ? (uint32_t)rl.slot[k] : k;
            const TriSetup &S = *reinterpret_cast<const TriSetup *>(&st.tri[sl * 6u]);
            fx = (float)(tile_x0 + lx) + 0.5f;
            const float fy = (float)(tile_y0px + ly) + 0.5f;
            a0 = S.ea[0]; a1 = S.ea[1]; a2 = S.ea[2];
            t0 = S.eb[0] * fy; t1 = S.eb[1] * fy; t2 = S.eb[2] * fy;
            c0 = S.ec[0]; c1 = S.ec[1]; c2 = S.ec[2];
            entry = sl | (lx << 8) | (ly << 16) | ((ly * RXR_TILE_W + lx) << 24) | (SPLIT ? ((g >> 31) << 15) : 0u);   // (bit 15: a cut-out candidate's item)
            static_assert(RXR_STAGE_TRIS <= 256 && RXR_TILE_W == 16 && TH <= 32, "bit fields of a ring entry");
        }
        // (the four pixel slots as straight-line code -- five copies of the drain -- were tried and retired)
#pragma unroll 1
        for (uint32_t px = 0; px < 4u; ++px) {
            // Edges::evaluate (edge.rs:28-36)
            const float r0 = a0 * fx + t0 + c0;
            const float r1 = a1 * fx + t1 + c1;
            const float r2 = a2 * fx + t2 + c2;
            const bool pass = px < valid && !((r0 < 0.0f) || (r1 < 0.0f) || (r2 < 0.0f));
            const unsigned long long m = __ballot(pass);
            if (m != 0ull) {  // (wave-uniform)
                const uint32_t at = head + fill + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                if (pass) ring[at & (RXR_ROWS_RING - 1u)] = entry;
                fill += (uint32_t)__popcll(m);
                if (fill >= 64u) {
                    __builtin_amdgcn_wave_barrier();  // (LDS instructions of one wave complete in order: the entries are there)
                    drain(64u);
                    head += 64u;
                    fill -= 64u;
                }
            }
            fx += 1.0f;               // (exact: the next pixel centre)
            entry += 0x01000100u;     // x + 1, cell + 1
        }
    }
    if (fill) {
        __builtin_amdgcn_wave_barrier();
        drain(fill);
    }
    } else {
    for (uint32_t base = 0; base < area_total; base += RXR_TILE_THREADS) {
        const uint32_t item = base + tid;
        if (item >= area_total) break;  // (no barrier inside the loop)
        uint32_t k = rl.chunk_owner[item >> 6];
        while (rl.row_start[k + 1u] <= item) ++k;  // candidates without pixels share their successor's start; row_start[n] = area_total > item
        const uint32_t g = rl.raw[k];
        const uint32_t local = item - rl.row_start[k];
        const uint32_t ry = (local * (g >> 14)) >> 13, rx = local - ry * ((g >> 9) & 31u);
        const uint32_t lx = (g & 15u) + rx, ly = ((g >> 4) & 31u) + ry;
        const TriSetup &S = *reinterpret_cast<const TriSetup *>(&st.tri[(INDIRECT ? rl.slot[k] : k) * 6u]);
        const uint32_t t = st.ids[k];
        const float fx = (float)(tile_x0 + lx) + 0.5f, fy = (float)(tile_y0px + ly) + 0.5f;
        // Edges::evaluate (edge.rs:28-36)
        const float r0 = S.ea[0] * fx + S.eb[0] * fy + S.ec[0];
        const float r1 = S.ea[1] * fx + S.eb[1] * fy + S.ec[1];
        const float r2 = S.ea[2] * fx + S.eb[2] * fy + S.ec[2];
        if ((r0 < 0.0f) || (r1 < 0.0f) || (r2 < 0.0f)) continue;
        // barycentric_weights_3d and depth, as visit()
        float alpha, beta, z;
        bary_depth<true>(S.v0x, S.v0y, S.v1x, S.v1y, S.v2x, S.v2y, S.area, S.iz0, S.iz1, S.iz2, fx, fy, alpha, beta, z, __uint_as_float(S.bx),
                         __uint_as_float(S.by), __uint_as_float(S.bflags));
        if (!(z < 1.0f)) continue;  // never closer than the cleared buffer; also NaN
        const unsigned long long key = ((unsigned long long)z_order_bits(z + 0.0f) << 32) | t;  // -0 -> +0: they compare equal
        unsigned long long *const cell = &rl.key[ly * RXR_TILE_W + lx];
        // (cells only ever decrease: a stale value is merely conservative.  A relaxed workgroup-scope atomic load, so that the read
        // is an LDS instruction -- a `volatile` read through the generic pointer became a FLAT load with a wait for ALL memory traffic)
        if (key >= __hip_atomic_load(cell, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) continue;
        atomicMin(cell, key);
    }
    }
    } else {
    if (tid < n) rl.row_start[tid] = ((before + inc) & 0x1FFFu) - rows;
    if (tid == 0) rl.row_start[n] = rows_total;
    __syncthreads();

    for (uint32_t item = tid; item < rows_total; item += RXR_TILE_THREADS) {
        // candidate of this row: the largest k with row_start[k] <= item (candidates without rows share their successor's start)
        uint32_t lo = 0, hi = n;
        while (hi - lo > 1u) {
            const uint32_t mid = (lo + hi) >> 1;
            if (rl.row_start[mid] <= item) lo = mid;
            else hi = mid;
        }
        const TriSetup &S = *reinterpret_cast<const TriSetup *>(&st.tri[(INDIRECT ? rl.slot[lo] : lo) * 6u]);
        const uint32_t t = st.ids[lo];
        const uint32_t x0 = max(S.bx & 0xFFFFu, tile_x0), x1 = min(S.bx >> 16, tile_x0 + RXR_TILE_W);
        const uint32_t y = max(S.by & 0xFFFFu, tile_y0px) + (item - rl.row_start[lo]);
        const float fy = (float)y + 0.5f;
        const float ea0 = S.ea[0], ea1 = S.ea[1], ea2 = S.ea[2], ec0 = S.ec[0], ec1 = S.ec[1], ec2 = S.ec[2];
        const float by0 = S.eb[0] * fy, by1 = S.eb[1] * fy, by2 = S.eb[2] * fy;
        const float v0x = S.v0x, v0y = S.v0y, v1x = S.v1x, v1y = S.v1y, v2x = S.v2x, v2y = S.v2y;
        const float area_t = S.area, iz0 = S.iz0, iz1 = S.iz1, iz2 = S.iz2;
        unsigned long long *const zrow = &rl.key[(y - tile_y0px) * RXR_TILE_W];
        for (uint32_t x = x0; x < x1; ++x) {
            const float fx = (float)x + 0.5f;
            // Edges::evaluate (edge.rs:28-36)
            const float r0 = ea0 * fx + by0 + ec0;
            const float r1 = ea1 * fx + by1 + ec1;
            const float r2 = ea2 * fx + by2 + ec2;
            if ((r0 < 0.0f) || (r1 < 0.0f) || (r2 < 0.0f)) continue;
            // barycentric_weights_3d and depth, as visit()
            const float pcx = v2x - fx, pcy = v2y - fy;
            const float pbx = v1x - fx, pby = v1y - fy;
            const float apx = fx - v0x, apy = fy - v0y;
            const float acx = v2x - v0x, acy = v2y - v0y;
            const float alpha = (pcx * pby - pcy * pbx) / area_t;
            const float beta = (acx * apy - acy * apx) / area_t;
            const float gamma = 1.0f - alpha - beta;
            const float one_over_z = iz0 * alpha + iz1 * beta + iz2 * gamma;
            const float z = 1.0f / one_over_z;
            if (!(z < 1.0f)) continue;  // never closer than the cleared buffer; also NaN
            const unsigned long long key = ((unsigned long long)z_order_bits(z + 0.0f) << 32) | t;  // -0 -> +0: they compare equal
            unsigned long long *const cell = &zrow[x - tile_x0];
            if (key >= *(volatile unsigned long long *)cell) continue;  // (cells only ever decrease: a stale value is merely conservative)
            atomicMin(cell, key);
        }
    }
    }
    __syncthreads();  // the stage and rl are reused by the next round
    return leftovers ? 2u : 1u;
}

// after the last round: this lane's pixel takes the z-buffer's winner if it beats what the pixel-parallel rounds found
// (the winner's shading record is fetched together with its set-up record: one memory latency instead of two)
__device__ __forceinline__ void rows_resolve(const RasterParams &P, const RowLds &rl, uint32_t lx, uint32_t ly, float fx, float fy, Vis &vis,
                                                TriShade &shade, int &shade_of) {
    const unsigned long long key = rl.key[ly * RXR_TILE_W + lx];
    if (key >= RXR_ZKEY_INIT) return;
    const uint32_t t = (uint32_t)key;
    const TriSetup S = P.tri_setup[t];
    shade = P.tri_shade[t];
    shade_of = (int)t;
    float alpha, beta, z;
    bary_depth(S.v0x, S.v0y, S.v1x, S.v1y, S.v2x, S.v2y, S.area, S.iz0, S.iz1, S.iz2, fx, fy, alpha, beta, z);
    const bool closer = z < vis.zmin || (z == vis.zmin && vis.best >= 0 && (int)t < vis.best);
    // Branch-free update.  Written as `if (!closer) return; vis.x = ...;` hipcc (ROCm 7.2) kept the OLD vis.batch for the lanes
    // that win an exact tie (z == vis.zmin, smaller index): its if-conversion restored the old value for every lane of the
    // `!(z < zmin)` region before merging (seen in the ISA; tests/test_gpu_rows.py "mixed" caught it as a wrong texture on
    // duplicated geometry).  The selects below leave it nothing to merge.
    vis.zmin = closer ? z : vis.zmin;
    vis.best = closer ? (int)t : vis.best;
    vis.alpha = closer ? alpha : vis.alpha;
    vis.beta = closer ? beta : vis.beta;
    vis.slot = closer ? 0u : vis.slot;
    vis.batch = closer ? S.batch : vis.batch;
}

// Visibility pass over the tile's candidate triangles = [large-triangle list, filtered against the
// tile rectangle] ++ [this tile's bin list].  Per round of RXR_STAGE_TRIS list entries:
//   1. the first RXR_STAGE_TRIS threads fetch one entry each (large entries also fetch their pixel
//      box and test it against the tile),
//   2. survivors are compacted with a wave ballot + popcount prefix sum (+ a 4-entry cross-wave sum),
//   3. all 256 threads copy the survivors' 96-byte TriSetup records into LDS with coalesced 16-byte
//      loads,
//   4. every lane walks the staged records (uniform LDS addresses -> broadcast reads).
template <bool OPACITY, Level LV>
__device__ __forceinline__ void scan_lists(const RasterParams &P, Stage &st, uint32_t b0, uint32_t b1, uint32_t tile_x0,
                                           uint32_t tile_y0px, uint32_t px, uint32_t py, float fx, float fy, Vis &vis,
                                           int surf_profile, const Vis *opf, RowLds *rl = nullptr) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t n_large = min(P.counters[CNT_LARGE], P.n_tris3d);
    const uint32_t total = n_large + (b1 - b0);
    const float4 *g4 = reinterpret_cast<const float4 *>(P.tri_setup);
    for (uint32_t base = 0; base < total; base += RXR_STAGE_TRIS) {
        // 1. fetch + test
        uint32_t id = 0;
        bool keep = false;
        const uint32_t e = base + tid;
        if (tid < RXR_STAGE_TRIS && e < total) {
            if (e < n_large) {
                id = min(P.large_list[e], P.n_tris3d - 1u);
                const uint2 box = *reinterpret_cast<const uint2 *>(&P.tri_setup[id].bx);
                uint32_t min_x = box.x & 0xFFFFu, max_x = box.x >> 16, min_y = box.y & 0xFFFFu, max_y = box.y >> 16;
                keep = !(min_x >= tile_x0 + RXR_TILE_W || max_x <= tile_x0 || min_y >= tile_y0px + RXR_TILE_H || max_y <= tile_y0px);
            } else {
                id = P.bin_list[b0 + (e - n_large)];
                keep = true;
            }
            // defensive: never follow an id outside this frame's triangle records
            if (id >= P.n_tris3d) {
                keep = false;
                id = 0;
            }
            if (keep) {
                const TriSetup &R = P.tri_setup[id];
                // (the opacity pass only ever takes candidates of the opacity lists -- visit() -- : the others need not be staged and walked
                // by every pixel to find that out)
                if (OPACITY && !(R.bflags & DB_OPACITY_LIST)) keep = false;
                else if (tile_outside_edges(R.ea, R.eb, R.ec, tile_x0, tile_y0px)) keep = false;
            }
        }
        // 2. compaction
        const unsigned long long m = __ballot(keep);
        const uint32_t before = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) st.wave_cnt[wave] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t off = 0, n = 0;
#pragma unroll
        for (uint32_t w = 0; w < RXR_TILE_THREADS / 64; ++w) {
            uint32_t c = st.wave_cnt[w];
            if (w < wave) off += c;
            n += c;
        }
        if (keep) st.ids[off + before] = id;
        __syncthreads();
        // 3. stage the records
        for (uint32_t f = tid; f < n * 6u; f += RXR_TILE_THREADS) {
            uint32_t k = f / 6u, j = f - k * 6u;
            st.tri[f] = g4[(size_t)st.ids[k] * 6u + j];
        }
        __syncthreads();
        // 4. walk (or, for rounds of small triangles, the rows of their boxes: rows_round)
        if constexpr (!OPACITY && !feat<LV>.chunk && !feat<LV>.programs) {
            if (rl != nullptr && rows_round<false, true>(P, st, *rl, n, tile_x0, tile_y0px)) continue;
        }
        for (uint32_t k = 0; k < n; ++k) {
            const TriSetup &S = *reinterpret_cast<const TriSetup *>(&st.tri[k * 6u]);
            const uint32_t t = st.ids[k];
            visit<OPACITY, LV>(P, S, &P.tri_shade[t], t, k, px, py, fx, fy, vis, surf_profile, opf);
        }
        __syncthreads();  // the stage is reused by the next round
    }
}

// scan_lists for k_raster_rows (opaque pass, Level::Common).  Binned scenes of small triangles are bound by the chain of
// dependent memory latencies per tile, not by arithmetic, so this variant stages FIRST and tests afterwards: the records
// of all list entries of the round go to LDS as soon as their ids are known, the tile-level reject runs on the LDS copies
// and compacts slot numbers instead of moving records -- one global round trip fewer than scan_lists (which reads the
// edges from HBM for the reject and the records again for staging).  The round is then handed to rows_round or walked.
// SPLITR (k_raster_rows_cut*: frames with cut-out or profiled batches, RasterParams.split_rounds): rounds run in row mode around the
// candidates row mode cannot take (rows_round SPLIT) instead of being walked as a whole.  A variant of its own, not a branch: compiled into
// the plain kernels the few extra lines cost the 1 M-triangle grid 2-9 % through register allocation alone (profiles/r04/HISTORY).
template <Level LV, bool SPLITR = false>
__device__ __forceinline__ void scan_lists_rows(const RasterParams &P, Stage &st, RowLds &rl, bool row_mode, uint32_t b0, uint32_t b1,
                                                uint32_t tile_x0, uint32_t tile_y0px, uint32_t px, uint32_t py, float fx, float fy, Vis &vis,
                                                int surf_profile, const Vis *opf, uint32_t *queue PHASE_PARAM) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t n_large = min(P.counters[CNT_LARGE], P.n_tris3d);
    const uint32_t total = n_large + (b1 - b0);
    const float4 *g4 = reinterpret_cast<const float4 *>(P.tri_setup);
    for (uint32_t base = 0; base < total; base += RXR_STAGE_TRIS) {
        const uint32_t m = min(total - base, (uint32_t)RXR_STAGE_TRIS);
        // 1. ids of the round's list entries
        if (tid < m) {
            const uint32_t e = base + tid;
            rl.raw[tid] = e < n_large ? P.large_list[e] : P.bin_list[b0 + (e - n_large)];
        }
        __syncthreads();
        // 2. their records (ids outside this frame's records are never followed: clamped here, dropped in step 3)
        for (uint32_t f = tid; f < m * 6u; f += RXR_TILE_THREADS) {
            const uint32_t k = f / 6u, j = f - k * 6u;
            st.tri[f] = g4[(size_t)min(rl.raw[k], P.n_tris3d - 1u) * 6u + j];
        }
        __syncthreads();
        // 3. pixel box and tile-level edge reject on the LDS copies; survivors' slots are ballot-compacted
        bool keep = false;
        uint32_t id = 0;
        if (tid < m) {
            id = rl.raw[tid];
            const TriSetup &R = *reinterpret_cast<const TriSetup *>(&st.tri[tid * 6u]);
            const uint32_t min_x = R.bx & 0xFFFFu, max_x = R.bx >> 16, min_y = R.by & 0xFFFFu, max_y = R.by >> 16;
            keep = id < P.n_tris3d && !(min_x >= tile_x0 + RXR_TILE_W || max_x <= tile_x0 || min_y >= tile_y0px + RXR_TILE_H || max_y <= tile_y0px);
            if (keep && tile_outside_edges(R.ea, R.eb, R.ec, tile_x0, tile_y0px)) keep = false;
        }
        const unsigned long long mk = __ballot(keep);
        const uint32_t before = (uint32_t)__popcll(mk & ((1ull << lane) - 1ull));
        if (lane == 0) st.wave_cnt[wave] = (uint32_t)__popcll(mk);
        __syncthreads();
        uint32_t off = 0, n = 0;
#pragma unroll
        for (uint32_t w = 0; w < RXR_TILE_THREADS / 64; ++w) {
            const uint32_t c = st.wave_cnt[w];
            if (w < wave) off += c;
            n += c;
        }
        if (keep) {
            rl.slot[off + before] = (uint8_t)tid;
            st.ids[off + before] = id;
        }
        __syncthreads();
        // 4. the rows of the candidates' boxes, or the walk
        PHASE_MARK(1);
        constexpr bool pixel_items = feat<LV>.pixel_items;  // (false: row items until the end of round 4, rows_round PIX)
        if constexpr (SPLITR) {
            // the candidates every pixel walks: all of the round when row mode refuses it (0), else the ones row mode left over (2: cut-outs;
            // profiled ones under an opacity pass -- rows_round SPLIT wrote their bits in front of its barriers; their records are untouched)
            unsigned long long walk_lo = n >= 64u ? ~0ull : ((1ull << n) - 1ull), walk_hi = n > 64u ? (n >= 128u ? ~0ull : ((1ull << (n - 64u)) - 1ull)) : 0ull;
            const uint32_t rows_ret = row_mode ? rows_round<true, pixel_items, RXR_TILE_H, pixel_items, pixel_items>(P, st, rl, n, tile_x0, tile_y0px, queue) : 0u;
            if (rows_ret) {
                walk_lo = walk_hi = 0ull;
                if (pixel_items && rows_ret == 2u) {  // (uniform)
                    const uint32_t c0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)rl.cut[0]), c1 = (uint32_t)__builtin_amdgcn_readfirstlane((int)rl.cut[1]);
                    const uint32_t c2 = (uint32_t)__builtin_amdgcn_readfirstlane((int)rl.cut[2]), c3 = (uint32_t)__builtin_amdgcn_readfirstlane((int)rl.cut[3]);
                    walk_lo = (unsigned long long)c0 | ((unsigned long long)c1 << 32);
                    walk_hi = (unsigned long long)c2 | ((unsigned long long)c3 << 32);
                }
                PHASE_MARK(7);
            }
            if (walk_lo | walk_hi) {  // (uniform over the workgroup)
                for (uint32_t h = 0; h < 2u; ++h) {
                    for (unsigned long long m = h ? walk_hi : walk_lo; m; m &= m - 1ull) {
                        const uint32_t k = h * 64u + (uint32_t)__builtin_ctzll(m);
                        const uint32_t sl = rl.slot[k];
                        const TriSetup &S = *reinterpret_cast<const TriSetup *>(&st.tri[sl * 6u]);
                        const uint32_t t = st.ids[k];
                        visit<false, LV>(P, S, &P.tri_shade[t], t, sl, px, py, fx, fy, vis, surf_profile, opf);
                    }
                }
                __syncthreads();  // the stage is reused by the next round
            } else if (!rows_ret) {
                __syncthreads();
            }
            PHASE_MARK(10);
        } else {
            if (row_mode && rows_round<true, pixel_items, RXR_TILE_H, pixel_items>(P, st, rl, n, tile_x0, tile_y0px, queue)) {
                PHASE_MARK(7);
                continue;
            }
            for (uint32_t k = 0; k < n; ++k) {
                const uint32_t sl = rl.slot[k];
                const TriSetup &S = *reinterpret_cast<const TriSetup *>(&st.tri[sl * 6u]);
                const uint32_t t = st.ids[k];
                visit<false, LV>(P, S, &P.tri_shade[t], t, sl, px, py, fx, fy, vis, surf_profile, opf);
            }
            __syncthreads();  // the stage is reused by the next round
            PHASE_MARK(10);
        }
    }
}


// Small-scene mode 2 ("implicit list": the whole frame has <= RXR_STAGE_TRIS triangles and k_setup3d has
// written their records): no lists at all.  All records are copied to LDS with one round of coalesced
// loads, THEN thread t tests record t against the tile from LDS and the survivors' indices are
// ballot-compacted -- one global-memory latency per tile instead of three dependent ones.
template <bool OPACITY, Level LV>
__device__ __forceinline__ void scan_implicit(const RasterParams &P, Stage &st, uint32_t tile_x0, uint32_t tile_y0px, uint32_t px, uint32_t py,
                                              float fx, float fy, Vis &vis, int surf_profile, const Vis *opf, uint32_t *win_flags = nullptr) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t n_all = min(P.n_tris3d, (uint32_t)RXR_STAGE_TRIS);
    const float4 *g4 = reinterpret_cast<const float4 *>(P.tri_setup);
    for (uint32_t f = tid; f < n_all * 6u; f += RXR_TILE_THREADS) st.tri[f] = g4[f];
    __syncthreads();
    bool keep = false;
    if (tid < n_all) {
        const TriSetup &R = *reinterpret_cast<const TriSetup *>(&st.tri[tid * 6u]);
        uint32_t min_x = R.bx & 0xFFFFu, max_x = R.bx >> 16, min_y = R.by & 0xFFFFu, max_y = R.by >> 16;
        keep = !(min_x >= tile_x0 + RXR_TILE_W || max_x <= tile_x0 || min_y >= tile_y0px + RXR_TILE_H || max_y <= tile_y0px);
        if (keep && tile_outside_edges(R.ea, R.eb, R.ec, tile_x0, tile_y0px)) keep = false;
    }
    const unsigned long long m = __ballot(keep);
    const uint32_t before = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) st.wave_cnt[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t off = 0, n = 0;
#pragma unroll
    for (uint32_t w = 0; w < RXR_TILE_THREADS / 64; ++w) {
        uint32_t c = st.wave_cnt[w];
        if (w < wave) off += c;
        n += c;
    }
    // (the survivors keep their order: the walk below is in ascending submission index)
    bool cover = false;
    if constexpr (!OPACITY) {
        if (keep) cover = covers_plainly(*reinterpret_cast<const TriSetup *>(&st.tri[tid * 6u]), tile_x0, tile_y0px);
    }
    if (keep) st.ids[off + before] = tid | (cover ? RXR_COVER_BIT : 0u);
    __syncthreads();
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t e = (uint32_t)__builtin_amdgcn_readfirstlane((int)st.ids[k]);  // (uniform: branches and addresses on the scalar unit)
        const uint32_t t = e & ~RXR_COVER_BIT;
        const TriSetup &S = *reinterpret_cast<const TriSetup *>(&st.tri[t * 6u]);
        if (e & RXR_COVER_BIT) visit_cover<true, true>(S, t, t, fx, fy, vis);
        else visit<OPACITY, LV, true, true>(P, S, &P.tri_shade[t], t, t, px, py, fx, fy, vis, surf_profile, opf);
    }
    // (LEAN: slot == index in this path, and the winner's record is still staged)
    vis.slot = (uint32_t)max(vis.best, 0);
    vis.batch = reinterpret_cast<const TriSetup *>(&st.tri[vis.slot * 6u])->batch;
    // (the record carries a copy of its batch's flags: the shading phase need not fetch them from the header)
    if (win_flags) *win_flags = reinterpret_cast<const TriSetup *>(&st.tri[vis.slot * 6u])->bflags;
    __syncthreads();  // the stage is reused (second pass, 2D pass)
}

// Fused small-scene path (P.fused_small: the whole frame has <= RXR_STAGE_TRIS triangles, so one
// staging round holds them all): no k_setup3d / k_scan / k_fill launches and no records in HBM --
// thread t builds triangle t's TriSetup / TriShade itself (make_setup), tests its pixel box against
// the tile, survivors are ballot-compacted straight into LDS, then every lane walks them.
template <bool OPACITY, Level LV>
__device__ __forceinline__ void scan_fused(const RasterParams &P, Stage &st, StageShade &sh, uint32_t tile_x0, uint32_t tile_y0px, uint32_t px,
                                           uint32_t py, float fx, float fy, Vis &vis, int surf_profile, const Vis *opf) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    bool keep = false;
    TriSetup S;
    TriShade H;
    if (tid < RXR_STAGE_TRIS && tid < P.n_tris3d) {
        if (make_setup(P, tid, S, H)) {
            uint32_t min_x = S.bx & 0xFFFFu, max_x = S.bx >> 16, min_y = S.by & 0xFFFFu, max_y = S.by >> 16;
            keep = !(min_x >= tile_x0 + RXR_TILE_W || max_x <= tile_x0 || min_y >= tile_y0px + RXR_TILE_H || max_y <= tile_y0px);
            if (keep && tile_outside_edges(S.ea, S.eb, S.ec, tile_x0, tile_y0px)) keep = false;
        }
    }
    const unsigned long long m = __ballot(keep);
    const uint32_t before = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) st.wave_cnt[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t off = 0, n = 0;
#pragma unroll
    for (uint32_t w = 0; w < RXR_TILE_THREADS / 64; ++w) {
        uint32_t c = st.wave_cnt[w];
        if (w < wave) off += c;
        n += c;
    }
    if (keep) {
        const uint32_t slot = off + before;
        st.ids[slot] = tid;
        *reinterpret_cast<TriSetup *>(&st.tri[slot * 6u]) = S;
        sh.shade[slot] = H;
    }
    __syncthreads();
    for (uint32_t k = 0; k < n; ++k) {
        const TriSetup &SK = *reinterpret_cast<const TriSetup *>(&st.tri[k * 6u]);
        visit<OPACITY, LV>(P, SK, &sh.shade[k], st.ids[k], k, px, py, fx, fy, vis, surf_profile, opf);
    }
    __syncthreads();  // a second pass (opacity, then opaque) rebuilds the stage
}

// Does the Bresenham walk of one segment (rasterizer.rs:1777-1821) plot pixel (px, py)?  Closed form of
// the reference's loop (err = dx - dy; x steps when 2*err > -dy, y steps when 2*err < dx; the end point
// is not plotted): on an x-major segment (dx >= dy) x advances in every iteration, so iteration
// k = |px - x0| is the only one that can plot column px, and the number of y steps taken before it is
// max(0, ceil((2*k*dy - dx) / (2*dx))); y-major segments are the mirror image.  O(1) per pixel instead
// of one walk per tile; verified exhaustively against the sequential walk (tests/test_bresenham_closed_form.py).
__device__ __forceinline__ bool bresenham_hits(const Prim2D &Ln, int px, int py) {
    const long long x0 = __float_as_int(Ln.v0x), y0 = __float_as_int(Ln.v0y), x1 = __float_as_int(Ln.v1x), y1 = __float_as_int(Ln.v1y);
    const long long dx = x1 > x0 ? x1 - x0 : x0 - x1, dy = y1 > y0 ? y1 - y0 : y0 - y1;
    const long long sx = x0 < x1 ? 1 : -1, sy = y0 < y1 ? 1 : -1;
    if (dx >= dy) {
        const long long k = ((long long)px - x0) * sx;
        if (k < 0 || k >= dx) return false;
        const long long a = 2 * k * dy - dx;
        const long long j = a <= 0 ? 0 : (a + 2 * dx - 1) / (2 * dx);
        return (long long)py == y0 + sy * j;
    }
    const long long k = ((long long)py - y0) * sy;
    if (k < 0 || k >= dy) return false;
    const long long a = 2 * k * dx - dy;
    const long long i = a <= 0 ? 0 : (a + 2 * dy - 1) / (2 * dy);
    return (long long)px == x0 + sx * i;
}

// one 2D primitive against this lane's pixel (rasterizer.rs:636-655 coverage, then fragment2d / the line colour)
template <Level LV>
__device__ __forceinline__ uint32_t prim2d_pixel(const RasterParams &P, const Prim2D &T, uint32_t px, uint32_t py, float fx, float fy,
                                                 uint32_t color) {
    const uint32_t min_x = T.bx & 0xFFFFu, max_x = T.bx >> 16, min_y = T.by & 0xFFFFu, max_y = T.by >> 16;
    if (T.batch_kind & 2u) {  // Bresenham segment
        // (the walk never leaves its end-point box -- the box test only matters for a batch clipped to the reference's tiles,
        // rxr_ref_tile_span: then it is smaller)
        if (px >= min_x && px < max_x && py >= min_y && py < max_y && bresenham_hits(T, (int)px, (int)py)) color = __float_as_uint(T.v2x);
        return color;
    }
    bool in = px >= min_x && px < max_x && py >= min_y && py < max_y && (T.batch_kind & 1u);
    float r0 = T.ea[0] * fx + T.eb[0] * fy + T.ec[0];
    float r1 = T.ea[1] * fx + T.eb[1] * fy + T.ec[1];
    float r2 = T.ea[2] * fx + T.eb[2] * fy + T.ec[2];
    in = in && !(r0 < 0.0f) && !(r1 < 0.0f) && !(r2 < 0.0f);
    if (in) {
        // (the primitive is the same for every lane: its batch header comes through the scalar cache, not as a vector load per wave)
        const DevBatch B = uniform_record(P.batches2d, T.batch_kind >> 2);
        color = fragment2d<LV>(P, T, B, px, py, fx, fy, color);
    }
    return color;
}

// stages the Prim2D records of `n` primitive ids (st.ids-like array `ids`, already in submission order)
// through LDS in rounds of RXR_STAGE_TRIS and applies them to this lane's pixel in order
template <Level LV>
__device__ __forceinline__ uint32_t walk_prims2d(const RasterParams &P, Stage &st, const uint32_t *ids, uint32_t n, bool implicit_ids,
                                                 uint32_t px, uint32_t py, float fx, float fy, uint32_t color) {
    const uint32_t tid = threadIdx.x;
    const float4 *g4 = reinterpret_cast<const float4 *>(P.prim2d);
    for (uint32_t base = 0; base < n; base += RXR_STAGE_TRIS) {
        const uint32_t m = min(n - base, (uint32_t)RXR_STAGE_TRIS);
        for (uint32_t f = tid; f < m * 6u; f += RXR_TILE_THREADS) {
            uint32_t k = f / 6u, j = f - k * 6u;
            uint32_t id = implicit_ids ? base + k : ids[base + k];
            st.tri[f] = g4[(size_t)id * 6u + j];
        }
        __syncthreads();
        for (uint32_t k = 0; k < m; ++k) {
            const Prim2D &T = *reinterpret_cast<const Prim2D *>(&st.tri[k * 6u]);
            color = prim2d_pixel<LV>(P, T, px, py, fx, fy, color);
        }
        __syncthreads();
    }
    return color;
}

}  // namespace

// tuning knob: occupancy bound of k_raster
#ifndef RXR_RASTER_WAVES_PER_SIMD
#define RXR_RASTER_WAVES_PER_SIMD 8  // bench frame (4K, 16 lights), built without SLP vectorisation: unbounded (67 VGPRs) 217 us, 7: 211, 8: 210
#endif

// does the union of the 2D primitives' pixel boxes reach this tile?  The box is a launch constant (host-built Prim2D records) or, for
// device-projected 2D batches, four words k_proj2d_prims has left in memory (a uniform load)
__device__ __forceinline__ bool d2_box_meets(const RasterParams &P, uint32_t tile_x0, uint32_t tile_y0px) {
    uint32_t x0, x1, y0, y1;
    if (P.d2_box_dev) {  // uniform
        const uint4 b = *reinterpret_cast<const uint4 *>(P.d2_box_dev);
        x0 = b.x; x1 = b.y; y0 = b.z; y1 = b.w;
    } else {
        x0 = P.d2_box[0]; x1 = P.d2_box[1]; y0 = P.d2_box[2]; y1 = P.d2_box[3];
    }
    return tile_x0 < x1 && tile_x0 + RXR_TILE_W > x0 && tile_y0px < y1 && tile_y0px + RXR_TILE_H > y0;
}

// The 2D pass of one tile (rasterizer.rs:501-553), strictly in submission order; the caller has checked that the union of the 2D
// pixel boxes reaches the tile.  Uses the stage (and s_bin) of the workgroup: every thread of the workgroup must call it.
template <Level LV>
__device__ __forceinline__ uint32_t pass2d(const RasterParams &P, Stage &stage, uint32_t *s_bin, uint32_t *s_sort, const uint32_t sort_cap, uint32_t bin,
                                           uint32_t tile_x0, uint32_t tile_y0px, uint32_t px, uint32_t py, float fx, float fy, uint32_t color) {
    const uint32_t tid = threadIdx.x;
    __syncthreads();  // the 3D pass is done with the stage
    if (!P.binned2d) {
        // few primitives (<= RXR_STAGE_TRIS): thread t tests primitive t's pixel box against the tile, the
        // survivors are ballot-compacted (which keeps submission order) and only they are staged
        const uint32_t lane = tid & 63u, wave = tid >> 6;
        bool keep = false;
        if (tid < P.n_prims2d) {
            const uint2 box = *reinterpret_cast<const uint2 *>(&P.prim2d[tid].bx);
            uint32_t min_x = box.x & 0xFFFFu, max_x = box.x >> 16, min_y = box.y & 0xFFFFu, max_y = box.y >> 16;
            keep = !(min_x >= tile_x0 + RXR_TILE_W || max_x <= tile_x0 || min_y >= tile_y0px + RXR_TILE_H || max_y <= tile_y0px);
        }
        const unsigned long long m = __ballot(keep);
        const uint32_t before = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) stage.wave_cnt[wave] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t off = 0, n = 0;
#pragma unroll
        for (uint32_t w = 0; w < RXR_TILE_THREADS / 64; ++w) {
            uint32_t c = stage.wave_cnt[w];
            if (w < wave) off += c;
            n += c;
        }
        if (keep) stage.ids[off + before] = tid;
        __syncthreads();
        if (n) color = walk_prims2d<LV>(P, stage, stage.ids, n, false, px, py, fx, fy, color);
    } else {
        // candidates = [large 2D primitives whose box touches the tile] ++ [this tile's bin list], gathered
        // into LDS, sorted by primitive index (submission order), then staged and applied in order
        const uint32_t lane = tid & 63u, wave = tid >> 6;
        if (tid == 0) {
            uint32_t cnt = P.bin2d_count[bin];
            uint32_t start = P.chunk2d_base[bin / RXR_SCAN_CHUNK] + P.bin2d_offset[bin];
            s_bin[0] = min(start, P.list2d_capacity);
            s_bin[1] = min(start + cnt, P.list2d_capacity);
            s_bin[2] = 0u;  // number of gathered candidates
            if (cnt) P.bin2d_count[bin] = 0u;
        }
        __syncthreads();
        const uint32_t c0 = s_bin[0], c1 = s_bin[1];
        const uint32_t n_large = P.blockscan2d_cap ? 0u : min(P.counters2d[CNT_LARGE], P.n_prims2d);  // (k_blockscan2d keeps no such list)
        const uint32_t total = n_large + (c1 - c0);
        for (uint32_t base = 0; base < total; base += RXR_TILE_THREADS) {
            const uint32_t e = base + tid;
            uint32_t id = 0;
            bool keep = false;
            if (e < total) {
                if (e < n_large) {
                    id = min(P.large2d_list[e], P.n_prims2d - 1u);
                    const uint2 box = *reinterpret_cast<const uint2 *>(&P.prim2d[id].bx);
                    uint32_t min_x = box.x & 0xFFFFu, max_x = box.x >> 16, min_y = box.y & 0xFFFFu, max_y = box.y >> 16;
                    keep = !(min_x >= tile_x0 + RXR_TILE_W || max_x <= tile_x0 || min_y >= tile_y0px + RXR_TILE_H || max_y <= tile_y0px);
                } else {
                    id = P.bin2d_list[c0 + (e - n_large)];
                    keep = id < P.n_prims2d;
                }
            }
            const unsigned long long m = __ballot(keep);
            const uint32_t before = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            if (lane == 0) stage.wave_cnt[wave] = (uint32_t)__popcll(m);
            __syncthreads();
            uint32_t off = s_bin[2], n = 0;
#pragma unroll
            for (uint32_t w = 0; w < RXR_TILE_THREADS / 64; ++w) {
                uint32_t c = stage.wave_cnt[w];
                if (w < wave) off += c;
                n += c;
            }
            if (keep && off + before < sort_cap) s_sort[off + before] = id;
            __syncthreads();
            if (tid == 0) s_bin[2] = min(s_bin[2] + n, sort_cap + 1u);  // MAX + 1 flags "too many"
            __syncthreads();
        }
        const uint32_t n_cand = s_bin[2];
        if (n_cand > sort_cap) {
            // more candidates than the LDS sort holds: walk every primitive in order (correct, slow)
            color = walk_prims2d<LV>(P, stage, nullptr, P.n_prims2d, true, px, py, fx, fy, color);
        } else if (P.blockscan2d_cap) {
            // k_blockscan2d's lists are in submission order already, and the gather above keeps the order
            color = walk_prims2d<LV>(P, stage, s_sort, n_cand, false, px, py, fx, fy, color);
        } else {
            // bitonic sort of s_sort[0 .. n_cand) padded to the next power of two with 0xFFFFFFFF
            uint32_t n2 = 1;
            while (n2 < n_cand) n2 <<= 1;
            for (uint32_t i2 = n_cand + tid; i2 < n2; i2 += RXR_TILE_THREADS) s_sort[i2] = 0xFFFFFFFFu;
            __syncthreads();
            for (uint32_t k2 = 2; k2 <= n2; k2 <<= 1) {
                for (uint32_t j2 = k2 >> 1; j2 > 0; j2 >>= 1) {
                    for (uint32_t i2 = tid; i2 < n2; i2 += RXR_TILE_THREADS) {
                        uint32_t l2 = i2 ^ j2;
                        if (l2 > i2) {
                            uint32_t a = s_sort[i2], b = s_sort[l2];
                            bool up = (i2 & k2) == 0;
                            if ((a > b) == up) {
                                s_sort[i2] = b;
                                s_sort[l2] = a;
                            }
                        }
                    }
                    __syncthreads();
                }
            }
            color = walk_prims2d<LV>(P, stage, s_sort, n_cand, false, px, py, fx, fy, color);
        }
    }
    return color;
}

// (A retired measurement: N useless full-rate VALU instructions per wave in front of the light loop or in front of the visibility scan.
// A kernel bound by VALU issue pays their issue cycles, one bound by latency does not: profiles/r03/bench_kernel_experiments.txt.)
// LDS of the fused instantiation only
template <bool F>
struct ShadeStore {
    StageShade s;
};
template <>
struct ShadeStore<false> {};

template <bool F>
struct RowStore {
    RowLds r;
};
template <>
struct RowStore<false> {};

// SPANS: the kernel looks RasterParams.row_spans up (sparse frames).  The two common Level::Common kernels of binned scenes exist in both forms
// (k_raster_rows[_rl] / ..._sp): the look-up in front of every tile cost the dense bench frame 0.6 % when every kernel carried it
// (profiles/r04/row_spans_lookup_cost_bench.txt); the small-scene kernels never take spans, the rarer levels always check.
template <bool FUSED, Level LV, bool ROWS = false, bool RL = false, bool SPANS = (feat<LV>.chunk || feat<LV>.programs), bool SPLITR = false>
__device__ __forceinline__ void raster_tile(const RasterParams &P) {
    __shared__ Stage stage;
    __shared__ uint32_t s_bin[4];
    __shared__ ShadeStore<FUSED> shade_store;
    __shared__ RowStore<ROWS> row_store;
    __shared__ uint32_t s_sort[RXR_SORT2D_MAX];  // the gathered candidates of a binned 2D pass; during the 3D passes row mode's fragment queue
    // 2-D grid, no integer division in front of every tile.  Workgroups go to the eight XCDs round robin in launch order
    // (x fastest), and every XCD has its own L2: with column = blockIdx.x, horizontally adjacent tiles -- which share the records
    // of the triangles that straddle them -- always sit on different XCDs.  Tried and retired: handing each XCD groups of G
    // adjacent columns instead (block x stands for column (q / G) * 8G + (x & 7) * G + q % G, q = x / 8; the grid padded to
    // a multiple of 8G columns).  Measured (tools/try_cfg_parity.sh, one box): the 1 M-triangle grid's frame 0.706 ms plain, 0.708 /
    // 0.700 / 0.700 ms with G = 2 / 4 / 8 -- nothing beyond noise, the raster kernels are bound by instruction issue and
    // dependent latencies, not by L2 misses -- while the bench frame loses 1 / 5 / 7 % (neighbouring columns differ in cost, and
    // round robin by single columns is the finest balance there is).  Whole vertical bands per XCD lose far more: grid 561 ->
    // 810 us, bench frame 199 -> 217 us.  Hence the hardware's own round robin.
    // (dispatching the launch's bottom tile rows first, for frames whose expensive tiles are at the bottom, was an A-B variant too: retired)
    uint32_t tx = blockIdx.x;
    const uint32_t ty = blockIdx.y;
    if constexpr (SPANS) {
        if (P.row_spans) {  // (uniform; sparse frames only: see RasterParams.row_spans)
            const uint2 span = uniform_record(P.row_spans, P.tile_y0 + ty);
            tx += span.x;
            if (tx >= span.y) return;  // (the whole workgroup, in front of every barrier)
        }
    }
    const uint32_t bin = (ty + P.bin_row0) * P.tiles_x + tx;
    const uint32_t tid = threadIdx.x;
    const uint32_t tile_x0 = tx * RXR_TILE_W, tile_y0px = (P.tile_y0 + ty * P.tile_stride) * RXR_TILE_H;
    // wave w owns rows 4w .. 4w+3 of the tile (16 x 4 pixels: 64-byte row segments on the store; an 8x8 quadrant per wave was tried and retired)
    const uint32_t lx = tid & (RXR_TILE_W - 1), ly = tid / RXR_TILE_W;
    const uint32_t px = tile_x0 + lx;
    const uint32_t py = tile_y0px + ly;
    const float fx = (float)px + 0.5f, fy = (float)py + 0.5f;  // rasterizer.rs:1022
    const bool in_frame = px < P.width && py >= P.row0 && py < P.row1;
    PHASE_DECL;

    // tile initial colour: zeros | background colour | background shader (rasterizer.rs:277-308)
    // (in 3D mode the resolve loop overwrites every pixel -- hit: shaded colour, miss: [0,0,0,255], :420-461 -- before anything reads
    // the background, so it is not evaluated at all: a division, a clamp and a conversion per lane of every tile)
    uint32_t color = 0u;
    const bool bg_dead = (P.flags & RXR_FLAG_D3_ACTIVE) != 0u;  // uniform
    if (!bg_dead && (P.flags & RXR_FLAG_HAS_BACKGROUND_COLOR)) color = P.background_color;
    if (!bg_dead && !(P.flags & RXR_FLAG_IGNORE_BG_SHADER)) {
        if (P.background_kind == RXR_BG_VGRADIENT) {
            uint32_t i = sat_u8(rclamp(((float)py / P.fheight) * 128.0f, 0.0f, 128.0f));  // shader/vgradient.rs:11-15
            color = pack4(i, i, i, 255u);
        } else if (feat<LV>.chunk && P.background_kind == RXR_BG_GRID) {  // (editor-only: a chunk path, see rxr_upload_frame)
            color = grid_shade(P, px, py);
        } else if (P.background_kind == RXR_BG_HOST_PIXELS && in_frame) {
            color = P.bg_pixels[(size_t)py * P.width + px];
        }
    }

    // Small frames whose records the host made (fused_small 2): the tile rows outside [d3_trow0, d3_trow1) are out of every triangle's
    // reach (rxr_tri_tile_rows, the tile reject below asked of whole rows at upload), so a workgroup there would stage the records,
    // reject them all, pass four barriers and find `hit` false in every lane.  It takes the miss colour at once: two scalar compares,
    // uniform over the workgroup and in front of every barrier.  k_raster and k_raster_rl only (the kernels such frames get; the
    // other instantiations do not carry the test).
    constexpr bool D3_ROWS = !FUSED && !ROWS && LV == Level::Common;
    bool d3_skip = false;
    if constexpr (D3_ROWS) {
        const uint32_t trow = P.tile_y0 + ty * P.tile_stride;
        d3_skip = P.fused_small == 2u && (trow < P.d3_trow0 || trow >= P.d3_trow1);
    }
    if (D3_ROWS && d3_skip) {
        color = pack4(0u, 0u, 0u, 255u);  // miss (:420-461; fused_small is only ever non-zero in 3D mode: render_impl)
    } else if (P.flags & RXR_FLAG_D3_ACTIVE) {
        constexpr bool fused = FUSED;
        uint32_t b0 = 0, b1 = 0;
        uint32_t my_bin_count = 0;
        const bool rows_binned = ROWS && P.fused_small == 0u;  // (k_raster_chunk / k_raster_vm also serve small scenes)
        if (rows_binned) {
            // every thread reads the (uniform) list bounds itself: no LDS round trip and no barrier in front of the first
            // list fetch; the bin count is handed back zeroed after the scan, when every thread has long read it
            my_bin_count = P.bin_count[bin];
            // (k_blockscan's lists, tried and retired: the first 64 row ids fetched into LDS in the same round trip as the count.  The 1 M-triangle
            // frame 0.574 -> 0.591 ms -- more than half of its tiles are empty and fetch 256 bytes of stale slots for nothing, and the others wait
            // for the ids in the prologue instead of behind the first barrier: profiles/r04/prefetch_ids_ab_c5.txt)
            const uint32_t start = P.chunk_base[bin / RXR_SCAN_CHUNK] + P.bin_offset[bin];
            b0 = min(start, P.list_capacity);
            b1 = min(start + my_bin_count, P.list_capacity);
        } else if (!fused && P.fused_small == 0u) {  // (s_bin[0..1]: this tile's 3D list)
            // this tile's bin list; the bin count is handed back zeroed for the next launch
            if (tid == 0) {
                uint32_t cnt = P.bin_count[bin];
                uint32_t start = P.chunk_base[bin / RXR_SCAN_CHUNK] + P.bin_offset[bin];
                s_bin[0] = min(start, P.list_capacity);
                s_bin[1] = min(start + cnt, P.list_capacity);  // on overflow the frame is re-rendered (rxr_synchronize)
                if (cnt) P.bin_count[bin] = 0u;
            }
            __syncthreads();
            b0 = s_bin[0];
            b1 = s_bin[1];
        }
        int surf_profile = -1;
        Vis op;
        op.zmin = 1.0f; op.best = -1; op.alpha = 0.0f; op.beta = 0.0f; op.slot = 0; op.batch = 0;
        front_init(op);
        uint32_t op_color = 0u;  // the opacity winner is shaded at once: the opaque pass rebuilds the stage
        if (P.has_opacity) {
            if constexpr (FUSED) scan_fused<true, LV>(P, stage, shade_store.s, tile_x0, tile_y0px, px, py, fx, fy, op, -1, nullptr);
            else if (P.fused_small == 2u) scan_implicit<true, LV>(P, stage, tile_x0, tile_y0px, px, py, fx, fy, op, -1, nullptr);
            else scan_lists<true, LV>(P, stage, b0, b1, tile_x0, tile_y0px, px, py, fx, fy, op, -1, nullptr);
            if (op.best >= 0) {
                const DevBatch &OB = P.batches3d[op.batch];
                surf_profile = (OB.flags & DB_HAS_PROFILE) ? (int)OB.profile_id : -1;
                TriShade OS;
                if constexpr (FUSED) OS = shade_store.s.shade[op.slot];
                else OS = P.tri_shade[op.best];
                op_color = shade3d_opacity<LV>(P, OS, op.batch, op.alpha, op.beta, op.zmin, fx, fy);
            }
            __syncthreads();  // everyone has copied its record before the stage is rebuilt
        }
        Vis vis;
        vis.zmin = 1.0f; vis.best = -1; vis.alpha = 0.0f; vis.beta = 0.0f; vis.slot = 0; vis.batch = 0;
        TriShade HS;     // shading record of the winner
        int hs_of = -1;  // triangle whose record HS already holds (row mode fetches it early)
        uint32_t win_flags = 0u;  // the winner's batch flags, where the visibility pass had them at hand (scan_implicit)
        const bool have_flags = !FUSED && P.fused_small == 2u;  // (uniform)
        PHASE_MARK(0);
        if constexpr (FUSED) scan_fused<false, LV>(P, stage, shade_store.s, tile_x0, tile_y0px, px, py, fx, fy, vis, surf_profile, &op);
        else if (P.fused_small == 2u) scan_implicit<false, LV>(P, stage, tile_x0, tile_y0px, px, py, fx, fy, vis, surf_profile, &op, &win_flags);
        else if (rows_binned) {
            // (the per-pixel surface_id of the opacity pass lives in the owning lane's registers: frames with opacity batches walk)
            if constexpr (ROWS) {
                // (until the end of round 4 a frame with an opacity pass walked every round: ONE translucent pane made the reduced box grid's
                // raster kernel 3.6 times slower.  The opacity pass only matters to opaque candidates that carry a profile id (the
                // surface_id rule, :1044-1048): rounds with such a candidate walk, like rounds with cut-outs -- rows_round)
                const bool row_mode = true;
                if (row_mode) row_store.r.key[ly * RXR_TILE_W + lx] = RXR_ZKEY_INIT;  // own cell; published by the barriers of the first staging round
                scan_lists_rows<LV, SPLITR>(P, stage, row_store.r, row_mode, b0, b1, tile_x0, tile_y0px, px, py, fx, fy, vis, surf_profile, &op,
                                   s_sort PHASE_ARG);
                if (tid == 0 && my_bin_count) P.bin_count[bin] = 0u;  // (a non-empty list went through the barriers of a round)
                PHASE_MARK(1);
                if (row_mode) rows_resolve(P, row_store.r, lx, ly, fx, fy, vis, HS, hs_of);  // (the last round ended with a barrier)
                PHASE_MARK(9);
            }
        } else scan_lists<false, LV>(P, stage, b0, b1, tile_x0, tile_y0px, px, py, fx, fy, vis, surf_profile, &op);

        PHASE_MARK(1);
        // The opacity layer's colour and depth wait in LDS while the fragment is shaded (each thread its own two words of s_sort: the
        // 2D pass has not begun, and row mode -- whose fragment queue lives there -- does not run in frames with an opacity pass): the
        // shading code sits at the kernel's 64 registers, and values that are live across it without being used in it are what the
        // compiler sends to scratch memory (4 bytes per pixel and frame for the colour alone, in frames that have no opacity pass at all).
        // (not in the kernels of Level::Chunk: k_raster_chunk[_rl] answered with MORE scratch -- 6 -> 20 spill instructions -- and ran 1.4 % slower)
        static_assert(RXR_SORT2D_MAX >= 2 * RXR_TILE_THREADS, "two words per thread");
        constexpr bool PARK_OPACITY = !feat<LV>.chunk || feat<LV>.programs;
        if (PARK_OPACITY && P.has_opacity) {  // (uniform)
            s_sort[tid] = op_color;
            s_sort[RXR_TILE_THREADS + tid] = __float_as_uint(op.best >= 0 ? op.zmin : 1.0f);
        }
        // resolve (rasterizer.rs:409-497): hit -> shaded colour; miss -> [0,0,0,255]
        const bool hit = vis.best >= 0;
        Frag F;
        F.world = F.normal = F.view_dir = F.base = F.lit = F.emis = mk3(0.0f, 0.0f, 0.0f);
        F.opacity = 0.0f;
        F.alpha_bits = 0u;
        F.rough = 0.5f;
        F.metal = 0.0f;
        if (hit) {
            if constexpr (FUSED) HS = shade_store.s.shade[vis.slot];
            else if (!ROWS || hs_of != vis.best) HS = P.tri_shade[vis.best];
            shade3d_begin<LV, RL>(P, HS, vis.batch, vis.alpha, vis.beta, vis.zmin, fx, fy, F, have_flags, win_flags);
        }
        PHASE_MARK(2);
        // (the kernels with split rounds keep the general loop alone, like the pair kernel: k_raster_rows_cut_rl answered with 8 more bytes of scratch)
        if (P.n_lights) shade3d_lights<LV, RL, RL && !SPLITR>(P, hit, F);  // wave-uniform call
        PHASE_MARK(3);
        color = hit ? shade3d_end<LV, RL>(F) : pack4(0u, 0u, 0u, 255u);
        if constexpr (feat<LV>.chunk) {
            if (P.has_brush && !hit) color = miss_brush_preview(P, px, py);  // :435-458
        }
        PHASE_MARK(4);
        float op_z = 1.0f;  // (1.0: no opacity fragment here)
        if constexpr (PARK_OPACITY) {
            if (P.has_opacity) op_z = __uint_as_float(s_sort[RXR_TILE_THREADS + tid]);
        } else {
            if (op.best >= 0) op_z = op.zmin;
        }
        if (op_z < 1.0f && vis.zmin > op_z) {  // :464-495
            uint32_t src = PARK_OPACITY ? s_sort[tid] : op_color;
            float src_r = (float)(src & 0xFFu), src_g = (float)((src >> 8) & 0xFFu), src_b = (float)((src >> 16) & 0xFFu);
            float src_a = byte_over_255(src >> 24);
            float dst_r = (float)(color & 0xFFu), dst_g = (float)((color >> 8) & 0xFFu), dst_b = (float)((color >> 16) & 0xFFu);
            float dst_a = byte_over_255(color >> 24);
            float inv_a = 1.0f - src_a;
            float out_r = src_r * src_a + dst_r * inv_a;
            float out_g = src_g * src_a + dst_g * inv_a;
            float out_b = src_b * src_a + dst_b * inv_a;
            float out_a = !(P.flags & RXR_FLAG_PRESERVE_TRANSPARENCY) ? 1.0f : rclamp(src_a + dst_a * inv_a, 0.0f, 1.0f);
            color = pack4(sat_u8(rclamp(out_r, 0.0f, 255.0f)), sat_u8(rclamp(out_g, 0.0f, 255.0f)), sat_u8(rclamp(out_b, 0.0f, 255.0f)),
                          sat_u8(rclamp(out_a * 255.0f, 0.0f, 255.0f)));
        }
    }

    // rasterizer.rs:501-553, strictly in submission order.  Tiles that no 2D pixel box reaches skip the pass
    // (a primitive only ever writes inside its box: :636-655, :1777-1821)
    const bool d2_here = (P.flags & RXR_FLAG_D2_ACTIVE) && P.n_prims2d && d2_box_meets(P, tile_x0, tile_y0px);
    if (d2_here) {
        color = pass2d<LV>(P, stage, s_bin, s_sort, RXR_SORT2D_MAX, bin, tile_x0, tile_y0px, px, py, fx, fy, color);
    }

    PHASE_MARK(5);
    if (in_frame) {
        // (the row inside the tile once more from the thread index, through a value the compiler cannot see through: kept alive from the
        // first line of the kernel to this one, `ly` was SPILLED by the 64-register kernels -- a scratch store and load per thread for a shift)
        uint32_t tid_again = threadIdx.x;
        asm volatile("" : "+v"(tid_again));
        const uint32_t ly_again = tid_again / RXR_TILE_W;
        const int64_t row = P.compact ? (int64_t)(ty * RXR_TILE_H + ly_again) : (int64_t)py - P.out_base_row;
        P.out[(size_t)row * P.out_row_stride + px] = color;
    }
    PHASE_MARK(6);
    PHASE_FLUSH;
}

// ---- pairs of tiles (binned scenes, Level::Common, no opacity pass) ---------------------------------------------------------------
// A tile of a scene of small triangles spends a quarter of its instructions on what does not depend on its pixels: list bounds, the
// staging of its ~20 candidates, the tile-level reject, the scans and the owner search of a row-mode round.  A workgroup of the pair
// kernels takes TWO vertically adjacent tiles -- the bins stay 16 x 16, the pre-pass and the stripes of a multi-GPU launch are untouched
// -- as one 16 x 32 tile: both bin lists are staged into the same rounds (an entry of the lower bin whose box starts above it is in the
// upper bin's list as well and is dropped: exact, a bin lists every triangle whose box meets it), the z-buffer in LDS has 512 cells,
// row mode runs over the boxes clipped to 32 rows, and every lane then resolves and shades its two pixels one after the other.  ALL
// visibility goes through the z-buffer's (z, index) keys here: a round that is walked (large triangles, cut-outs) merges each lane's
// winner into the lane's own two cells, so no per-pixel state lives in registers across the rounds.  Same fragments, same arg-min,
// same shading code: byte-identical to the single-tile kernels (tests/test_gpu_rows.py, the full-size configurations).
template <Level LV>
__device__ __forceinline__ void scan_lists_pair(const RasterParams &P, Stage &st, RowLdsT<32> &rl, uint32_t a0, uint32_t a1, uint32_t b0, uint32_t b1,
                                                uint32_t tile_x0, uint32_t tile_y0px, uint32_t lx, uint32_t ly) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t n_large = min(P.counters[CNT_LARGE], P.n_tris3d);
    const uint32_t n_a = a1 - a0, total = n_large + n_a + (b1 - b0);
    const uint32_t y_lower = tile_y0px + RXR_TILE_H;  // first row of the lower tile
    const float4 *g4 = reinterpret_cast<const float4 *>(P.tri_setup);
    for (uint32_t base = 0; base < total; base += RXR_STAGE_TRIS) {
        const uint32_t m = min(total - base, (uint32_t)RXR_STAGE_TRIS);
        // 1. ids of the round's list entries: large list, upper bin, lower bin
        if (tid < m) {
            const uint32_t e = base + tid;
            rl.raw[tid] = e < n_large ? P.large_list[e] : (e < n_large + n_a ? P.bin_list[a0 + (e - n_large)] : P.bin_list[b0 + (e - n_large - n_a)]);
        }
        __syncthreads();
        // 2. their records (ids outside this frame's records are never followed: clamped here, dropped in step 3)
        for (uint32_t f = tid; f < m * 6u; f += RXR_TILE_THREADS) {
            const uint32_t k = f / 6u, j = f - k * 6u;
            st.tri[f] = g4[(size_t)min(rl.raw[k], P.n_tris3d - 1u) * 6u + j];
        }
        __syncthreads();
        // 3. pixel box and tile-level edge reject on the LDS copies, against the 16 x 32 rectangle; survivors' slots are compacted
        bool keep = false;
        uint32_t id = 0;
        if (tid < m) {
            id = rl.raw[tid];
            const TriSetup &R = *reinterpret_cast<const TriSetup *>(&st.tri[tid * 6u]);
            const uint32_t min_x = R.bx & 0xFFFFu, max_x = R.bx >> 16, min_y = R.by & 0xFFFFu, max_y = R.by >> 16;
            keep = id < P.n_tris3d && !(min_x >= tile_x0 + RXR_TILE_W || max_x <= tile_x0 || min_y >= tile_y0px + 2u * RXR_TILE_H || max_y <= tile_y0px);
            // the lower bin's entry is the upper bin's entry too when its box begins above the lower tile
            if (base + tid >= n_large + n_a && min_y < y_lower) keep = false;
            if (keep && rxr_rect_outside_edges(R.ea, R.eb, R.ec, tile_x0, tile_y0px, RXR_TILE_W, 2u * RXR_TILE_H)) keep = false;
        }
        const unsigned long long mk = __ballot(keep);
        const uint32_t before = (uint32_t)__popcll(mk & ((1ull << lane) - 1ull));
        if (lane == 0) st.wave_cnt[wave] = (uint32_t)__popcll(mk);
        __syncthreads();
        uint32_t off = 0, n = 0;
#pragma unroll
        for (uint32_t w = 0; w < RXR_TILE_THREADS / 64; ++w) {
            const uint32_t c = st.wave_cnt[w];
            if (w < wave) off += c;
            n += c;
        }
        if (keep) {
            rl.slot[off + before] = (uint8_t)tid;
            st.ids[off + before] = id;
        }
        __syncthreads();
        // 4. the pixels of the candidates' boxes (row mode), or the walk -- merged into the same keys
        if (rows_round<true, true, 32u>(P, st, rl, n, tile_x0, tile_y0px)) continue;
#pragma unroll 1
        for (uint32_t h = 0; h < 2u; ++h) {
            const uint32_t px = tile_x0 + lx, py = tile_y0px + h * RXR_TILE_H + ly;
            const float fx = (float)px + 0.5f, fy = (float)py + 0.5f;
            Vis vis;
            vis.zmin = 1.0f; vis.best = -1; vis.alpha = 0.0f; vis.beta = 0.0f; vis.slot = 0; vis.batch = 0;
            for (uint32_t k = 0; k < n; ++k) {
                const uint32_t sl = rl.slot[k];
                const TriSetup &S = *reinterpret_cast<const TriSetup *>(&st.tri[sl * 6u]);
                const uint32_t t = st.ids[k];
                visit<false, LV>(P, S, &P.tri_shade[t], t, sl, px, py, fx, fy, vis, -1, nullptr);
            }
            if (vis.best >= 0) {  // (z < 1.0: visit starts from the cleared buffer's 1.0, :1060)
                // this lane's own cell; the rounds are separated by barriers, so nobody else touches it now
                const unsigned long long key = ((unsigned long long)z_order_bits(vis.zmin + 0.0f) << 32) | (uint32_t)vis.best;
                unsigned long long *const cell = &rl.key[(h * RXR_TILE_H + ly) * RXR_TILE_W + lx];
                if (key < *cell) *cell = key;
            }
        }
        __syncthreads();  // the stage is reused by the next round
    }
}

template <Level LV, bool RL>
__device__ __forceinline__ void raster_tile_pair(const RasterParams &P) {
    static_assert(!feat<LV>.chunk && !feat<LV>.programs, "the pair kernels serve Level::Common");
    __shared__ Stage stage;
    __shared__ uint32_t s_bin[4];
    __shared__ RowLdsT<32> rl;
    const uint32_t tx = blockIdx.x, ty0 = 2u * blockIdx.y, ty1 = ty0 + 1u;  // launch-local tile rows (tile_stride == 1: adjacent)
    const bool has_lower = ty1 < P.tiles_y;
    const uint32_t tid = threadIdx.x;
    const uint32_t tile_x0 = tx * RXR_TILE_W, tile_y0px = (P.tile_y0 + ty0) * RXR_TILE_H;
    const uint32_t lx = tid & (RXR_TILE_W - 1), ly = tid / RXR_TILE_W;
    const uint32_t bin_a = (ty0 + P.bin_row0) * P.tiles_x + tx, bin_b = (ty1 + P.bin_row0) * P.tiles_x + tx;
    // every thread reads the (uniform) list bounds itself; the counts are handed back zeroed below
    const uint32_t cnt_a = P.bin_count[bin_a], cnt_b = has_lower ? P.bin_count[bin_b] : 0u;
    const uint32_t start_a = P.chunk_base[bin_a / RXR_SCAN_CHUNK] + P.bin_offset[bin_a];
    const uint32_t start_b = has_lower ? P.chunk_base[bin_b / RXR_SCAN_CHUNK] + P.bin_offset[bin_b] : 0u;
    const uint32_t a0 = min(start_a, P.list_capacity), a1 = min(start_a + cnt_a, P.list_capacity);
    const uint32_t b0 = min(start_b, P.list_capacity), b1 = min(start_b + cnt_b, P.list_capacity);
    rl.key[tid] = RXR_ZKEY_INIT;  // own cells; published by the barriers of the first staging round
    rl.key[RXR_TILE_THREADS + tid] = RXR_ZKEY_INIT;
    scan_lists_pair<LV>(P, stage, rl, a0, a1, b0, b1, tile_x0, tile_y0px, lx, ly);
    if (tid == 0) {  // (a non-empty list went through the barriers of a round: every thread has read the counts)
        if (cnt_a) P.bin_count[bin_a] = 0u;
        if (cnt_b) P.bin_count[bin_b] = 0u;
    }
    // The 2D pass of a tile gathers its candidates in the UPPER tile's half of the z-buffer (2 KB = 512 entries; a tile with more walks
    // every primitive: correct, slow): each lane has read its upper winner before pass2d's first barrier, and the lower tile's half is
    // left alone until its own iteration -- so the workgroup's LDS stays under 20 KB and eight of them fit a CU.
    static_assert(sizeof(rl.key) / 2 >= 512 * sizeof(uint32_t), "the 2D candidate array aliases half of the z-buffer");
#pragma unroll 1
    for (uint32_t h = 0; h < 2u; ++h) {
        if (h == 1u && !has_lower) break;  // (uniform)
        const uint32_t px = tile_x0 + lx, py = tile_y0px + h * RXR_TILE_H + ly;
        const float fx = (float)px + 0.5f, fy = (float)py + 0.5f;
        const bool in_frame = px < P.width && py >= P.row0 && py < P.row1;
        Vis vis;
        vis.zmin = 1.0f; vis.best = -1; vis.alpha = 0.0f; vis.beta = 0.0f; vis.slot = 0; vis.batch = 0;
        TriShade HS;
        {
            // the winner of the pixel: its records are fetched together, its barycentrics re-derived (rows_resolve)
            const unsigned long long key = rl.key[(h * RXR_TILE_H + ly) * RXR_TILE_W + lx];
            if (key < RXR_ZKEY_INIT) {
                const uint32_t t = (uint32_t)key;
                const TriSetup S = P.tri_setup[t];
                HS = P.tri_shade[t];
                float alpha, beta, z;
                bary_depth(S.v0x, S.v0y, S.v1x, S.v1y, S.v2x, S.v2y, S.area, S.iz0, S.iz1, S.iz2, fx, fy, alpha, beta, z);
                vis.zmin = z; vis.best = (int)t; vis.alpha = alpha; vis.beta = beta; vis.batch = S.batch;
            }
        }
        const bool hit = vis.best >= 0;
        Frag F;
        F.world = F.normal = F.view_dir = F.base = F.lit = F.emis = mk3(0.0f, 0.0f, 0.0f);
        F.opacity = 0.0f;
        F.alpha_bits = 0u;
        F.rough = 0.5f;
        F.metal = 0.0f;
        if (hit) shade3d_begin<LV, RL>(P, HS, vis.batch, vis.alpha, vis.beta, vis.zmin, fx, fy, F);
        if (P.n_lights) shade3d_lights<LV, RL, false>(P, hit, F);  // wave-uniform call (no prefix loop: see shade3d_lights)
        uint32_t color = hit ? shade3d_end<LV, RL>(F) : pack4(0u, 0u, 0u, 255u);
        const uint32_t tile_yh = tile_y0px + h * RXR_TILE_H;
        const bool d2_here = (P.flags & RXR_FLAG_D2_ACTIVE) && P.n_prims2d && d2_box_meets(P, tile_x0, tile_yh);
        if (d2_here) color = pass2d<LV>(P, stage, s_bin, reinterpret_cast<uint32_t *>(rl.key), 512u, h ? bin_b : bin_a, tile_x0, tile_yh, px, py, fx, fy, color);
        if (in_frame) {
            const int64_t row = P.compact ? (int64_t)((ty0 + h) * RXR_TILE_H + ly) : (int64_t)py - P.out_base_row;
            P.out[(size_t)row * P.out_row_stride + px] = color;
        }
    }
}

__device__ __forceinline__ const RasterParams &kernarg_params_early() { return *(const RasterParams *)__builtin_amdgcn_kernarg_segment_ptr(); }
// two instantiations so that each path gets its own register allocation
// Every raster kernel reads its parameter block in place in the kernarg segment (kernarg_params) instead of taking it by
// value: with a by-value block the compiler fetches the fields at the top of the kernel, runs out of SGPRs and parks them
// in VGPR lanes (369 v_writelane / v_readlane in k_raster, 51 of them executed by every wave before its first useful
// instruction); read in place they are scalar loads at the point of use (17 spill instructions).  Measured A-B-A-B on one
// box: bench frame 208 -> 198 us, the 1-light frame 126 -> 117 us.
#ifdef RXR_JIT
// the kernel of a run-time compiled program set, one level per compilation (rxr_jit.hip compiles a level when the first frame that
// needs it is launched): RXR_JIT_LEVEL is one of jit_level_number, JIT_LV its level (jit_slot_level: Vm, VmV or JitPlain)
// (1 M triangles with the configuration-C5 program, raster kernel: VmV at 8 waves per SIMD (64 VGPRs) 656 us, 7: 676, 6: 710;
// Vm at 8: 695 us, 7: 666, 6: 694, 5: 763; JitPlain at 8: 566 us -- the interpreter kernels take 1180 us)
#ifndef RXR_JIT_LEVEL
#define RXR_JIT_LEVEL 8
#endif
static_assert(jit_slot_of_number(RXR_JIT_LEVEL) >= 0, "RXR_JIT_LEVEL is none of jit_level_number");
constexpr Level JIT_LV = jit_slot_level[jit_slot_of_number(RXR_JIT_LEVEL)];
#ifndef RXR_JIT_WAVES_PER_SIMD
#define RXR_JIT_WAVES_PER_SIMD (feat<JIT_LV>.vis_programs ? 7 : 8)
#endif
extern "C" __global__ void __launch_bounds__(RXR_TILE_THREADS, RXR_JIT_WAVES_PER_SIMD) k_raster_jit(RasterParams) { raster_tile<false, JIT_LV, true>(kernarg_params_early()); }
static_assert((RXR_JIT_LEVEL != 2) == !feat<JIT_LV>.vis_programs, "k_raster_jit_cut: the levels at which no program decides visibility");
#if RXR_JIT_LEVEL != 2
// ... and for frames with cut-out or profiled batches (RasterParams.split_rounds), as k_raster_rows_cut: the same code object carries both
extern "C" __global__ void __launch_bounds__(RXR_TILE_THREADS, RXR_JIT_WAVES_PER_SIMD) k_raster_jit_cut(RasterParams) { raster_tile<false, JIT_LV, true, false, true, true>(kernarg_params_early()); }
#endif
#else
extern "C" __global__ void __launch_bounds__(RXR_TILE_THREADS, RXR_RASTER_WAVES_PER_SIMD) k_raster(RasterParams) { raster_tile<false, Level::Common>(kernarg_params_early()); }
extern "C" __global__ void __launch_bounds__(RXR_TILE_THREADS) k_raster_fused(RasterParams) { raster_tile<true, Level::Common>(kernarg_params_early()); }
// RXR_LIGHT_MATH=relaxed (RasterParams.relaxed_lights): the same kernels with the relaxed light loop (shade3d_lights<LV, true>)
extern "C" __global__ void __launch_bounds__(RXR_TILE_THREADS, RXR_RASTER_WAVES_PER_SIMD) k_raster_rl(RasterParams) { raster_tile<false, Level::Common, false, true>(kernarg_params_early()); }
// binned scenes (more than RXR_STAGE_TRIS triangles): the walk may switch to row mode per round (rows_round)
#ifndef RXR_ROWS_WAVES_PER_SIMD
#define RXR_ROWS_WAVES_PER_SIMD 8  // C5: unbounded (87 VGPRs, 5 waves) 797 us, 6: 718, 7: 727; with the parameter block in place 6: 654, 8: 628
#endif
extern "C" __global__ void __launch_bounds__(RXR_TILE_THREADS, RXR_ROWS_WAVES_PER_SIMD) k_raster_rows(RasterParams) { raster_tile<false, Level::Common, true>(kernarg_params_early()); }
extern "C" __global__ void __launch_bounds__(RXR_TILE_THREADS, RXR_ROWS_WAVES_PER_SIMD) k_raster_rows_rl(RasterParams) { raster_tile<false, Level::Common, true, true>(kernarg_params_early()); }
// ... and for sparse frames (RasterParams.row_spans)
extern "C" __global__ void __launch_bounds__(RXR_TILE_THREADS, RXR_ROWS_WAVES_PER_SIMD) k_raster_rows_sp(RasterParams) { raster_tile<false, Level::Common, true, false, true>(kernarg_params_early()); }
extern "C" __global__ void __launch_bounds__(RXR_TILE_THREADS, RXR_ROWS_WAVES_PER_SIMD) k_raster_rows_rl_sp(RasterParams) { raster_tile<false, Level::Common, true, true, true>(kernarg_params_early()); }
// ... and for frames with cut-out batches (texel alpha) or, under an opacity pass, batches with a profile id (RasterParams.split_rounds):
// rounds in row mode AROUND such candidates (scan_lists_rows SPLITR) -- two batches with a fence texture among the 96 of the reduced box
// grid: 98.5 -> 72 us, one in eight: 131 -> 79 us; kernels of their own so that the plain ones stay what they are
extern "C" __global__ void __launch_bounds__(RXR_TILE_THREADS, RXR_ROWS_WAVES_PER_SIMD) k_raster_rows_cut(RasterParams) { raster_tile<false, Level::Common, true, false, true, true>(kernarg_params_early()); }
extern "C" __global__ void __launch_bounds__(RXR_TILE_THREADS, RXR_ROWS_WAVES_PER_SIMD) k_raster_rows_cut_rl(RasterParams) { raster_tile<false, Level::Common, true, true, true, true>(kernarg_params_early()); }
// two tiles per workgroup (raster_tile_pair): binned scenes without an opacity pass, launches whose tile rows are adjacent
#ifndef RXR_PAIR_WAVES_PER_SIMD
#define RXR_PAIR_WAVES_PER_SIMD 8
#endif
extern "C" __global__ void __launch_bounds__(RXR_TILE_THREADS, RXR_PAIR_WAVES_PER_SIMD) k_raster_pair(RasterParams) { raster_tile_pair<Level::Common, false>(kernarg_params_early()); }
extern "C" __global__ void __launch_bounds__(RXR_TILE_THREADS, RXR_PAIR_WAVES_PER_SIMD) k_raster_pair_rl(RasterParams) { raster_tile_pair<Level::Common, true>(kernarg_params_early()); }
// the rarer levels (rxr_device.h): k_raster_chunk -- chunk textures and the full-fragment alpha test they need -- and k_raster_vm, whose
// interpreter (rxr_vm.h) keeps its state in scratch memory.  These two contain real (out-of-line) calls that take the parameter block
// by reference.  Handing them the by-value kernel argument would make the compiler copy all of it to scratch and turn every P.field
// into a scratch load (measured: 3.5x on the whole kernel); the kernarg segment itself is addressable, so they read it in place.
__device__ __forceinline__ const RasterParams &kernarg_params() {
    return *(const RasterParams *)__builtin_amdgcn_kernarg_segment_ptr();
}
// Bench frame forced through k_raster_chunk (RXR_MIN_KERNEL_LEVEL=1): unbounded (97 VGPRs, 5 waves per SIMD) 297 us, 6: 230, 7: 219,
// 8: 209 (k_raster: 197).  Before the staircase left scratch memory (front_insert) and the last real call was inlined it
// took 330 us with the same VALU instruction count: per-wave latency, not arithmetic.
#ifndef RXR_CHUNK_WAVES_PER_SIMD
#define RXR_CHUNK_WAVES_PER_SIMD 8
#endif
extern "C" __global__ void __launch_bounds__(RXR_TILE_THREADS, RXR_CHUNK_WAVES_PER_SIMD) k_raster_chunk(RasterParams) { raster_tile<false, Level::Chunk, true>(kernarg_params()); }
extern "C" __global__ void __launch_bounds__(RXR_TILE_THREADS, RXR_CHUNK_WAVES_PER_SIMD) k_raster_chunk_rl(RasterParams) { raster_tile<false, Level::Chunk, true, true>(kernarg_params()); }
// ... and with rounds in row mode around cut-out / profiled candidates (RasterParams.split_rounds), as k_raster_rows_cut*
extern "C" __global__ void __launch_bounds__(RXR_TILE_THREADS, RXR_CHUNK_WAVES_PER_SIMD) k_raster_chunk_cut(RasterParams) { raster_tile<false, Level::Chunk, true, false, true, true>(kernarg_params()); }
extern "C" __global__ void __launch_bounds__(RXR_TILE_THREADS, RXR_CHUNK_WAVES_PER_SIMD) k_raster_chunk_cut_rl(RasterParams) { raster_tile<false, Level::Chunk, true, true, true, true>(kernarg_params()); }
extern "C" __global__ void __launch_bounds__(RXR_TILE_THREADS, RXR_VM_WAVES_PER_SIMD) k_raster_vm(RasterParams) { raster_tile<false, Level::Vm, true>(kernarg_params()); }
extern "C" __global__ void __launch_bounds__(RXR_TILE_THREADS, RXR_VM_WAVES_PER_SIMD) k_raster_vm_s(RasterParams) { raster_tile<false, Level::VmS, true>(kernarg_params()); }
extern "C" __global__ void __launch_bounds__(RXR_TILE_THREADS, RXR_VM_WAVES_PER_SIMD) k_raster_vm_sv(RasterParams) { raster_tile<false, Level::VmSV, true>(kernarg_params()); }
extern "C" __global__ void __launch_bounds__(RXR_TILE_THREADS, RXR_VM_WAVES_PER_SIMD) k_raster_vm_p(RasterParams) { raster_tile<false, Level::VmP, true>(kernarg_params()); }
extern "C" __global__ void __launch_bounds__(RXR_TILE_THREADS, RXR_VM_WAVES_PER_SIMD) k_raster_vm_v(RasterParams) { raster_tile<false, Level::VmV, true>(kernarg_params()); }

#if RXR_PHASE_TIMING
extern "C" int rxr_debug_phase_read(unsigned long long *out16, int reset) {
    static unsigned long long h[1024][16];
    if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_phase), sizeof(h)) != hipSuccess) return -1;
    for (int k = 0; k < 16; ++k) {
        out16[k] = 0;
        for (int i = 0; i < 1024; ++i) out16[k] += h[i][k];
    }
    if (reset) {
        memset(h, 0, sizeof(h));
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_phase), h, sizeof(h)) != hipSuccess) return -1;
    }
    return 0;
}
#endif

// rows of the framebuffer that nothing of the frame can reach (render_impl, rxr_ctx::content_row0 / 1): one value, 16-byte stores
extern "C" __global__ void __launch_bounds__(256) k_fill_words(uint32_t *dst, unsigned long long n_words, uint32_t value) {
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    const unsigned long long head = min(n_words, (unsigned long long)(((16u - ((uintptr_t)dst & 15u)) & 15u) >> 2));  // words up to 16-byte alignment
    const unsigned long long n16 = (n_words - head) >> 2, tail0 = head + (n16 << 2);
    u32x4 *const d16 = reinterpret_cast<u32x4 *>(dst + head);
    const u32x4 v = {value, value, value, value};
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256u + threadIdx.x; i < n16; i += (unsigned long long)gridDim.x * 256u) d16[i] = v;
    if (blockIdx.x == 0) {
        if (threadIdx.x < head) dst[threadIdx.x] = value;
        if (tail0 + threadIdx.x < n_words) dst[tail0 + threadIdx.x] = value;  // (fewer than four words)
    }
}

// the pixels of a launch's rows that lie outside its rows' spans (RasterParams.row_spans): the 3D miss colour.  One workgroup per PIXEL
// row (grid: tile rows x RXR_TILE_H -- one workgroup per tile row took 13 us for the 8K frame's 186 rows); 16-byte stores where the
// segment's alignment allows them.
extern "C" __global__ void __launch_bounds__(256) k_fill_outside_spans(RasterParams P) {
    const uint32_t trow = P.tile_y0 + blockIdx.x, y = trow * RXR_TILE_H + blockIdx.y;
    if (y < P.row0 || y >= P.row1) return;
    const uint2 span = P.row_spans[trow];
    const uint32_t x_lo = min(span.x * RXR_TILE_W, P.width), x_hi = min(max(span.y, span.x) * RXR_TILE_W, P.width);  // pixels [x_lo, x_hi) belong to the raster
    uint32_t *const row = P.out + (size_t)((int64_t)y - P.out_base_row) * P.out_row_stride;
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    const u32x4 v4 = {0xFF000000u, 0xFF000000u, 0xFF000000u, 0xFF000000u};
#pragma unroll
    for (int part = 0; part < 2; ++part) {
        uint32_t *const seg = part ? row + x_hi : row;
        const uint32_t n = part ? P.width - x_hi : x_lo;
        if ((((uintptr_t)seg) & 15u) == 0u) {  // (uniform) tile columns are 64 bytes wide: aligned whenever the row is
            for (uint32_t i = threadIdx.x; i < (n >> 2); i += 256u) reinterpret_cast<u32x4 *>(seg)[i] = v4;
            if (threadIdx.x < (n & 3u)) seg[(n & ~3u) + threadIdx.x] = 0xFF000000u;
        } else {
            for (uint32_t i = threadIdx.x; i < n; i += 256u) seg[i] = 0xFF000000u;
        }
    }
}

// Device-projected frames (rxr_project.hip): the batch boxes exist on the device only, so the row spans of a sparse frame are made here --
// RasterParams.row_spans arrives holding what the HOST knows (the pixel box of a host-projected 2D pass, or nothing) and leaves as its
// union with the pixel box of a device-projected 2D pass (`d2_box`, k_proj2d_prims; NULL: none) and every kept mesh's box, through the
// same arithmetic as rxr_upload_frame's for host-projected batches (the batch box reject of make_setup, then the reference's own tiles
// that pass its box test: rxr_ref_tile_span; rasterizer.rs:978-983).  Idempotent: a second render of the same resident frame finds the
// same table.  One workgroup per 64 tile rows; a thread per mesh reduces it to its tile rectangle and marks the workgroup's rows that
// it crosses with LDS atomics that return nothing (a thread per ROW walking the rectangles was a chain of LDS round trips: 16 us).
#define RXR_SPAN_MESHES_MAX 1024u
extern "C" __global__ void __launch_bounds__(256) k_spans_from_meshes(RasterParams P, uint32_t n_tile_rows, const uint32_t *d2_box, uint2 *host_copy) {
    __shared__ uint32_t s_lo[64], s_hi[64];
    const uint32_t tid = threadIdx.x, row_base = blockIdx.x * 64u;
    uint2 *const spans = const_cast<uint2 *>(P.row_spans);
    if (tid < 64u) {
        const uint32_t row = row_base + tid;
        const uint2 base = row < n_tile_rows ? spans[row] : make_uint2(0u, 0u);
        const bool any = base.x < base.y;
        uint32_t lo0 = any ? base.x : 0xFFFFFFFFu, hi0 = any ? base.y : 0u;
        if (d2_box) {  // (uniform) pixels [x0, x1) x [y0, y1), as rxr_upload_frame's add_span takes the host's
            const uint32_t x0 = d2_box[0], x1 = min(d2_box[1], P.width), y0 = d2_box[2], y1 = min(d2_box[3], P.height);
            if (x0 < x1 && y0 < y1 && row >= y0 / RXR_TILE_H && row < min((y1 + RXR_TILE_H - 1u) / RXR_TILE_H, n_tile_rows)) {
                lo0 = min(lo0, x0 / RXR_TILE_W);
                hi0 = max(hi0, min((x1 + RXR_TILE_W - 1u) / RXR_TILE_W, P.tiles_x));
            }
        }
        s_lo[tid] = lo0;
        s_hi[tid] = hi0;
    }
    __syncthreads();
    auto dec = [](uint32_t e) { return __uint_as_float((e & 0x80000000u) ? (e ^ 0x80000000u) : ~e); };
    for (uint32_t m = tid; m < P.n_batches3d; m += 256u) {
        const DevBBox bb = P.dev_bbox[m];
        const float bx = dec(bb.min_x), by = dec(bb.min_y), bw = dec(bb.max_x) - bx, bh = dec(bb.max_y) - by;
        const bool keep = !(P.batches3d[m].flags & DB_SKIP) && bx < (float)P.width && (bx + bw) > 0.0f && by < (float)P.height && (by + bh) > 0.0f;
        if (!keep) continue;
        uint32_t x0 = 0, x1 = 0, y0 = 0, y1 = 0;
        rxr_ref_tile_span_quick(by, bh, P.height, P.ref_tile, 0.0f, y0, y1);
        if (y0 >= y1) continue;
        const uint32_t r0 = max(y0 / RXR_TILE_H, row_base), r1 = min(min((y1 + RXR_TILE_H - 1u) / RXR_TILE_H, n_tile_rows), row_base + 64u);
        if (r0 >= r1) continue;  // (none of this workgroup's rows)
        rxr_ref_tile_span_quick(bx, bw, P.width, P.ref_tile, 0.0f, x0, x1);
        if (x0 >= x1) continue;
        const uint32_t c0 = x0 / RXR_TILE_W, c1 = min((x1 + RXR_TILE_W - 1u) / RXR_TILE_W, P.tiles_x);
        for (uint32_t r = r0; r < r1; ++r) {
            atomicMin(&s_lo[r - row_base], c0);
            atomicMax(&s_hi[r - row_base], c1);
        }
    }
    __syncthreads();
    if (tid < 64u && row_base + tid < n_tile_rows) {
        const uint32_t a = s_lo[tid], b = s_hi[tid];
        const uint2 v = a < b ? make_uint2(a, b) : make_uint2(0u, 0u);
        spans[row_base + tid] = v;
        if (host_copy) host_copy[row_base + tid] = v;  // (page-locked host memory: rxr_render_download learns which rows need not cross PCIe)
    }
}

// ---- host-callable launchers (used by rxr_api.hip) ------------------------------------------------
extern "C" uint32_t rxr_span_meshes_max(void) { return RXR_SPAN_MESHES_MAX; }
extern "C" void rxr_launch_spans_from_meshes(const RasterParams *P, uint32_t n_tile_rows, const uint32_t *d2_box, uint2 *host_copy, hipStream_t s) {
    if (!P->row_spans || !P->dev_bbox || !n_tile_rows) return;
    RXR_LAUNCH(k_spans_from_meshes, dim3((n_tile_rows + 63u) / 64u), dim3(256), s, *P, n_tile_rows, d2_box, host_copy);
}
extern "C" void rxr_launch_setup(const RasterParams *P, hipStream_t s) {
    if (P->n_tris3d == 0) return;
    uint32_t blocks = (P->n_tris3d + 255u) / 256u;
    RXR_LAUNCH(k_setup3d, dim3(blocks), dim3(256), s, *P);
}
extern "C" void rxr_launch_scan(const ScanArgs *A, hipStream_t s) {
    uint32_t chunks = (A->n + RXR_SCAN_CHUNK - 1u) / RXR_SCAN_CHUNK;
    if (chunks == 0) chunks = 1;
    RXR_LAUNCH(k_scan, dim3(chunks), dim3(256), s, *A);
}
extern "C" void rxr_launch_bin2d_count(const RasterParams *P, hipStream_t s) {
    if (P->n_prims2d == 0) return;
    RXR_LAUNCH(k_bin2d_count, dim3((P->n_prims2d + 255u) / 256u), dim3(256), s, *P);
}
extern "C" void rxr_launch_bin2d_fill(const RasterParams *P, hipStream_t s) {
    if (P->n_prims2d == 0) return;
    RXR_LAUNCH(k_bin2d_fill, dim3((P->n_prims2d + 255u) / 256u), dim3(256), s, *P);
}
extern "C" void rxr_launch_blockscan(const RasterParams *P, hipStream_t s) {
    if (P->n_tris3d == 0 || P->tiles_x * P->tiles_y == 0) return;
    const uint32_t blocks = ((P->tiles_x + 3u) / 4u) * ((P->tiles_y + 3u) / 4u);
    RXR_LAUNCH(k_blockscan, dim3(blocks), dim3(256), s, *P);
}
extern "C" void rxr_launch_blockscan2d(const RasterParams *P, hipStream_t s) {
    if (P->n_prims2d == 0 || P->tiles_x * P->tiles_y == 0) return;
    const uint32_t blocks = ((P->tiles_x + 3u) / 4u) * ((P->tiles_y + 3u) / 4u);
    RXR_LAUNCH(k_blockscan2d, dim3(blocks), dim3(256), s, *P);
}
extern "C" void rxr_launch_fill(const RasterParams *P, hipStream_t s) {
    if (P->n_tris3d == 0) return;
    uint32_t blocks = (P->n_tris3d + 255u) / 256u;
    RXR_LAUNCH(k_fill, dim3(blocks), dim3(256), s, *P);
}
extern "C" void rxr_launch_fill_words(uint32_t *dst, uint64_t n_words, uint32_t value, hipStream_t s) {
    if (!n_words) return;
    const uint64_t want = (n_words / 4u + 1023u) / 1024u;  // four 16-byte stores per thread
    const uint32_t blocks = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(want, 1u), 8192u);
    RXR_LAUNCH(k_fill_words, dim3(blocks), dim3(256), s, dst, (unsigned long long)n_words, value);
}
extern "C" void rxr_launch_fill_outside_spans(const RasterParams *P, hipStream_t s) {
    if (!P->row_spans || !P->tiles_y) return;
    RXR_LAUNCH(k_fill_outside_spans, dim3(P->tiles_y, RXR_TILE_H), dim3(256), s, *P);
}
// the route of a launch (rxr_route.h); spans: is -- or, for the host's question, would be -- the span table attached?
static rxr_route::Choice raster_route_of(const RasterParams *P, bool spans) {
    rxr_route::Facts f;
    f.kernel_level = P->kernel_level;
    f.plain_programs = P->plain_programs != 0;
    f.fused_small = P->fused_small;
    f.d3_active = (P->flags & RXR_FLAG_D3_ACTIVE) != 0;
    f.split_rounds = P->split_rounds != 0;
    f.spans = spans;
    f.rl = P->relaxed_lights && P->n_lights;
    f.has_opacity = P->has_opacity != 0;
    f.tile_stride = P->tile_stride;
    f.no_rows = getenv("RXR_NO_ROWS") != nullptr;  // tuning knob
    const char *pt = getenv("RXR_PAIR_TILES");     // (both read per launch: the tests switch them)
    f.pairs_on = pt && pt[0] == '1';
    return rxr_route::raster_route(f);
}
// would the kernel of this launch look RasterParams.row_spans up if the table were attached?  (the host asks before it attaches the
// table, narrows the grid and fills outside the spans)
extern "C" int rxr_raster_takes_spans(const RasterParams *P) { return raster_route_of(P, true).takes_spans ? 1 : 0; }
// grid_x: workgroups per tile row (0: tiles_x; with RasterParams.row_spans the widest span of the launch's rows)
// Returns the symbol name of the kernel it launched ("" when there was nothing to launch): rxr_debug_last_raster_kernel hands it to the
// tests (tests/test_gpu_routes.py pins every kernel to a scene of its own).
extern "C" const char *rxr_launch_raster_grid(const RasterParams *P, uint32_t grid_x, hipStream_t s);
extern "C" const char *rxr_launch_raster(const RasterParams *P, hipStream_t s) { return rxr_launch_raster_grid(P, 0u, s); }
extern "C" const char *rxr_launch_raster_grid(const RasterParams *P, uint32_t grid_x, hipStream_t s) {
    if (P->tiles_x * P->tiles_y == 0) return "";
    if (!grid_x || !P->row_spans) grid_x = P->tiles_x;
    // route id -> kernel and its symbol name: RXR_RASTER is the one place a name comes from
    struct Entry {
        rxr_route::Route id;
        void (*kernel)(RasterParams);
        const char *name;
    };
#define RXR_RASTER(kernel, id) {rxr_route::id, kernel, #kernel}
    static constexpr Entry table[] = {
        RXR_RASTER(k_raster, RASTER), RXR_RASTER(k_raster_fused, FUSED), RXR_RASTER(k_raster_rl, RASTER_RL),
        RXR_RASTER(k_raster_rows, ROWS), RXR_RASTER(k_raster_rows_rl, ROWS_RL), RXR_RASTER(k_raster_rows_sp, ROWS_SP),
        RXR_RASTER(k_raster_rows_rl_sp, ROWS_RL_SP), RXR_RASTER(k_raster_rows_cut, ROWS_CUT), RXR_RASTER(k_raster_rows_cut_rl, ROWS_CUT_RL),
        RXR_RASTER(k_raster_pair, PAIR), RXR_RASTER(k_raster_pair_rl, PAIR_RL),
        RXR_RASTER(k_raster_chunk, CHUNK), RXR_RASTER(k_raster_chunk_rl, CHUNK_RL), RXR_RASTER(k_raster_chunk_cut, CHUNK_CUT),
        RXR_RASTER(k_raster_chunk_cut_rl, CHUNK_CUT_RL),
        RXR_RASTER(k_raster_vm, VM), RXR_RASTER(k_raster_vm_s, VM_S), RXR_RASTER(k_raster_vm_sv, VM_SV), RXR_RASTER(k_raster_vm_p, VM_P),
        RXR_RASTER(k_raster_vm_v, VM_V),
    };
    static_assert(sizeof(table) / sizeof(table[0]) == rxr_route::N_ROUTES, "one entry per route");
    static_assert([] {
        for (int i = 0; i < rxr_route::N_ROUTES; ++i)
            if (table[i].id != i) return false;
        return true;
    }(), "in the order of the enum");
    const rxr_route::Choice c = raster_route_of(P, P->row_spans != nullptr);
    const Entry &e = table[c.route];
    // tiles_y <= 2048 (frames of at most 32768 rows)
    const dim3 grid = c.pair_grid ? dim3(P->tiles_x, (P->tiles_y + 1u) / 2u) : dim3(grid_x, P->tiles_y);
    RXR_LAUNCH(e.kernel, grid, dim3(RXR_TILE_THREADS), s, *P);
    return e.name;
}
#undef RXR_RASTER
#endif  // !RXR_JIT
