// rxr_bake.hip -- running a Rusteria program over an image: Rusteria::shade (rusteria/src/lib.rs:161-210) followed by
// RenderBuffer::as_rgba_bytes (rusteria/src/renderbuffer.rs:88-107, :152-155), the bake Chunk::add_shader (src/chunk.rs:104-122)
// runs at 64 x 64 for chunk.shader_textures[i].  include/rxr.h: rxr_bake_shaders, rxr_bake_shaders_to (rxr_check_bake, the
// validation alone, sits next to rxr_check_shaders in rxr_api.hip).
//
// Semantics, per texel (x, y) of a W x H bake of program p (row-major, top row first, as RenderBuffer stores it):
//   * uv = (x as f32 / W as f32, 1.0 - (y as f32 / H as f32), 0.0), color = 0 (lib.rs:188-194); every other Execution field holds its
//     Execution::new value -- roughness 0.5, the rest 0, `time` and `hitpoint` included: the bake never sets them;
//   * Execution::shade(shade_index) -- the interpreter of rxr_vm.h, the same instantiation the programmed raster kernels run;
//   * float pixel = [color.x, color.y, color.z, 1.0] through RenderBuffer::accum_from with accum == 1 (renderbuffer.rs:77-82:
//     old * (1 - 1) + new * 1 with old == 0), the identity except that -0.0 becomes +0.0: written here as `c + 0.0f`;
//   * byte pixel = ((c.powf(0.4545) * 255.0) as u8) for r, g, b and 255 for alpha (renderbuffer.rs:96-101); Rust's cast saturates,
//     truncates and maps NaN to 0.  powf is the device math library's.
// The reference walks the image in 80 x 80 tiles with one Execution per tile (lib.rs:167-177) and resets only uv and color between
// texels.  For the programs accepted here -- those rxr_set_shaders accepts (no leaking locals / globals / emissive) that also never
// read roughness / metallic / opacity / normal / bump before writing it when they write it (rxr_bake_refusal, rxr_ctx.h) -- no
// texel can see what an earlier one left, so the tile split and the walking order have no effect on the result (as SURVEY row R9
// notes for the raster path's tiles).  Texture::generate_normals (chunk.rs:119) fills Texture.data_ext only, which
// src/rasterizer.rs never reads: not computed.
//
// Kernel: one launch covers all n bakes of a call.  A workgroup is 256 consecutive texels of ONE bake, so the program index is
// uniform for the workgroup and the interpreter's code fetches stay scalar loads; the value stack's LDS part is the block the
// programmed raster kernels use (rxvm::stack_block).  A lane writes one 16-byte store to the float buffer and one packed 32-bit
// store to the byte buffer.  Bakes always run the interpreter: the run-time compiled kernels of a set (rxr_jit.hip) are neither
// used nor touched, and the buffers (rxr_ctx: d_bake_*) are the bake's own -- an uploaded frame renders as if no bake had run.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "rxr_debug.h"
#include "rxr_query.h"
#include "rxr_vm.h"

struct BakeArgs {
    const uint32_t *vm_code;
    const DevProgram *programs;
    const DevPattern *patterns;
    const float *pattern_data;
    const float *palette;
    uint32_t n_programs, n_patterns, n_normal_patterns, n_palette;
    const uint32_t *jobs;      // per bake: the program
    uint32_t width, height, texels, groups_per_job;   // texels = width * height; groups_per_job = ceil(texels / 256)
    float4 *pixels;            // [n][height][width] or null
    uint32_t *rgba;            // [n][height][width] packed r | g << 8 | b << 16 | a << 24, or null
    uint32_t *fault;           // BAKE_FAULT_WORDS
};

// `(c.powf(0.4545) * 255.0) as u8`
__device__ __forceinline__ uint32_t gamma_byte(float c) {
    const float v = powf(c, 0.4545f) * 255.0f;
    return !(v > 0.0f) ? 0u : (v >= 255.0f ? 255u : (uint32_t)v);   // (NaN -> 0)
}

template <bool SSP>
__device__ __forceinline__ void bake_texels(const BakeArgs &A) {
    const uint32_t job = blockIdx.x / A.groups_per_job;
    const uint32_t t = (blockIdx.x - job * A.groups_per_job) * RXR_TILE_THREADS + threadIdx.x;
    if (t >= A.texels) return;
    const uint32_t pi = A.jobs[job];   // (uniform: a scalar load)
    // what the interpreter reads of a frame's parameter block
    RasterParams P{};
    P.vm_code = A.vm_code;
    P.programs = A.programs;
    P.patterns = A.patterns;
    P.pattern_data = A.pattern_data;
    P.palette = A.palette;
    P.n_programs = A.n_programs;
    P.n_patterns = A.n_patterns;
    P.n_normal_patterns = A.n_normal_patterns;
    P.n_palette = A.n_palette;
    P.vm_fault = A.fault + BAKE_FAULT_SCRATCH;   // (the interpreter's own report: a word nobody reads; the record below names the texel)
    const uint32_t y = t / A.width, x = t - y * A.width;
    rxvm::IO io;
    rxvm::io_defaults(io);
    io.uv = rxvm::mk((float)x / (float)A.width, 1.0f - ((float)y / (float)A.height), 0.0f);
    const uint32_t fault = rxvm::shade_inline<SSP>(P, pi, io, rxvm::stack_block());
    if (fault && atomicCAS(A.fault + BAKE_FAULT_CODE, 0u, fault) == 0u) {   // the first faulting texel is the one reported
        A.fault[BAKE_FAULT_PROGRAM] = pi;
        A.fault[BAKE_FAULT_JOB] = job;
        A.fault[BAKE_FAULT_X] = x;
        A.fault[BAKE_FAULT_Y] = y;
    }
    const float r = io.color.x + 0.0f, g = io.color.y + 0.0f, b = io.color.z + 0.0f;   // accum_from: -0.0 -> +0.0
    const size_t at = (size_t)job * A.texels + t;
    if (A.pixels) A.pixels[at] = make_float4(r, g, b, 1.0f);
    if (A.rgba) A.rgba[at] = gamma_byte(r) | (gamma_byte(g) << 8) | (gamma_byte(b) << 16) | 0xFF000000u;
}

// k_bake: the interpreter with per-lane stack depths; k_bake_s: the set carries static depths (rxr_ctx::programs_static), as k_raster_vm / _s
extern "C" __global__ __launch_bounds__(RXR_TILE_THREADS) void k_bake(BakeArgs A) { bake_texels<false>(A); }
extern "C" __global__ __launch_bounds__(RXR_TILE_THREADS) void k_bake_s(BakeArgs A) { bake_texels<true>(A); }

namespace {

// the argument checks both entry points share; `who` starts the message
int bake_check(rxr_ctx *ctx, const char *who, const uint32_t *programs, uint32_t n, uint32_t width, uint32_t height) {
    const std::string w = who;
    if (n && !programs) return rxr_fail(ctx, RXR_ERR_INVALID, w + ": NULL program list");
    if (!width || !height || width > RXR_BAKE_MAX_DIM || height > RXR_BAKE_MAX_DIM)
        return rxr_fail(ctx, RXR_ERR_INVALID, w + ": width and height must lie in [1, " + std::to_string(RXR_BAKE_MAX_DIM) + "]");
    if ((uint64_t)n * width * height > RXR_BAKE_MAX_TEXELS)
        return rxr_fail(ctx, RXR_ERR_INVALID, w + ": more than " + std::to_string(RXR_BAKE_MAX_TEXELS) + " texels in one call");
    if (n && ctx->programs.empty()) return rxr_fail(ctx, RXR_ERR_INVALID, w + ": no shader set is resident (rxr_set_shaders)");
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t p = programs[i];
        auto refuse = [&](int code, const char *why) { return rxr_fail(ctx, code, w + ": programs[" + std::to_string(i) + "] = " + std::to_string(p) + ": " + why); };
        if (p >= ctx->programs.size()) return refuse(RXR_ERR_INVALID, "no such program in the resident set");
        if (ctx->programs[p].shade_entry == 0xFFFFFFFFu)
            return refuse(RXR_ERR_INVALID, "the program has no shade function (shade_index -1): Chunk::add_shader bakes nothing for it");
        if (const char *why = rxr_bake_refusal(ctx->program_field_reads[p], ctx->program_field_writes[p])) return refuse(RXR_ERR_UNSUPPORTED, why);
    }
    return RXR_OK;
}

// the whole bake into device arrays, queued on `s`
int bake_run(rxr_ctx *ctx, const uint32_t *programs, uint32_t n, uint32_t width, uint32_t height, float *dev_pixels, uint8_t *dev_rgba, hipStream_t s) {
    if (!ctx->h_bake_fault) {
        HIPCHK(ctx, hipHostMalloc((void **)&ctx->h_bake_fault, BAKE_FAULT_WORDS * sizeof(uint32_t), hipHostMallocDefault));
        memset(ctx->h_bake_fault, 0, BAKE_FAULT_WORDS * sizeof(uint32_t));
    }
    int rc;
    if (!ctx->d_bake_fault.p) {
        if ((rc = rxr_ensure(ctx, ctx->d_bake_fault, BAKE_FAULT_WORDS * sizeof(uint32_t))) != RXR_OK) return rc;
        HIPCHK(ctx, hipMemsetAsync(ctx->d_bake_fault.p, 0, BAKE_FAULT_WORDS * sizeof(uint32_t), ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    // the program list: appended to a ring in device memory that earlier, still queued bakes may be reading; when it is full
    // everything queued is waited for and the ring starts over.  The copy leaves page-locked memory of the same layout, so it is
    // asynchronous and the caller's array is free when this call returns.
    if (ctx->bake_jobs_used + n > ctx->bake_jobs_cap) {
        if ((rc = rxr_quiesce(ctx)) != RXR_OK) return rc;   // (bake_jobs_used = 0)
        if ((size_t)n > ctx->bake_jobs_cap) {
            const size_t words = std::max<size_t>(n, 65536);
            ctx->bake_jobs_cap = 0;
            if ((rc = rxr_ensure(ctx, ctx->d_bake_jobs, words * sizeof(uint32_t))) != RXR_OK) return rc;
            if (ctx->h_bake_jobs) HIPCHK(ctx, hipHostFree(ctx->h_bake_jobs));
            ctx->h_bake_jobs = nullptr;
            HIPCHK(ctx, hipHostMalloc((void **)&ctx->h_bake_jobs, words * sizeof(uint32_t), hipHostMallocDefault));
            ctx->bake_jobs_cap = words;
        }
    }
    uint32_t *h_jobs = ctx->h_bake_jobs + ctx->bake_jobs_used;
    uint32_t *d_jobs = (uint32_t *)ctx->d_bake_jobs.p + ctx->bake_jobs_used;
    ctx->bake_jobs_used += n;
    memcpy(h_jobs, programs, (size_t)n * sizeof(uint32_t));
    if ((rc = rxr_query_begin(ctx, ctx->lane[Q_BAKE], s)) != RXR_OK) return rc;  // (a bake on another stream: the fault words' host copy is refreshed in order)
    HIPCHK(ctx, hipMemcpyAsync(d_jobs, h_jobs, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    BakeArgs A{};
    A.vm_code = (const uint32_t *)ctx->d_vm_code.p;
    A.programs = (const DevProgram *)ctx->d_programs.p;
    A.patterns = (const DevPattern *)ctx->d_patterns.p;
    A.pattern_data = (const float *)ctx->d_pattern_data.p;
    A.palette = (const float *)ctx->d_palette.p;
    A.n_programs = (uint32_t)ctx->programs.size();
    A.n_patterns = ctx->n_patterns;
    A.n_normal_patterns = ctx->n_normal_patterns;
    A.n_palette = ctx->n_palette;
    A.jobs = d_jobs;
    A.width = width;
    A.height = height;
    A.texels = width * height;
    A.groups_per_job = (A.texels + RXR_TILE_THREADS - 1) / RXR_TILE_THREADS;
    A.pixels = (float4 *)dev_pixels;
    A.rgba = (uint32_t *)dev_rgba;
    A.fault = (uint32_t *)ctx->d_bake_fault.p;
    const dim3 grid(n * A.groups_per_job);   // (at most RXR_BAKE_MAX_TEXELS / 256 + n workgroups)
    hipLaunchKernelGGL(ctx->programs_static ? k_bake_s : k_bake, grid, dim3(RXR_TILE_THREADS), 0, s, A);
    ctx->last_bake_kernel = ctx->programs_static ? 2u : 1u;
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_bake_fault, ctx->d_bake_fault.p, BAKE_FAULT_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    return rxr_query_end(ctx, ctx->lane[Q_BAKE], s);
}

}  // namespace

// rxr_synchronize / rxr_bake_shaders, streams idle: the fault a bake left in the pinned words as status + message; clears them
int rxr_bake_report_fault(rxr_ctx *ctx) {
    static const char *const what[] = {"", "stack underflow", "stack overflow", "local index out of range", "global index out of range",
                                       "call depth", "loop depth", "instruction limit (runaway loop)", "clamp with min > max",
                                       "call of a missing function", "bad opcode", "too many locals"};
    uint32_t w[BAKE_FAULT_WORDS];
    memcpy(w, ctx->h_bake_fault, sizeof(w));
    memset(ctx->h_bake_fault, 0, sizeof(w));
    HIPCHK(ctx, hipMemsetAsync(ctx->d_bake_fault.p, 0, sizeof(w), ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    const uint32_t code = w[BAKE_FAULT_CODE];
    return rxr_fail(ctx, RXR_ERR_INVALID,
                    std::string("bake: shader program fault: ") + (code < sizeof(what) / sizeof(what[0]) ? what[code] : "?") + " in program " +
                        std::to_string(w[BAKE_FAULT_PROGRAM]) + " (bake " + std::to_string(w[BAKE_FAULT_JOB]) + " of the call) at texel (" +
                        std::to_string(w[BAKE_FAULT_X]) + ", " + std::to_string(w[BAKE_FAULT_Y]) + ")");
}

extern "C" {

int rxr_bake_shaders(rxr_ctx *ctx, const uint32_t *programs, uint32_t n, uint32_t width, uint32_t height, float *pixels, uint8_t *rgba) {
    if (!ctx) return RXR_ERR_INVALID;
    if (ctx->group) return rxr_as_member0(ctx, [&](rxr_ctx *m) { return rxr_bake_shaders(m, programs, n, width, height, pixels, rgba); });
    int rc = bake_check(ctx, "rxr_bake_shaders", programs, n, width, height);
    if (rc != RXR_OK) return rc;
    if (!n) return RXR_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t texels = (size_t)n * width * height;
    QueryIO io{ctx, ctx->lane[Q_BAKE]};
    const unsigned i_px = io.out(pixels, texels * 16), i_rgba = io.out(rgba, texels * 4);
    if ((rc = io.upload()) != RXR_OK) return rc;
    if ((rc = bake_run(ctx, programs, n, width, height, io.dev<float>(i_px), io.dev<uint8_t>(i_rgba), ctx->stream)) != RXR_OK) return rc;
    if ((rc = io.download()) != RXR_OK) return rc;
    if (ctx->h_bake_fault[BAKE_FAULT_CODE]) return rxr_bake_report_fault(ctx);
    return RXR_OK;
}

int rxr_bake_shaders_to(rxr_ctx *ctx, const uint32_t *programs, uint32_t n, uint32_t width, uint32_t height, float *dev_pixels,
                        uint8_t *dev_rgba, void *hip_stream) {
    if (!ctx) return RXR_ERR_INVALID;
    if (ctx->group) return rxr_fail(ctx, RXR_ERR_UNSUPPORTED, "rxr_bake_shaders_to on a multi-device context: device pointers and streams belong to ONE device (use rxr_member)");
    int rc = bake_check(ctx, "rxr_bake_shaders_to", programs, n, width, height);
    if (rc != RXR_OK) return rc;
    if (!n || (!dev_pixels && !dev_rgba)) return RXR_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t texels = (size_t)n * width * height;
    if (((uintptr_t)dev_pixels & 15u) || ((uintptr_t)dev_rgba & 3u))
        return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_bake_shaders_to: dev_pixels must be 16-byte aligned and dev_rgba 4-byte aligned");
    if ((dev_pixels && !rxr_on_device(ctx, dev_pixels, texels * 16)) || (dev_rgba && !rxr_on_device(ctx, dev_rgba, texels * 4)))
        return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_bake_shaders_to: an output array is not device memory of the context's device (or is too small)");
    return bake_run(ctx, programs, n, width, height, dev_pixels, dev_rgba, hip_stream ? (hipStream_t)hip_stream : ctx->stream);
}

// tests: the kernel of the context's most recent bake launch -- 1 k_bake (per-lane stack depths), 2 k_bake_s (static depths), 0 when
// the context has launched no bake; a multi-device handle answers for member 0
uint32_t rxr_debug_last_bake_kernel(rxr_ctx *ctx) {
    if (ctx && ctx->group) ctx = rxr_member(ctx, 0);
    return ctx ? ctx->last_bake_kernel : 0u;
}

}  // extern "C"
