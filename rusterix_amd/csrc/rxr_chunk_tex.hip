// rxr_chunk_tex.hip -- resident chunk textures (include/rxr.h: rxr_check_chunk_textures, rxr_set_chunk_textures,
// rxr_update_chunk_textures(_to), rxr_read_chunk_texture).  chunk.terrain_texture and chunk.shader_textures (src/chunk.rs:36, :53) are
// registered once into a pool of their own and rewritten in place from device memory -- the layout rxr_bake_terrain_to and
// rxr_bake_shaders_to write -- instead of crossing the ABI in every rxr_upload_frame.  The raster kernels do not know: a frame's
// DevTexDesc table names the pool through RasterParams.frame_texels exactly as it names the frame blob's own texels (rxr_upload.hip).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "rxr_debug.h"
#include "rxr_query.h"

// One launch: at most RXR_CHUNK_TEX_LAUNCH sources, each copied into its slot in segments of RXR_CHUNK_TEX_SEGMENT texels.  Everything the
// kernel needs travels in its arguments (3 KiB): a queued launch reads no memory the caller can change but the sources themselves.
#define RXR_CHUNK_TEX_LAUNCH 256u
#define RXR_CHUNK_TEX_SEGMENT 4096u     // texels: 16 KiB, four 16-byte accesses (or sixteen dword accesses) per lane of a 256-lane workgroup
#define RXR_CHUNK_TEX_GRID_X 1024u      // segments of one source in flight; a larger source strides

struct ChunkTexArgs {
    const uint32_t *src;      // the launch's sources, back to back (4-byte aligned)
    uint32_t *pool;           // the resident pool (16-byte aligned)
    uint32_t *flags;          // one word per source of this launch, 1 when the launch starts
    uint32_t n;
    uint32_t texels[RXR_CHUNK_TEX_LAUNCH];    // per source: w * h
    uint32_t src_off[RXR_CHUNK_TEX_LAUNCH];   // ... its first texel, from src
    uint32_t dst_off[RXR_CHUNK_TEX_LAUNCH];   // ... its slot's first texel, from pool (a multiple of four)
};

// blockIdx.y: the source; blockIdx.x, strided by gridDim.x: its segments.  A segment starts a multiple of RXR_CHUNK_TEX_SEGMENT texels
// into its slot, so its destination is 16-byte aligned; where its source is too, whole groups of four texels move as 16-byte accesses
// (1 KiB per wave instruction, four independent loads per lane in flight) and the up to three texels behind them as dwords; a
// source that is only 4-byte aligned (it follows a source whose texel count is no multiple of four) moves as dwords throughout.  The
// decision is workgroup-uniform.  The flag: a wave that has loaded a texel with alpha != 255 stores 0 -- every writer writes the same
// value over the 1 the host put there, so no atomic is needed.
extern "C" __global__ void __launch_bounds__(256) k_chunk_tex_commit(const ChunkTexArgs A) {
    const uint32_t e = blockIdx.y;
    const uint32_t n_tex = A.texels[e];
    const uint32_t *const src_e = A.src + A.src_off[e];
    uint32_t *const dst_e = A.pool + A.dst_off[e];
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    for (uint32_t t0 = blockIdx.x * RXR_CHUNK_TEX_SEGMENT; t0 < n_tex; t0 += gridDim.x * RXR_CHUNK_TEX_SEGMENT) {
        const uint32_t n = min(n_tex - t0, RXR_CHUNK_TEX_SEGMENT);
        const uint32_t *src = src_e + t0;
        uint32_t *dst = dst_e + t0;
        uint32_t alpha = 0xFF000000u;   // the AND of every texel this lane has loaded
        uint32_t done = 0;              // texels moved by the 16-byte body
        if (((uintptr_t)src & 15u) == 0u) {
            const uint32_t n16 = n >> 2;
            u32x4 v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t i = (uint32_t)k * 256u + threadIdx.x;
                v[k] = i < n16 ? __builtin_nontemporal_load((const u32x4 *)src + i) : (u32x4)(0xFF000000u);
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t i = (uint32_t)k * 256u + threadIdx.x;
                if (i < n16) ((u32x4 *)dst)[i] = v[k];
                alpha &= v[k].x & v[k].y & v[k].z & v[k].w;
            }
            done = n16 << 2;
            if (threadIdx.x < n - done) {   // the tail: at most three texels
                const uint32_t w = src[done + threadIdx.x];
                dst[done + threadIdx.x] = w;
                alpha &= w;
            }
        } else {
            uint32_t v[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const uint32_t i = (uint32_t)k * 256u + threadIdx.x;
                v[k] = i < n ? __builtin_nontemporal_load(src + i) : 0xFF000000u;
            }
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const uint32_t i = (uint32_t)k * 256u + threadIdx.x;
                if (i < n) dst[i] = v[k];
                alpha &= v[k];
            }
        }
        if (__ballot((alpha >> 24) != 255u) != 0ull && (threadIdx.x & 63u) == 0u) A.flags[e] = 0u;
    }
}

namespace {

// the registration's shape, or why there is none
struct ChunkTexShape {
    std::vector<ChunkTextures::Slot> slots;
    size_t pool_texels = 0;   // padded
};

int check_chunk_textures(const rxr_texture *textures, uint32_t n_textures, const int32_t *chunk_terrain, const uint32_t *chunk_shader_first,
                         const int32_t *chunk_shader_slots, uint32_t n_chunks, ChunkTexShape &shape, std::string &err) {
    auto fail = [&](const std::string &why) {
        err = why;
        return (int)RXR_ERR_INVALID;
    };
    if (n_textures && !textures) return fail("NULL textures with n_textures > 0");
    if (n_chunks && (!chunk_terrain || !chunk_shader_first)) return fail("NULL chunk_terrain / chunk_shader_first with n_chunks > 0");
    size_t texels = 0, padded = 0;
    shape.slots.resize(n_textures);
    for (uint32_t i = 0; i < n_textures; ++i) {
        const rxr_texture &t = textures[i];
        const std::string at = "textures[" + std::to_string(i) + "]";
        if (t.width == 0 || t.height == 0) return fail(at + ": a side of 0 texels");
        if (t.width > 32768 || t.height > 32768) return fail(at + ": a side above 32768 texels");
        const size_t n = (size_t)t.width * t.height;
        texels += n;
        if (texels >= (1ull << 31)) return fail(at + ": chunk textures too large (2^31 texels or more in all)");
        if (padded + align_up(n, 4) >= (1ull << 32)) return fail(at + ": too many slots (the padded pool would reach 2^32 texels)");
        shape.slots[i] = ChunkTextures::Slot{t.width, t.height, (uint32_t)padded, 0u};
        padded += align_up(n, 4);
    }
    shape.pool_texels = padded;
    for (uint32_t c = 0; c < n_chunks; ++c) {
        const int32_t s = chunk_terrain[c];
        if (s < -1 || (s >= 0 && (uint32_t)s >= n_textures))
            return fail("chunk_terrain[" + std::to_string(c) + "] = " + std::to_string(s) + ": slot out of range (" + std::to_string(n_textures) + " slots)");
    }
    if (n_chunks) {
        if (chunk_shader_first[0] != 0u) return fail("chunk_shader_first[0] is not 0");
        for (uint32_t c = 0; c < n_chunks; ++c)
            if (chunk_shader_first[c + 1] < chunk_shader_first[c]) return fail("chunk_shader_first[" + std::to_string(c + 1) + "]: the prefix decreases");
        const uint32_t n_entries = chunk_shader_first[n_chunks];
        if (n_entries && !chunk_shader_slots) return fail("NULL chunk_shader_slots with shader entries");
        for (uint32_t k = 0; k < n_entries; ++k) {
            const int32_t s = chunk_shader_slots[k];
            if (s < -1 || (s >= 0 && (uint32_t)s >= n_textures))
                return fail("chunk_shader_slots[" + std::to_string(k) + "] = " + std::to_string(s) + ": slot out of range (" + std::to_string(n_textures) + " slots)");
        }
    }
    return RXR_OK;
}

// `n` sources, back to back at device address `src` in the order of `slots`, into their places in `pool`; flags come back into
// slot_table[slots[i]].opaque.  Queued on `s`, which is synchronised before this returns.
int commit_run(rxr_ctx *ctx, std::vector<ChunkTextures::Slot> &slot_table, uint32_t *pool, const uint32_t *slots, uint32_t n, const uint8_t *src, hipStream_t s) {
    ChunkTextures &T = ctx->ctex;
    int rc = rxr_ensure(ctx, T.flags, std::max<size_t>((size_t)n * 4, 256));
    if (rc != RXR_OK) return rc;
    HIPCHK(ctx, hipMemsetD32Async((hipDeviceptr_t)T.flags.p, 1, n, s));
    T.launches = 0;
    size_t at = 0;   // texels from src
    ChunkTexArgs A{};
    A.pool = pool;
    for (uint32_t c0 = 0; c0 < n; c0 += RXR_CHUNK_TEX_LAUNCH) {
        const uint32_t nc = std::min(n - c0, RXR_CHUNK_TEX_LAUNCH);
        A.src = (const uint32_t *)src + at;
        A.flags = (uint32_t *)T.flags.p + c0;
        A.n = nc;
        uint32_t off = 0, most = 1;
        for (uint32_t i = 0; i < nc; ++i) {
            const ChunkTextures::Slot &S = slot_table[slots[c0 + i]];
            A.texels[i] = S.w * S.h;
            A.src_off[i] = off;
            A.dst_off[i] = S.offset;
            off += A.texels[i];
            most = std::max(most, (A.texels[i] + RXR_CHUNK_TEX_SEGMENT - 1u) / RXR_CHUNK_TEX_SEGMENT);
        }
        at += off;
        hipLaunchKernelGGL(k_chunk_tex_commit, dim3(std::min(most, RXR_CHUNK_TEX_GRID_X), nc), dim3(256), 0, s, A);
        HIPCHK(ctx, hipGetLastError());
        ++T.launches;
    }
    std::vector<uint32_t> flags(n);
    HIPCHK(ctx, hipMemcpyAsync(flags.data(), T.flags.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    for (uint32_t i = 0; i < n; ++i) slot_table[slots[i]].opaque = flags[i] ? 1u : 0u;
    return RXR_OK;
}

// what both update forms refuse before anything is queued, but for their pointers; bytes: the sources' size
int update_check(rxr_ctx *ctx, const char *who, const uint32_t *slots, uint32_t n, size_t &bytes) {
    const std::string w = who;
    const ChunkTextures &T = ctx->ctex;
    if (!T.set) return rxr_fail(ctx, RXR_ERR_INVALID, w + ": no registration (rxr_set_chunk_textures)");
    if (!slots) return rxr_fail(ctx, RXR_ERR_INVALID, w + ": NULL slots");
    std::vector<uint8_t> named(T.slots.size(), 0);
    bytes = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const std::string at = w + ": slots[" + std::to_string(i) + "] = " + std::to_string(slots[i]);
        if (slots[i] >= T.slots.size()) return rxr_fail(ctx, RXR_ERR_INVALID, at + ": no such slot (" + std::to_string(T.slots.size()) + " are registered)");
        if (named[slots[i]]) return rxr_fail(ctx, RXR_ERR_INVALID, at + ": named twice");
        named[slots[i]] = 1;
        bytes += (size_t)T.slots[slots[i]].w * T.slots[slots[i]].h * 4;
    }
    return RXR_OK;
}

// the caller's host texels, back to back, in the lane's device buffer (through the pinned staging blob; the streams are idle)
int stage_sources(rxr_ctx *ctx, const uint8_t *const *rgba, const size_t *bytes, uint32_t n, size_t total, const uint8_t *&dev) {
    QueryLane &lane = ctx->lane[Q_CHUNK_TEX];
    int rc;
    if ((rc = rxr_ensure_stage(ctx, total)) != RXR_OK) return rc;
    if ((rc = rxr_ensure(ctx, lane.io, std::max<size_t>(total, 256))) != RXR_OK) return rc;
    uint8_t *st = (uint8_t *)ctx->h_stage;
    size_t at = 0;
    for (uint32_t i = 0; i < n; ++i) {
        memcpy(st + at, rgba[i], bytes[i]);
        at += bytes[i];
    }
    HIPCHK(ctx, hipMemcpyAsync(lane.io.p, st, total, hipMemcpyHostToDevice, ctx->stream));
    dev = (const uint8_t *)lane.io.p;
    return RXR_OK;
}

}  // namespace

extern "C" {

int rxr_check_chunk_textures(const rxr_texture *textures, uint32_t n_textures, const int32_t *chunk_terrain, const uint32_t *chunk_shader_first,
                             const int32_t *chunk_shader_slots, uint32_t n_chunks, char *message, uint32_t message_capacity) {
    ChunkTexShape shape;
    std::string err;
    const int rc = check_chunk_textures(textures, n_textures, chunk_terrain, chunk_shader_first, chunk_shader_slots, n_chunks, shape, err);
    rxr_copy_message(err, message, message_capacity);
    return rc;
}

int rxr_set_chunk_textures(rxr_ctx *ctx, const rxr_texture *textures, uint32_t n_textures, const int32_t *chunk_terrain, const uint32_t *chunk_shader_first,
                           const int32_t *chunk_shader_slots, uint32_t n_chunks) {
    if (!ctx) return RXR_ERR_INVALID;
    ChunkTexShape shape;
    std::string err;
    int rc = check_chunk_textures(textures, n_textures, chunk_terrain, chunk_shader_first, chunk_shader_slots, n_chunks, shape, err);
    if (rc != RXR_OK) return rxr_fail(ctx, rc, "rxr_set_chunk_textures: " + err);
    if (ctx->group)   // (the refusals above depend on the arguments alone: all members accept or all refuse)
        return rxr_group_each(ctx, [&](rxr_ctx *m) { return rxr_set_chunk_textures(m, textures, n_textures, chunk_terrain, chunk_shader_first, chunk_shader_slots, n_chunks); });
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if ((rc = rxr_quiesce(ctx)) != RXR_OK) return rc;   // renders read the pool that is replaced here
    ChunkTextures &T = ctx->ctex;
    if (n_chunks == 0) {   // the registration is removed: frames carry their chunk textures again
        T.set = false;
        T.slots.clear();
        T.terrain.clear();
        T.shader_first.clear();
        T.shader_slots.clear();
        ctx->has_frame = false;
        ctx->trace_set = false;   // (rxr_trace.hip: its terrain records name slots of the pool)
        return RXR_OK;
    }
    // a pool of its own first: until everything has succeeded the previous registration stays as it was
    DevBuf pool;
    pool.cap = std::max<size_t>(shape.pool_texels * 4, 256);
    {
        const hipError_t e = hipMalloc(&pool.p, pool.cap);
        if (e != hipSuccess) return rxr_fail(ctx, RXR_ERR_OOM, std::string("rxr_set_chunk_textures: hipMalloc: ") + hipGetErrorString(e));
    }
    auto give_up = [&](int code) {
        (void)hipStreamSynchronize(ctx->stream);
        (void)hipFree(pool.p);
        return code;
    };
    // a slot without bytes is zeros (not opaque) until an update writes it; the others go through the kernel, which also makes their flags
    if (hipMemsetAsync(pool.p, 0, pool.cap, ctx->stream) != hipSuccess) return give_up(rxr_fail(ctx, RXR_ERR_HIP, "rxr_set_chunk_textures: hipMemsetAsync failed"));
    std::vector<uint32_t> given;
    std::vector<const uint8_t *> rgba;
    std::vector<size_t> bytes;
    size_t total = 0;
    for (uint32_t i = 0; i < n_textures; ++i)
        if (textures[i].rgba) {
            given.push_back(i);
            rgba.push_back(textures[i].rgba);
            bytes.push_back((size_t)textures[i].width * textures[i].height * 4);
            total += bytes.back();
        }
    if (!given.empty()) {
        const uint8_t *dev = nullptr;
        if ((rc = stage_sources(ctx, rgba.data(), bytes.data(), (uint32_t)given.size(), total, dev)) != RXR_OK) return give_up(rc);
        if ((rc = commit_run(ctx, shape.slots, (uint32_t *)pool.p, given.data(), (uint32_t)given.size(), dev, ctx->stream)) != RXR_OK) return give_up(rc);
    } else {
        T.launches = 0;
    }
    if (hipStreamSynchronize(ctx->stream) != hipSuccess) return give_up(rxr_fail(ctx, RXR_ERR_HIP, "rxr_set_chunk_textures: hipStreamSynchronize failed"));
    if (T.pool.p) (void)hipFree(T.pool.p);
    T.pool = pool;
    T.slots = std::move(shape.slots);
    T.terrain.assign(chunk_terrain, chunk_terrain + n_chunks);
    T.shader_first.assign(chunk_shader_first, chunk_shader_first + n_chunks + 1);
    T.shader_slots.assign(chunk_shader_slots, chunk_shader_slots + (chunk_shader_first[n_chunks] ? chunk_shader_first[n_chunks] : 0u));
    T.set = true;
    ctx->trace_set = false;
    ctx->has_frame = false;   // (the resident frame names the frame blob's texels, or the pool that was just freed)
    return RXR_OK;
}

int rxr_update_chunk_textures(rxr_ctx *ctx, const uint32_t *slots, uint32_t n, const uint8_t *rgba) {
    if (!ctx) return RXR_ERR_INVALID;
    if (ctx->group) return rxr_group_each(ctx, [&](rxr_ctx *m) { return rxr_update_chunk_textures(m, slots, n, rgba); });   // (every member holds the same registration)
    size_t bytes = 0;
    int rc = update_check(ctx, "rxr_update_chunk_textures", slots, n, bytes);
    if (rc != RXR_OK) return rc;
    if (!n) return RXR_OK;
    if (!rgba) return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_update_chunk_textures: NULL rgba");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if ((rc = rxr_quiesce(ctx)) != RXR_OK) return rc;   // renders read the pool
    const uint8_t *dev = nullptr;
    if ((rc = stage_sources(ctx, &rgba, &bytes, 1, bytes, dev)) != RXR_OK) return rc;
    rc = commit_run(ctx, ctx->ctex.slots, (uint32_t *)ctx->ctex.pool.p, slots, n, dev, ctx->stream);
    if (rc != RXR_OK) (void)hipStreamSynchronize(ctx->stream);   // (the staging blob has been read before the call returns)
    ctx->has_frame = false;   // (the headers' alpha decisions came from the old flags)
    return rc;
}

int rxr_update_chunk_textures_to(rxr_ctx *ctx, const uint32_t *slots, uint32_t n, const uint8_t *dev_rgba, void *hip_stream) {
    if (!ctx) return RXR_ERR_INVALID;
    if (ctx->group) return rxr_fail(ctx, RXR_ERR_UNSUPPORTED, "rxr_update_chunk_textures_to on a multi-device context: device pointers and streams belong to ONE device (use rxr_member)");
    size_t bytes = 0;
    int rc = update_check(ctx, "rxr_update_chunk_textures_to", slots, n, bytes);
    if (rc != RXR_OK) return rc;
    if (!n) return RXR_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (!dev_rgba || ((uintptr_t)dev_rgba & 3u)) return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_update_chunk_textures_to: dev_rgba must be 4-byte aligned device memory");
    if (!rxr_on_device(ctx, dev_rgba, bytes)) return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_update_chunk_textures_to: dev_rgba is not device memory of the context's device (or is too small)");
    if ((rc = rxr_quiesce(ctx)) != RXR_OK) return rc;   // renders read the pool
    rc = commit_run(ctx, ctx->ctex.slots, (uint32_t *)ctx->ctex.pool.p, slots, n, dev_rgba, hip_stream ? (hipStream_t)hip_stream : ctx->stream);
    ctx->has_frame = false;
    return rc;
}

int rxr_read_chunk_texture(rxr_ctx *ctx, uint32_t slot, uint32_t size[2], uint32_t *all_opaque, uint8_t *rgba) {
    if (!ctx) return RXR_ERR_INVALID;
    if (ctx->group) return rxr_as_member0(ctx, [&](rxr_ctx *m) { return rxr_read_chunk_texture(m, slot, size, all_opaque, rgba); });
    const ChunkTextures &T = ctx->ctex;
    if (!T.set || slot >= T.slots.size()) return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_read_chunk_texture: no such slot");
    const ChunkTextures::Slot &S = T.slots[slot];
    if (size) {
        size[0] = S.w;
        size[1] = S.h;
    }
    if (all_opaque) *all_opaque = S.opaque;
    if (rgba) {
        HIPCHK(ctx, hipSetDevice(ctx->device));
        HIPCHK(ctx, hipMemcpyAsync(rgba, (const uint32_t *)T.pool.p + S.offset, (size_t)S.w * S.h * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    return RXR_OK;
}

// tests: the kernel's constants (sources per launch, texels per segment, segments of one source in flight) and the
// k_chunk_tex_commit launches of the last registration or update
void rxr_debug_chunk_tex_constants(uint32_t out[3]) {
    out[0] = RXR_CHUNK_TEX_LAUNCH;
    out[1] = RXR_CHUNK_TEX_SEGMENT;
    out[2] = RXR_CHUNK_TEX_GRID_X;
}
uint32_t rxr_debug_chunk_tex_launches(rxr_ctx *ctx) {
    if (!ctx) return 0;
    if (ctx->group) return rxr_debug_chunk_tex_launches(rxr_member(ctx, 0));
    return ctx->ctex.launches;
}

}  // extern "C"
