// rxr_upload.hip -- the frame hand-over of the C ABI (include/rxr.h; host side, compiled by hipcc).  rxr_upload_frame validates the projected
// frame, packs every per-frame array into ONE pinned staging blob and issues ONE host->device copy (large frames: pipelined in groups under
// the worker pool's copies); rxr_stream_* hand the 3D batches over while they are still being projected.  No CPU fallback anywhere.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <cmath>
#include <thread>
#include <cstdio>
#include <cstring>

#include "../../include/rusterix_vek.hpp"  // host-side Mat4 products for the device-projection path
#include "rxr_ctx.h"
#include "rxr_host_setup.h"
#include "rxr_parallel.h"

extern "C" uint32_t rxr_span_meshes_max(void);

namespace {

// Rust `x as isize` narrowed to i32 for the Bresenham end points (rasterizer.rs:1785-1788);
// coordinates beyond +-2^30 are rejected at upload (the walk would not terminate in a frame's time), and so is NaN: `NaN as isize` is 0,
// a point OUTSIDE the batch's bounding box (f32::min / max drop NaN, batch2d.rs:377-403), and the reference skips a batch for every
// tile its box does not meet (:594-600) -- which pixels of such a segment it draws depends on its tile size (found by
// tests/test_gpu_special_2d.py); the caller's CPU path draws it
bool to_isize32(float x, int32_t &out) {
    if (!(x == x)) {
        out = 0;
        return false;
    }
    if (x <= -1073741824.0f || x >= 1073741824.0f) return false;
    out = (int32_t)x;
    return true;
}

// `x as u32` (Rust: saturating, NaN -> 0), as the device's sat_u32
static uint32_t rust_as_u32(float x) {
    if (!(x > 0.0f)) return 0u;
    if (x >= 4294967296.0f) return 0xFFFFFFFFu;
    return (uint32_t)x;
}

// The LightFast record of one light (rxr_device.h): the fragment-independent factors of the relaxed point-light term, by the
// reference's own operations (CompiledLight::apply_flicker, light.rs:506-527; smoothstep(end, start, d), light.rs:545).
static void light_fast_record(const rxr_light &l, uint32_t hash_anim, LightFast &out) {
    memset(&out, 0, sizeof(out));
    memcpy(out.pos, l.position, 12);
    out.end_distance = l.end_distance;
    out.cull_kind = (l.light_type == RXR_LIGHT_POINT || l.light_type == RXR_LIGHT_SPOT || l.light_type == RXR_LIGHT_AREA || l.light_type == RXR_LIGHT_DAYLIGHT) ? 1u : 0u;
    const float ssd = l.start_distance - l.end_distance;
    const float a = std::fabs(ssd);
    // (the window of rxr_exact_math.h: 2^-40 .. 2^40; the fused form also wants start < end, as every real light has it)
    if (l.light_type != RXR_LIGHT_POINT || !l.emitting || !(a >= 0x1p-40f && a <= 0x1p40f) || !(l.start_distance < l.end_distance)) return;
    float ff = 1.0f;
    if (l.flicker > 0.0f) {
        const uint32_t combined = hash_anim + (rust_as_u32(l.position[0]) + rust_as_u32(l.position[1]) + rust_as_u32(l.position[2])) * 100u;
        float fv = (float)combined / 4294967296.0f;
        fv = fv < 0.0f ? 0.0f : (fv > 1.0f ? 1.0f : fv);
        ff = 1.0f - fv * l.flicker;
    }
    out.ss_r = 1.0f / ssd;
    out.c0 = -l.end_distance * out.ss_r;
    for (int k = 0; k < 3; ++k) out.cfi[k] = l.color[k] * l.intensity * ff;
}

struct Layout {
    size_t off_b3, off_base, off_pv, off_uv, off_nrm, off_idx, off_edges, off_tinfo, off_host_setup, off_host_shade, off_clip3d, off_lights, off_lights_fast, off_occ, off_ld, off_chunks, off_tdesc,
        off_ltex, off_b2, off_p2, off_bg, total;
};

// resolves a PixelSource to (tex index | constant texel); see include/rxr.h RXR_SOURCE_*
static int resolve_source(rxr_ctx *ctx, const rxr_source &src, bool is_3d, int chunk, uint64_t animation_frame, int32_t &tex,
                          uint32_t &pixel) {
    tex = -1;
    pixel = 0;
    auto from_tiles = [&](const std::vector<TileRange> &tiles) -> int {
        if (src.index >= tiles.size()) {
            if (is_3d) return RXR_ERR_INVALID;  // tile_list[index] panics, rasterizer.rs:1103
            pixel = 0;                          // 2D uses .get(): [0,0,0,0], :685-687
            return RXR_OK;
        }
        const TileRange &r = tiles[src.index];
        if (r.n == 0) return RXR_ERR_INVALID;  // `% 0` panics
        tex = (int32_t)(r.first + (uint32_t)(animation_frame % r.n));
        return RXR_OK;
    };
    switch (src.kind) {
        case RXR_SOURCE_STATIC_TILE: return from_tiles(ctx->tiles_static);
        case RXR_SOURCE_DYNAMIC_TILE: return from_tiles(ctx->tiles_dynamic);
        case RXR_SOURCE_PIXEL: pixel = pack_px(src.pixel); return RXR_OK;
        case RXR_SOURCE_MISSING: pixel = 0; return RXR_OK;
        case RXR_HOST_SOURCE_ENTITY_TILE:
        case RXR_HOST_SOURCE_ITEM_TILE: return RXR_ERR_INVALID;  // host-side variants: the host resolves them (include/rxr.h)
        case RXR_SOURCE_TERRAIN:
            if (chunk >= 0) pixel = 0;                       // chunk without a terrain texture, chunk.rs:150
            else pixel = is_3d ? 0xFF0000FFu : 0u;           // [255,0,0,255] (:1218) | [0,0,0,0] (:753)
            return RXR_OK;
        default: pixel = is_3d ? 0xFF000000u : 0u; return RXR_OK;  // [0,0,0,255] (:1221) | [0,0,0,0] (:757)
    }
}

// the frame blob up to the end of the projected arrays: headers, triangle bases, then the five pools (n_v vertices, n_t triangles)
BlobCursor layout_prefix(size_t n_b3, size_t n_v, size_t n_t, Layout &L) {
    BlobCursor take;
    L.off_b3 = take(n_b3 * sizeof(DevBatch));
    L.off_base = take((n_b3 + 1) * sizeof(uint32_t));
    L.off_pv = take(n_v * 16);
    L.off_uv = take(n_v * 8);
    L.off_nrm = take(n_v * 12);
    L.off_idx = take(n_t * 12);
    L.off_edges = take(n_t * sizeof(rxr_edges));
    return take;
}

}  // namespace

// rxr_stream_begin_pinned: the device pulls a group of batches out of the host's own (page-locked) arrays.  One workgroup per 16 KB
// piece; an entry's pieces are consecutive (first_piece), the workgroup finds its entry by bisection in the (pinned) table.  Sources
// and destinations are 4-byte aligned (destinations are v0 * 12 / t0 * 12 bytes into a pool): dword copies, 256 bytes per wave
// instruction, sixteen independent loads per lane in flight over PCIe.
#define RXR_GATHER_PIECE 16384u
extern "C" __global__ void __launch_bounds__(256) k_gather_host(const FrameStream::GatherEntry *entries, uint32_t n_entries, uint8_t *blob) {
    const uint32_t piece = blockIdx.x;
    uint32_t lo = 0, hi = n_entries;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (entries[mid].first_piece <= piece) lo = mid;
        else hi = mid;
    }
    const FrameStream::GatherEntry E = entries[lo];
    const uint32_t at = (piece - E.first_piece) * RXR_GATHER_PIECE;  // byte offset of this piece inside the entry
    const uint32_t n_bytes = min(E.bytes - at, RXR_GATHER_PIECE);
    const uint8_t *src = (const uint8_t *)E.src + at;
    uint8_t *dst = blob + E.dst_off + at;
    if ((((uintptr_t)src | (uintptr_t)dst | n_bytes) & 15u) == 0u) {
        // (workgroup-uniform) both ends 16-byte aligned -- the projected vertices always are: 1 KB per wave instruction
        const uint32_t n16 = n_bytes >> 4;
        typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
        u32x4 v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t i = (uint32_t)k * 256u + threadIdx.x;
            v[k] = i < n16 ? __builtin_nontemporal_load((const u32x4 *)src + i) : (u32x4)(0u);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t i = (uint32_t)k * 256u + threadIdx.x;
            if (i < n16) ((u32x4 *)dst)[i] = v[k];
        }
        return;
    }
    const uint32_t n_dw = n_bytes >> 2;
    uint32_t v[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const uint32_t i = (uint32_t)k * 256u + threadIdx.x;
        v[k] = i < n_dw ? __builtin_nontemporal_load((const uint32_t *)src + i) : 0u;
    }
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const uint32_t i = (uint32_t)k * 256u + threadIdx.x;
        if (i < n_dw) ((uint32_t *)dst)[i] = v[k];
    }
}

extern "C" {

void *rxr_alloc_pinned(size_t bytes) {
    void *p = nullptr;
    if (rxr_device_count() <= 0 || hipHostMalloc(&p, bytes ? bytes : 16, hipHostMallocPortable | hipHostMallocMapped) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    return p;
}
void rxr_free_pinned(void *ptr) {
    if (ptr) (void)hipHostFree(ptr);
}

static int stream_begin(rxr_ctx *ctx, uint32_t n_batches3d, const uint32_t *vertex_capacity, const uint32_t *triangle_capacity, bool pinned) {
    if (!ctx) return RXR_ERR_INVALID;
    if (ctx->group) return rxr_fail(ctx, RXR_ERR_UNSUPPORTED, "rxr_stream_begin on a multi-device context: hand the frame over with rxr_upload_frame");
    FrameStream &S = ctx->fstream;
    S.active = false;
    if (n_batches3d == 0 || !vertex_capacity || !triangle_capacity) return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_stream_begin: no batches / NULL capacities");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    size_t cv = 0, ct = 0;
    for (uint32_t i = 0; i < n_batches3d; ++i) {
        cv += vertex_capacity[i];
        ct += triangle_capacity[i];
    }
    if (cv >= (1ull << 31) || ct >= (1ull << 31)) return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_stream_begin: frame too large (>= 2^31 vertices or triangles)");
    Layout L{};
    const size_t prefix = layout_prefix(n_batches3d, cv, ct, L).o;
    // what follows the arrays in the blob (lights, 2D primitives, chunk textures ...) is only known at rxr_upload_frame: room for what
    // the last frame needed plus a margin; a frame that needs more falls back to the plain hand-over there
    const size_t tail_room = std::max<size_t>(16u << 20, 2 * ctx->last_blob_tail);
    int rc;
    // the previous frame's renders read the blob, its transfers the staging memory: nothing of that may still run
    if ((rc = rxr_quiesce(ctx)) != RXR_OK) return rc;
    if ((rc = rxr_ensure_stage(ctx, prefix + tail_room)) != RXR_OK) return rc;
    if ((rc = rxr_ensure(ctx, ctx->d_frame, prefix + tail_room)) != RXR_OK) return rc;
    S.n = n_batches3d;
    S.rec.assign(n_batches3d, FrameStream::Rec{});
    S.cap_v.assign(vertex_capacity, vertex_capacity + n_batches3d);
    S.cap_t.assign(triangle_capacity, triangle_capacity + n_batches3d);
    S.done.reset(new std::atomic<uint8_t>[n_batches3d]);
    for (uint32_t i = 0; i < n_batches3d; ++i) S.done[i].store(0, std::memory_order_relaxed);
    // few, large transfers (every hipMemcpyAsync costs its caller ~20 us): eight groups of consecutive batches
    static const uint32_t n_groups_wanted = []() {
        const char *e = getenv("RXR_STREAM_GROUPS");   // (tuning: tools/e2e_probe.py)
        const int v = e ? atoi(e) : 0;
        return (uint32_t)(v >= 1 && v <= 256 ? v : 8);
    }();
    S.group_size = std::max<uint32_t>(1u, (n_batches3d + n_groups_wanted - 1u) / n_groups_wanted);
    S.n_groups = (n_batches3d + S.group_size - 1u) / S.group_size;
    S.group_left.reset(new std::atomic<uint32_t>[S.n_groups]);
    for (uint32_t g = 0; g < S.n_groups; ++g) S.group_left[g].store(std::min(S.group_size, n_batches3d - g * S.group_size), std::memory_order_relaxed);
    S.next = 0;
    S.retired.store(0);
    S.copy_next.store(0);
    S.vcur = S.tcur = 0;
    S.total_cap_v = cv;
    S.total_cap_t = ct;
    S.off_pv = L.off_pv; S.off_uv = L.off_uv; S.off_nrm = L.off_nrm; S.off_idx = L.off_idx; S.off_edges = L.off_edges;
    S.off_after = prefix;
    S.blob_capacity = std::min(ctx->h_stage_cap, ctx->d_frame.cap);
    S.pinned = pinned;
    if (pinned && S.table_cap < (size_t)n_batches3d * 5u) {
        if (S.table) (void)hipHostFree(S.table);
        S.table = nullptr;
        S.table_cap = 0;
        HIPCHK(ctx, hipHostMalloc((void **)&S.table, ((size_t)n_batches3d * 5u + 64u) * sizeof(FrameStream::GatherEntry), hipHostMallocDefault));
        S.table_cap = (size_t)n_batches3d * 5u + 64u;
    }
    S.handed.store(0);
    S.failed.store(0);
    S.edgeless.store(-1);
    S.err.clear();
    ctx->has_frame = false;
    S.active = true;
    if (getenv("RXR_E2E_TIMING")) fprintf(stderr, "rxr_e2e_timing stream_begin (%s)\n", pinned ? "pinned" : "copy");
    return RXR_OK;
}
int rxr_stream_begin(rxr_ctx *ctx, uint32_t n_batches3d, const uint32_t *vertex_capacity, const uint32_t *triangle_capacity) {
    return stream_begin(ctx, n_batches3d, vertex_capacity, triangle_capacity, false);
}
int rxr_stream_begin_pinned(rxr_ctx *ctx, uint32_t n_batches3d, const uint32_t *vertex_capacity, const uint32_t *triangle_capacity) {
    return stream_begin(ctx, n_batches3d, vertex_capacity, triangle_capacity, true);
}

// copy mode: claims retired batches one by one, copies their arrays to their dense places in the pinned staging blob and ships a
// group's five ranges when its last batch has landed.  Any thread; `limit` bounds the batches taken by this call.
static bool rxr_stream_copy_some(rxr_ctx *ctx, uint32_t limit) {
    FrameStream &S = ctx->fstream;
    uint8_t *const st = (uint8_t *)ctx->h_stage;
    for (uint32_t taken = 0; taken < limit; ++taken) {
        uint32_t j = S.copy_next.load(std::memory_order_relaxed);
        for (;;) {
            if (j >= S.retired.load(std::memory_order_acquire)) return true;
            if (S.copy_next.compare_exchange_weak(j, j + 1u, std::memory_order_relaxed)) break;
        }
        const FrameStream::Rec &Q = S.rec[j];
        if (Q.nv) {
            memcpy(st + S.off_pv + Q.v0 * 16, Q.pv, (size_t)Q.nv * 16);
            memcpy(st + S.off_uv + Q.v0 * 8, Q.uv, (size_t)Q.nv * 8);
            if (Q.nrm) memcpy(st + S.off_nrm + Q.v0 * 12, Q.nrm, (size_t)Q.nv * 12);
        }
        if (Q.nt) {
            memcpy(st + S.off_idx + Q.t0 * 12, Q.idx, (size_t)Q.nt * 12);
            memcpy(st + S.off_edges + Q.t0 * S.tri5(), Q.edges, (size_t)Q.nt * S.tri5());
        }
        const uint32_t g = j / S.group_size;
        if (S.group_left[g].fetch_sub(1u, std::memory_order_acq_rel) == 1u) {
            // the group's last batch has landed in pinned memory: its five ranges go to the device
            const FrameStream::Rec &A = S.rec[g * S.group_size], &Z = S.rec[std::min(S.n, (g + 1u) * S.group_size) - 1u];
            const size_t v0 = A.v0, nv = Z.v0 + Z.nv - A.v0, t0 = A.t0, nt = Z.t0 + Z.nt - A.t0;
            const struct { size_t off, bytes; } r[5] = {{S.off_pv + v0 * 16, nv * 16}, {S.off_uv + v0 * 8, nv * 8}, {S.off_nrm + v0 * 12, nv * 12},
                                                        {S.off_idx + t0 * 12, nt * 12}, {S.off_edges + t0 * S.tri5(), nt * S.tri5()}};
            std::lock_guard<std::mutex> lk(S.ship_mu);
            hipError_t e = hipSetDevice(ctx->device);
            for (const auto &x : r)
                if (x.bytes && e == hipSuccess) e = hipMemcpyAsync((uint8_t *)ctx->d_frame.p + x.off, st + x.off, x.bytes, hipMemcpyHostToDevice, ctx->stream);
            if (e != hipSuccess) {
                std::lock_guard<std::mutex> lk2(S.mu);
                if (S.err.empty()) S.err = "rxr_stream_batch3d: host->device copy failed";
                S.failed.store(1);
                return false;
            }
        }
    }
    return true;
}

// thread-safe; never touches ctx->err (the failure is kept in the stream and reported by rxr_upload_frame's fall-back)
int rxr_stream_batch3d(rxr_ctx *ctx, uint32_t index, const rxr_batch3d *b) {
    if (!ctx || !b || ctx->group) return RXR_ERR_INVALID;
    FrameStream &S = ctx->fstream;
    if (!S.active || index >= S.n) return RXR_ERR_INVALID;
    static const bool timing = getenv("RXR_E2E_TIMING") != nullptr;
    struct Tick {
        std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
        bool on;
        uint32_t index;
        ~Tick() {
            if (!on) return;
            const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
            static std::atomic<uint64_t> total{0}, worst{0}, calls{0};
            total += (uint64_t)us;
            uint64_t w = worst.load();
            while ((uint64_t)us > w && !worst.compare_exchange_weak(w, (uint64_t)us)) {}
            if (++calls % 289 == 0) fprintf(stderr, "rxr_e2e_timing stream_batch3d: %llu calls, %.1f us each on average, worst %llu us\n", (unsigned long long)calls.load(), (double)total.load() / (double)calls.load(), (unsigned long long)worst.load());
        }
    } tick;
    tick.on = timing;
    tick.index = index;
    auto give_up = [&](const char *why) {
        std::lock_guard<std::mutex> lk(S.mu);
        if (S.err.empty()) S.err = why;
        S.failed.store(1);
        return RXR_ERR_INVALID;
    };
    if (S.failed.load()) return RXR_ERR_INVALID;
    if (S.done[index].load(std::memory_order_acquire)) return give_up("rxr_stream_batch3d: batch handed over twice");
    if (b->n_vertices > S.cap_v[index] || b->n_triangles > S.cap_t[index]) return give_up("rxr_stream_batch3d: batch exceeds the capacity announced to rxr_stream_begin");
    if ((b->n_triangles && (!b->clipped_indices || (!b->edges && !b->edge_visible))) || (b->n_vertices && (!b->projected_vertices || !b->clipped_uvs)))
        return give_up("rxr_stream_batch3d: NULL arrays");
    if (b->n_triangles) {  // with Edges records or without (ABI 5): one form per frame, fixed by the first batch that has triangles
        const int form = b->edges ? 0 : 1;
        int seen = -1;
        if (!S.edgeless.compare_exchange_strong(seen, form) && seen != form) return give_up("rxr_stream_batch3d: batches with and without Edges records in one frame");
        if (form == 1 && b->cull_mode > RXR_CULL_BACK) return give_up("rxr_stream_batch3d: bad cull mode");
    }
    const void *const fifth = b->edges ? (const void *)b->edges : (const void *)b->edge_visible;
    const size_t fifth_bytes = (size_t)b->n_triangles * (b->edges ? sizeof(rxr_edges) : sizeof(uint32_t));
    {
        uint32_t worst = 0;  // every index (the kernels trust them)
        for (size_t t = 0; t < (size_t)b->n_triangles * 3u; ++t) worst = std::max(worst, b->clipped_indices[t]);
        if (b->n_triangles && worst >= b->n_vertices) return give_up("batch3d: vertex index out of range");
    }
    const void *dev_ptr[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    if (S.pinned) {
        // the promise is VERIFIED, array by array, first and last byte: a pointer the device cannot read would be a GPU page fault
        // (which can take the whole node down), so it costs the caller a frame handed over the plain way instead.  The kernel reads
        // through the DEVICE address the runtime reports for the array (round-3 advisor finding: for memory locked with hipHostRegister
        // / rxr_pin_host_buffer the device's address of a page need not be the host's; hipHostMalloc / rxr_alloc_pinned memory has one
        // address for both), and only when first and last byte lie `bytes - 1` apart there too: one registration, mapped in one piece.
        const struct { const void *p; size_t bytes; } arr[5] = {{b->projected_vertices, (size_t)b->n_vertices * 16}, {b->clipped_uvs, (size_t)b->n_vertices * 8},
                                                                {b->clipped_normals, b->clipped_normals ? (size_t)b->n_vertices * 12 : 0},
                                                                {b->clipped_indices, (size_t)b->n_triangles * 12}, {fifth, fifth_bytes}};
        for (int i = 0; i < 5; ++i) {
            const auto &x = arr[i];
            if (!x.bytes) continue;
            hipPointerAttribute_t a0{}, a1{};
            const hipError_t e0 = hipPointerGetAttributes(&a0, x.p), e1 = hipPointerGetAttributes(&a1, (const uint8_t *)x.p + x.bytes - 1);
            if (e0 != hipSuccess || e1 != hipSuccess || a0.type != hipMemoryTypeHost || a1.type != hipMemoryTypeHost) {
                (void)hipGetLastError();
                return give_up("rxr_stream_batch3d: an array is not in page-locked, device-readable memory (the promise of rxr_stream_begin_pinned)");
            }
            if (!a0.devicePointer || !a1.devicePointer || (const uint8_t *)a1.devicePointer - (const uint8_t *)a0.devicePointer != (ptrdiff_t)(x.bytes - 1))
                return give_up("rxr_stream_batch3d: an array is page-locked but has no device address in one piece (registered in parts, or not mapped)");
            dev_ptr[i] = a0.devicePointer;
        }
    }
    FrameStream::Rec &R = S.rec[index];
    R.pv = b->projected_vertices; R.uv = b->clipped_uvs; R.nrm = b->clipped_normals; R.idx = b->clipped_indices; R.edges = fifth;
    R.nv = b->n_vertices; R.nt = b->n_triangles;
    for (int i = 0; i < 5; ++i) R.dev[i] = dev_ptr[i];
    S.done[index].store(1, std::memory_order_release);
    S.handed.fetch_add(1);
    // retire in index order: a batch's place in the pools is the sum of its predecessors' sizes
    uint32_t first, last;
    {
        std::lock_guard<std::mutex> lk(S.mu);
        first = S.next;
        while (S.next < S.n && S.done[S.next].load(std::memory_order_acquire)) {
            FrameStream::Rec &Q = S.rec[S.next];
            Q.v0 = S.vcur;
            Q.t0 = S.tcur;
            S.vcur += Q.nv;
            S.tcur += Q.nt;
            ++S.next;
        }
        last = S.next;
        S.retired.store(S.next, std::memory_order_release);
    }
    if (!S.pinned) {
        // copy mode: a retired batch is copied by whichever caller gets to it (the thread that retires a long run must not be the
        // one that copies all of it: the others would project on while it falls behind)
        return rxr_stream_copy_some(ctx, 0xFFFFFFFFu) ? RXR_OK : RXR_ERR_INVALID;
    }
    for (uint32_t j = first; j < last; ++j) {
        // no host copy: when the group's last batch has retired, one kernel pulls the group out of the caller's arrays
        const uint32_t g = j / S.group_size;
        if (S.group_left[g].fetch_sub(1u, std::memory_order_acq_rel) != 1u) continue;
        const uint32_t b0 = g * S.group_size, b1 = std::min(S.n, (g + 1u) * S.group_size);
        FrameStream::GatherEntry *T = S.table + (size_t)b0 * 5u;
        uint32_t n_e = 0, piece = 0;
        for (uint32_t k = b0; k < b1; ++k) {
            const FrameStream::Rec &B = S.rec[k];
            // (sources: the arrays' DEVICE addresses, verified when the batch was handed over)
            const struct { const void *src; size_t off, bytes; } r[5] = {{B.dev[0], S.off_pv + B.v0 * 16, (size_t)B.nv * 16}, {B.dev[1], S.off_uv + B.v0 * 8, (size_t)B.nv * 8},
                                                                         {B.dev[2], S.off_nrm + B.v0 * 12, B.nrm ? (size_t)B.nv * 12 : 0}, {B.dev[3], S.off_idx + B.t0 * 12, (size_t)B.nt * 12},
                                                                         {B.dev[4], S.off_edges + B.t0 * S.tri5(), (size_t)B.nt * S.tri5()}};
            for (const auto &x : r) {
                if (!x.bytes) continue;
                T[n_e++] = FrameStream::GatherEntry{x.src, (uint64_t)x.off, (uint32_t)x.bytes, piece};
                piece += (uint32_t)((x.bytes + RXR_GATHER_PIECE - 1u) / RXR_GATHER_PIECE);
            }
        }
        if (n_e) {
            std::lock_guard<std::mutex> lk(S.ship_mu);
            hipError_t e = hipSetDevice(ctx->device);
            if (e == hipSuccess) {
                hipLaunchKernelGGL(k_gather_host, dim3(piece), dim3(256), 0, ctx->stream, (const FrameStream::GatherEntry *)T, n_e, (uint8_t *)ctx->d_frame.p);
                e = hipGetLastError();
            }
            if (e != hipSuccess) return give_up("rxr_stream_batch3d: the gather launch failed");
        }
    }
    return RXR_OK;
}

}  // extern "C"

namespace {

// "ensure, and zero it if it moved": a buffer whose invariant is all-zero between launches
int ensure_zeroed(rxr_ctx *ctx, DevBuf &b, size_t bytes) {
    void *before = b.p;
    if (int rc = rxr_ensure(ctx, b, bytes); rc != RXR_OK) return rc;
    if (b.p != before) HIPCHK(ctx, hipMemsetAsync(b.p, 0, b.cap, ctx->stream));
    return RXR_OK;
}

// the four arrays of a bin-pointer set (3D: d_bins, 2D: d_bins2d) carved out of one buffer
void carve_bins(void *buf, size_t n_bins, size_t n_chunks, uint32_t *&offset, uint32_t *&cursor, uint32_t *&chunk_tot, uint32_t *&chunk_base) {
    offset = (uint32_t *)buf;
    cursor = offset + n_bins + 1;
    chunk_tot = cursor + n_bins + 1;
    chunk_base = chunk_tot + n_chunks;
}

// one group of consecutive batches of the pipelined array copy (FrameBuild::copy_arrays)
struct ShipGroup { size_t v0, v1, t0, t1; std::atomic<uint32_t> left{0}; };

struct LocalTex { const rxr_texture *t; bool opaque; };  // one chunk texture of this frame

// the frustum reject of one mesh: all eight corners of its box outside one plane (batch3d.rs:493-552)
bool frustum_rejects(const rvek::Mat4 &mvp, const HostMesh &h) {
    bool out_l = true, out_r = true, out_b = true, out_t = true, out_n = true, out_f = true;
    for (int c = 0; c < 8; ++c) {
        rvek::Vec4 corner{(c & 4) ? h.aabb_hi[0] : h.aabb_lo[0], (c & 2) ? h.aabb_hi[1] : h.aabb_lo[1],
                          (c & 1) ? h.aabb_hi[2] : h.aabb_lo[2], 1.0f};
        rvek::Vec4 v = mvp * corner;
        const float w = v.w;
        out_l &= v.x < -w;
        out_r &= v.x > w;
        out_b &= v.y < -w;
        out_t &= v.y > w;
        out_n &= v.z < -w;
        out_f &= v.z > w;
    }
    return out_l || out_r || out_b || out_t || out_n || out_f;
}

// `x as usize` after the clamp against the screen, as the device's sat_index (rasterizer.rs:631-634)
uint32_t sat_px(float x, uint32_t hi) {
    if (!(x > 0.0f)) return 0u;
    if (x >= (float)hi) return hi;
    return (uint32_t)x;
}

// the Prim2D record of triangle t of 2D batch i
Prim2D prim2d_triangle(const rxr_batch2d &b, uint32_t i, uint32_t t, float W, float H) {
    const uint32_t *ix = b.indices + 3 * (size_t)t;
    rxr_edges built;
    if (!b.edges) {
        // ABI 5: Batch2D::project's Edges::new([v0,v1,v2], [v1,v2,v0], true) (src/batch/batch2d.rs:413-424, src/edge.rs:12-24)
        // from the projected vertices, here on the host (this file is built -ffp-contract=off: the same floats)
        const float *v[3] = {b.projected_vertices + 2 * (size_t)ix[0], b.projected_vertices + 2 * (size_t)ix[1], b.projected_vertices + 2 * (size_t)ix[2]};
        for (int k = 0; k < 3; ++k) {
            const float *p = v[k], *q = v[(k + 1) % 3];
            built.a[k] = q[1] - p[1];
            built.b[k] = p[0] - q[0];
            built.c[k] = q[0] * p[1] - q[1] * p[0];
        }
        built.visible = 1u;
    }
    const rxr_edges &e = b.edges ? b.edges[t] : built;
    Prim2D T{};
    memcpy(T.ea, e.a, 12);
    memcpy(T.eb, e.b, 12);
    memcpy(T.ec, e.c, 12);
    T.v0x = b.projected_vertices[2 * ix[0]]; T.v0y = b.projected_vertices[2 * ix[0] + 1];
    T.v1x = b.projected_vertices[2 * ix[1]]; T.v1y = b.projected_vertices[2 * ix[1] + 1];
    T.v2x = b.projected_vertices[2 * ix[2]]; T.v2y = b.projected_vertices[2 * ix[2] + 1];
    T.u0 = b.uvs[2 * ix[0]]; T.v0 = b.uvs[2 * ix[0] + 1];
    T.u1 = b.uvs[2 * ix[1]]; T.v1 = b.uvs[2 * ix[1] + 1];
    T.u2 = b.uvs[2 * ix[2]]; T.v2 = b.uvs[2 * ix[2] + 1];
    T.batch_kind = (i << 2) | (e.visible ? 1u : 0u);
    // clamped pixel box of the triangle, rasterizer.rs:615-634 with tile = whole screen
    float min_xf = std::fmin(T.v0x, std::fmin(T.v1x, T.v2x)), max_xf = std::fmax(T.v0x, std::fmax(T.v1x, T.v2x));
    float min_yf = std::fmin(T.v0y, std::fmin(T.v1y, T.v2y)), max_yf = std::fmax(T.v0y, std::fmax(T.v1y, T.v2y));
    uint32_t min_x = sat_px(std::fmax(std::floor(min_xf), 0.0f), 0xFFFFu), max_x = sat_px(std::fmin(std::ceil(max_xf), W), 0xFFFFu);
    uint32_t min_y = sat_px(std::fmax(std::floor(min_yf), 0.0f), 0xFFFFu), max_y = sat_px(std::fmin(std::ceil(max_yf), H), 0xFFFFu);
    if (!(min_x < max_x && min_y < max_y) || !e.visible) min_x = max_x = min_y = max_y = 0;
    T.bx = min_x | (max_x << 16);
    T.by = min_y | (max_y << 16);
    return T;
}

// the Prim2D record of the segment (ia, ib) of 2D line batch i; false: an end point is NaN or beyond +-2^30
bool prim2d_segment(const rxr_batch2d &b, uint32_t i, uint32_t ia, uint32_t ib, uint32_t color, const rxr_frame *f, Prim2D &Ln) {
    int32_t x0, y0, x1, y1;
    if (!to_isize32(b.projected_vertices[2 * ia], x0) || !to_isize32(b.projected_vertices[2 * ia + 1], y0) ||
        !to_isize32(b.projected_vertices[2 * ib], x1) || !to_isize32(b.projected_vertices[2 * ib + 1], y1))
        return false;
    Ln = Prim2D{};
    memcpy(&Ln.v0x, &x0, 4);
    memcpy(&Ln.v0y, &y0, 4);
    memcpy(&Ln.v1x, &x1, 4);
    memcpy(&Ln.v1y, &y1, 4);
    memcpy(&Ln.v2x, &color, 4);
    Ln.batch_kind = (i << 2) | 2u | 1u;
    // the walk never leaves the end-point box (the last point is not plotted, :1800)
    int64_t lx0 = std::min(x0, x1), lx1 = (int64_t)std::max(x0, x1) + 1, ly0 = std::min(y0, y1), ly1 = (int64_t)std::max(y0, y1) + 1;
    auto cl = [](int64_t v, int64_t hi) { return (uint32_t)std::min<int64_t>(std::max<int64_t>(v, 0), hi); };
    uint32_t min_x = cl(lx0, (int64_t)f->width), max_x = cl(lx1, (int64_t)f->width);
    uint32_t min_y = cl(ly0, (int64_t)f->height), max_y = cl(ly1, (int64_t)f->height);
    if (!(min_x < max_x && min_y < max_y)) min_x = max_x = min_y = max_y = 0;
    Ln.bx = min_x | (max_x << 16);
    Ln.by = min_y | (max_y << 16);
    return true;
}

// a batch whose box arithmetic the reference's per-tile test cannot be trusted with: its primitives only count inside the tiles
// that pass it (pad 0.5, :594-600)
void clip_prims_to_batch_tiles(const rxr_batch2d &b, const rxr_frame *f, Prim2D *first, Prim2D *last) {
    uint32_t clip_x0 = 0, clip_x1 = f->width, clip_y0 = 0, clip_y1 = f->height;
    rxr_ref_tile_span(b.bounding_box[0], b.bounding_box[2], f->width, f->tile_size, 0.5f, clip_x0, clip_x1);
    rxr_ref_tile_span(b.bounding_box[1], b.bounding_box[3], f->height, f->tile_size, 0.5f, clip_y0, clip_y1);
    for (Prim2D *q = first; q < last; ++q) {
        Prim2D &T = *q;
        uint32_t x0 = std::max(T.bx & 0xFFFFu, clip_x0), x1 = std::min(T.bx >> 16, clip_x1), y0 = std::max(T.by & 0xFFFFu, clip_y0), y1 = std::min(T.by >> 16, clip_y1);
        if (!(x0 < x1 && y0 < y1)) x0 = x1 = y0 = y1 = 0u;
        T.bx = x0 | (x1 << 16);
        T.by = y0 | (y1 << 16);
    }
}

// What rxr_upload_frame knows about the frame it hands over.  Its phases are the member functions below, in the order they run; each
// returns an rxr_status and leaves what the later ones need in here.
struct FrameBuild {
    rxr_ctx *const ctx;
    const rxr_frame *const f;
    FrameStream &S = ctx->fstream;
    const bool streamed;  // the 3D arrays were handed over while they were projected (rxr_stream_batch3d) and match this frame
    const bool use_meshes = (f->use_meshes & 1u) != 0;     // the 3D batches are the meshes of rxr_set_meshes
    const bool use_meshes2d = (f->use_meshes & 2u) != 0;   // the 2D batches are the meshes of rxr_set_meshes2d
    const uint32_t n_b3 = use_meshes ? (uint32_t)ctx->meshes.size() : f->n_batches3d, n_b2 = use_meshes2d ? (uint32_t)ctx->meshes2d.size() : f->n_batches2d;
    const uint32_t n_res_tex = (uint32_t)ctx->h_tex.size();
    const bool resident_ctex = ctx->ctex.set;  // the chunk textures are the slots of rxr_set_chunk_textures (rxr_chunk_tex.hip), not the frame's
    const float W = (float)f->width, H = (float)f->height;
    const std::chrono::steady_clock::time_point ut0 = std::chrono::steady_clock::now();  // RXR_E2E_TIMING diagnostics (tools/e2e_probe.py)
    double ut_validated = 0, ut_quiesced = 0, ut_headers = 0, ut_arrays = 0;
    double ut_ms() const { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - ut0).count(); }
    // the frame-wide facts, folded in header by header
    bool uses_programs = false, uses_chunk_tex = false;
    bool vis_programs = false;  // an opaque-pass batch whose program may write `opacity`: the visibility loop has to run it (DB_FULL_ALPHA)
    bool any_3d_visible = false, any_3d_program = false;
    int edgeless3d = -1;  // ABI 5: -1 no triangles yet, 0 the batches carry Edges records, 1 they carry `edge_visible` words instead
    // emissive (rasterizer.rs:1323, :1394): see the check behind the 3D batches below
    bool emissive_writer_3d = false;        // a visible 3D batch (either pass) runs a program that contains SetEmissive
    bool opaque_without_emissive = false;   // a visible opaque-pass 3D batch whose fragments do NOT assign emissive themselves
    uint32_t reads_2d = 0;  // PF_* read-before-written by the programs of visible 2D batches
    int32_t first_opacity_chunk = -1;  // opacity batches in two or more chunks: surface_id needs the exact prefix order (KL_CHUNK)
    bool seen_profiled_opaque = false; // ... and so does an opacity batch submitted AFTER an opaque batch that carries a profile id:
                                       // that opaque batch must not see it (rasterizer.rs:314-357; found by tools/fuzz_sweep.py)
    uint32_t opacity_group = 0;  // (header3d)
    bool has_opacity = false;
    size_t n_v3 = 0, n_t3 = 0, n_t2 = 0, n_l2 = 0, n_occ_total = f->n_occluders;
    // this frame's chunk textures (terrain, baked shader textures): DevTexDesc indices after the resident ones
    std::vector<LocalTex> local_tex;
    std::vector<int32_t> chunk_terrain;
    std::vector<std::vector<int32_t>> chunk_baked;
    size_t local_texels = 0;
    // the pixel rows in which the reference can draw anything of this frame: per kept batch the rows of the reference's own tiles that pass
    // its batch box test (rxr_ref_tile_span: rasterizer.rs:978-983, :594-600) -- outside them a 3D frame is the miss colour
    uint32_t content_y0 = f->height, content_y1 = 0;
    // ... and per tile row of the frame the tile columns, from the same boxes (a frame of very many boxes gives up: span_budget)
    const uint32_t n_tile_rows = (f->height + RXR_TILE_H - 1u) / RXR_TILE_H, n_tile_cols = (f->width + RXR_TILE_W - 1u) / RXR_TILE_W;
    std::vector<uint32_t> span_lo = std::vector<uint32_t>(n_tile_rows, n_tile_cols), span_hi = std::vector<uint32_t>(n_tile_rows, 0u);
    long span_budget = 400000;  // row updates
    Layout L{};
    bool with_tri_info = false, any_risky3d = false, with_clip3d = false;  // (lay_out)
    // a small host-projected frame: the TriSetup / TriShade records are built here, for the band [0, height), and travel in the blob --
    // its renders on tile rows launch no k_setup3d (lay_out; build_setup_records; render_impl)
    bool host_setup = false;
    uint32_t d2_box[4] = {0xFFFFu, 0u, 0xFFFFu, 0u};  // union of the 2D primitives' pixel boxes (fold_d2_box)
    bool d2_folded = false;
    uint8_t *st = nullptr;  // ctx->h_stage, once it is large enough (reserve), and the sections the phases share (clip3d: null without with_clip3d)
    DevBatch *b3 = nullptr; uint32_t *base = nullptr; uint4 *clip3d = nullptr; Prim2D *p2 = nullptr;
    size_t p2cur = 0, t2cur = 0;
    std::vector<uint32_t> group_of;  // the pipelined array copy (copy_arrays)
    std::unique_ptr<ShipGroup[]> groups;
    size_t n_groups_ship = 0;
    bool arrays_shipped = false;  // the five pools are on their way: the final copy sends only what surrounds them
    uint32_t tiles_x = 0;  // device scratch (size_scratch)
    size_t n_bins = 0, n_blocks = 0, n_groups = 0, n_chunks = 0;
    bool binned2d = false;
    FrameBuild(rxr_ctx *c, const rxr_frame *fr, bool streamed_) : ctx(c), f(fr), streamed(streamed_) {}

    // batch.shader -> program: chunk.shaders.get(index) for chunk batches, scene.shaders.get(index) otherwise
    // (src/rasterizer.rs:763-766, :1285-1288, :1645-1648)
    uint32_t program_of(int32_t shader, int32_t chunk) const {
        if (shader < 0) return 0u;
        if (chunk >= 0) {
            const rxr_chunk &ck = f->chunks[chunk];
            return (uint32_t)shader < ck.n_programs ? ck.program_base + (uint32_t)shader + 1u : 0u;
        }
        return (uint32_t)shader < f->n_shader_programs ? (uint32_t)shader + 1u : 0u;
    }
    void add_span(uint32_t x0, uint32_t x1, uint32_t y0, uint32_t y1) {  // pixels [x0, x1) x [y0, y1)
        if (x0 >= x1 || y0 >= y1 || span_budget < 0) return;
        const uint32_t c0 = x0 / RXR_TILE_W, c1 = std::min((x1 + RXR_TILE_W - 1u) / RXR_TILE_W, n_tile_cols), r0 = y0 / RXR_TILE_H, r1 = std::min((y1 + RXR_TILE_H - 1u) / RXR_TILE_H, n_tile_rows);
        span_budget -= (long)(r1 - r0);
        for (uint32_t r = r0; r < r1 && span_budget >= 0; ++r) {
            span_lo[r] = std::min(span_lo[r], c0);
            span_hi[r] = std::max(span_hi[r], c1);
        }
    }
    int32_t add_local(const rxr_texture &t) {
        if (t.width == 0 || t.height == 0 || t.width > 32768 || t.height > 32768) return -2;
        bool opaque = true;
        const size_t n = (size_t)t.width * t.height;
        for (size_t k = 0; k < n && opaque; ++k) opaque = t.rgba[4 * k + 3] == 255;
        local_tex.push_back(LocalTex{&t, opaque});
        local_texels += n;
        return (int32_t)(n_res_tex + local_tex.size() - 1);
    }
    bool tex_opaque(int32_t tex) const { return (uint32_t)tex < n_res_tex ? ctx->h_tex[tex].all_opaque != 0 : local_tex[(uint32_t)tex - n_res_tex].opaque; }
    // What a host-projected batch (Rec = rxr_batch3d) and a device-projected mesh (HostMesh) share of a 3D header: the flags from profile id and
    // list, the opacity group, ambient, classify3d, DB_SKIP -- and, for a batch that is kept, its part in the frame-wide facts.  `keep` as for
    // classify3d; the caller has set the bases, the counts, DB_HAS_NORMALS and the mode.
    template <class Rec> int header3d(DevBatch &d, const Rec &r, const float *ambient, bool &keep, const char *what) {
        const bool opacity_list = r.list == RXR_LIST_CHUNK_OPACITY, has_profile = r.has_profile_id != 0;
        if (has_profile) d.flags |= DB_HAS_PROFILE;
        if (opacity_list) d.flags |= DB_OPACITY_LIST;
        d.profile_id = r.profile_id;
        d.repeat_mode = r.repeat_mode;
        d.chunk = r.chunk;
        // Opacity groups (rxr_kernels.hip front_insert): the surface_id staircase of a pixel keeps one entry per GROUP of opacity
        // batches -- a maximal run, in submission order, with no opaque batch that carries a profile id in between.  Only such
        // batches ever read surface_id (:1044-1048), and their triangles' indices lie outside every group's index range, so of a
        // group's prefix minima only the last can be what they see.  (Counting a batch that turns out to be skipped as a separator
        // only makes groups smaller, which is always safe.)
        if (opacity_list) {
            if (opacity_group >= 0xFFFFu) return rxr_fail(ctx, RXR_ERR_UNSUPPORTED, "more than 65534 groups of opacity batches");
            d.flags |= opacity_group << DB_GROUP_SHIFT;
        } else if (has_profile) {
            ++opacity_group;
        }
        memcpy(d.ambient, ambient, 12);
        if (int rc = classify3d(d, r.source, r.chunk, r.shader, r.list, keep, what); rc != RXR_OK) return rc;
        if (!keep) {
            d.flags |= DB_SKIP;
            return RXR_OK;
        }
        any_3d_visible = true;
        if (d.program_plus1) uses_programs = any_3d_program = true;
        if ((d.flags & (DB_TERRAIN | DB_FULL_ALPHA)) || d.baked_plus1) uses_chunk_tex = true;
        if (opacity_list) {
            if (first_opacity_chunk < 0) first_opacity_chunk = r.chunk;
            else if (first_opacity_chunk != r.chunk) uses_chunk_tex = true;
            if (seen_profiled_opaque) uses_chunk_tex = true;
        } else if (d.flags & DB_HAS_PROFILE) {
            seen_profiled_opaque = true;
        }
        return RXR_OK;
    }
    // The header of one 2D batch (Rec = rxr_batch2d, or a mesh of rxr_set_meshes2d whose box reject is the device's: keep == true): mode, program,
    // texel source.  A program counts for the frame even when the batch is skipped.
    template <class Rec> int header2d(DevBatch &d, const Rec &r, uint32_t n_tris, uint32_t n_verts, bool keep, const char *no_texture) {
        d = DevBatch{};
        d.n_tris = n_tris;
        d.n_verts = n_verts;
        d.mode = r.mode;
        d.repeat_mode = r.repeat_mode;
        d.chunk = r.chunk;
        d.flags = r.receives_light ? DB_RECEIVES_LIGHT : 0u;
        d.program_plus1 = program_of(r.shader, r.chunk);
        if (d.program_plus1 && ctx->programs[d.program_plus1 - 1].shade_entry == 0xFFFFFFFFu) d.program_plus1 = 0;
        if (d.program_plus1) {
            d.flags |= DB_HAS_PROGRAM;
            uses_programs = true;
            reads_2d |= ctx->program_field_reads[d.program_plus1 - 1];
        }
        if (!keep) {
            d.flags |= DB_SKIP;
        } else if (r.source.kind == RXR_SOURCE_TERRAIN && r.chunk >= 0 && chunk_terrain[r.chunk] >= 0) {  // :749-751
            d.tex = chunk_terrain[r.chunk];
            d.flags |= DB_TERRAIN;
            uses_chunk_tex = true;
        } else {
            const int rc = resolve_source(ctx, r.source, false, r.chunk, f->animation_frame, d.tex, d.pixel);
            if (rc != RXR_OK) return rxr_fail(ctx, rc, no_texture);
        }
        return RXR_OK;
    }
    void copy_batch(size_t i) {
        const rxr_batch3d &b = f->batches3d[i];
        const size_t v0 = b3[i].vert_base, t0 = b3[i].tri_base;
        if (b.n_vertices) {
            memcpy(st + L.off_pv + v0 * 16, b.projected_vertices, (size_t)b.n_vertices * 16);
            memcpy(st + L.off_uv + v0 * 8, b.clipped_uvs, (size_t)b.n_vertices * 8);
            if (b.clipped_normals) memcpy(st + L.off_nrm + v0 * 12, b.clipped_normals, (size_t)b.n_vertices * 12);
        }
        if (b.n_triangles) {
            memcpy(st + L.off_idx + t0 * 12, b.clipped_indices, (size_t)b.n_triangles * 12);
            if (edgeless3d == 1) memcpy(st + L.off_edges + t0 * sizeof(uint32_t), b.edge_visible, (size_t)b.n_triangles * sizeof(uint32_t));
            else memcpy(st + L.off_edges + t0 * sizeof(rxr_edges), b.edges, (size_t)b.n_triangles * sizeof(rxr_edges));
        }
        if (n_groups_ship) groups[group_of[i]].left.fetch_sub(1u, std::memory_order_release);
    }
    // the calling thread of the pipelined copy: ships the five array ranges of a group as soon as its last batch has landed
    hipError_t ship_groups() {
        hipError_t ship_err = hipSuccess;
        uint8_t *const dst = (uint8_t *)ctx->d_frame.p;
        for (size_t g = 0; g < n_groups_ship; ++g) {
            ShipGroup &G = groups[g];
            while (G.left.load(std::memory_order_acquire) != 0u) std::this_thread::yield();
            const size_t nv = G.v1 - G.v0, nt = G.t1 - G.t0, tri5 = edgeless3d == 1 ? sizeof(uint32_t) : sizeof(rxr_edges);
            const struct { size_t off, bytes; } r[5] = {{L.off_pv + G.v0 * 16, nv * 16}, {L.off_uv + G.v0 * 8, nv * 8}, {L.off_nrm + G.v0 * 12, nv * 12},
                                                        {L.off_idx + G.t0 * 12, nt * 12}, {L.off_edges + G.t0 * tri5, nt * tri5}};
            for (const auto &x : r)
                if (x.bytes && ship_err == hipSuccess) ship_err = hipMemcpyAsync(dst + x.off, st + x.off, x.bytes, hipMemcpyHostToDevice, ctx->stream);
        }
        return ship_err;
    }
    bool spans_fit() const { return span_budget >= 0 && n_tile_rows <= RXR_MAX_TILE_ROWS; }
    static bool row_spans_on() { return !(getenv("RXR_ROW_SPANS") && atoi(getenv("RXR_ROW_SPANS")) == 0); }
    // writes the page-locked table from the spans of add_span and ships it: always, or when the spans leave out enough of tile rows [r0, r1)
    int ship_row_spans(uint32_t r0, uint32_t r1, bool always, bool &shipped) {
        size_t inside = 0;
        for (uint32_t r = 0; r < n_tile_rows; ++r) {
            const bool any = span_lo[r] < span_hi[r];
            ctx->h_row_spans[r] = make_uint2(any ? span_lo[r] : 0u, any ? span_hi[r] : 0u);
            if (r >= r0 && r < r1 && any) inside += span_hi[r] - span_lo[r];
        }
        // the spans pay when they leave out a good part of the content rows' tiles (a table look-up in front of every tile otherwise buys nothing)
        shipped = always || (inside * 100u <= (size_t)(r1 - r0) * n_tile_cols * 85u && (size_t)(r1 - r0) * n_tile_cols - inside >= content_min_tiles());
        if (!shipped) return RXR_OK;
        if (int rc = rxr_ensure(ctx, ctx->d_row_spans, RXR_MAX_TILE_ROWS * sizeof(uint2)); rc != RXR_OK) return rc;
        HIPCHK(ctx, hipMemcpyAsync(ctx->d_row_spans.p, ctx->h_row_spans, n_tile_rows * sizeof(uint2), hipMemcpyHostToDevice, ctx->stream));
        return RXR_OK;
    }

    // ---- the phases, in the order rxr_upload_frame runs them ----
    // the frame-level checks, then the 3D batches (with the parallel index check), the 2D batches, the chunks and their local textures
    int validate_and_count() {
        if (f->n_shader_programs > ctx->programs.size())
            return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_upload_frame: n_shader_programs exceeds the programs set with rxr_set_shaders");
        if (f->use_meshes > 3u) return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_upload_frame: use_meshes has unknown bits");
        if (use_meshes && f->n_batches3d) return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_upload_frame: use_meshes with batches3d");
        if (use_meshes2d && f->n_batches2d) return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_upload_frame: use_meshes (2D) with batches2d");
        if (use_meshes2d)
            for (const rxr_ctx::HostMesh2D &h : ctx->meshes2d)
                if (h.chunk >= (int32_t)f->n_chunks) return rxr_fail(ctx, RXR_ERR_INVALID, "mesh2d: chunk index out of range");
        if (use_meshes)
            for (const HostMesh &h : ctx->meshes) {
                if (h.chunk >= (int32_t)f->n_chunks) return rxr_fail(ctx, RXR_ERR_INVALID, "mesh: chunk index out of range");
                if (h.list == RXR_LIST_CHUNK_OPACITY) has_opacity = true;
            }
        for (uint32_t i = 0; i < f->n_batches3d; ++i) {
            const rxr_batch3d &b = f->batches3d[i];
            if (b.n_triangles && (!b.clipped_indices || (!b.edges && !b.edge_visible))) return rxr_fail(ctx, RXR_ERR_INVALID, "batch3d: NULL indices/edges");
            if (b.n_triangles) {  // ABI 5: with Edges records or without, one form per frame
                const int form = b.edges ? 0 : 1;
                if (edgeless3d < 0) edgeless3d = form;
                else if (edgeless3d != form) return rxr_fail(ctx, RXR_ERR_INVALID, "batch3d: batches with and without Edges records in one frame");
                if (form == 1 && b.cull_mode > RXR_CULL_BACK) return rxr_fail(ctx, RXR_ERR_INVALID, "batch3d: bad cull mode");
            }
            if (b.n_vertices && (!b.projected_vertices || !b.clipped_uvs)) return rxr_fail(ctx, RXR_ERR_INVALID, "batch3d: NULL vertex arrays");
            if (b.chunk >= (int32_t)f->n_chunks) return rxr_fail(ctx, RXR_ERR_INVALID, "batch3d: chunk index out of range");
            if (b.list == RXR_LIST_CHUNK_OPACITY) has_opacity = true;
            n_v3 += b.n_vertices;
            n_t3 += b.n_triangles;
        }
        if (!streamed) {  // (a streamed batch was checked when it was handed over)
            // every index of every batch (the kernels trust them): one job per batch on the host worker pool (rxr_parallel.h)
            std::atomic<bool> bad{false};
            rxr_parallel::run(f->n_batches3d, n_t3, [this, &bad](size_t i) {
                const rxr_batch3d &b = f->batches3d[i];
                uint32_t worst = 0;
                for (size_t t = 0; t < (size_t)b.n_triangles * 3u; ++t) worst = std::max(worst, b.clipped_indices[t]);
                if (b.n_triangles && worst >= b.n_vertices) bad.store(true, std::memory_order_relaxed);
            });
            if (bad.load()) return rxr_fail(ctx, RXR_ERR_INVALID, "batch3d: vertex index out of range");
        }
        if (n_v3 >= (1ull << 31) || n_t3 >= (1ull << 31)) return rxr_fail(ctx, RXR_ERR_INVALID, "frame too large (>= 2^31 vertices or triangles)");
        for (uint32_t i = 0; i < f->n_batches2d; ++i) {
            const rxr_batch2d &b = f->batches2d[i];
            if (b.n_triangles && !b.indices) return rxr_fail(ctx, RXR_ERR_INVALID, "batch2d: NULL indices");  // (edges may be NULL since ABI 5: built below)
            if (b.n_vertices && (!b.projected_vertices || !b.uvs)) return rxr_fail(ctx, RXR_ERR_INVALID, "batch2d: NULL vertex arrays");
            if (b.chunk >= (int32_t)f->n_chunks) return rxr_fail(ctx, RXR_ERR_INVALID, "batch2d: chunk index out of range");
            if (b.mode > RXR_MODE_LINE_LOOP) return rxr_fail(ctx, RXR_ERR_INVALID, "batch2d: bad mode");
            if (b.mode == RXR_MODE_TRIANGLES || b.mode == RXR_MODE_LINES)
                for (size_t t = 0; t < (size_t)b.n_triangles * 3u; ++t) {
                    if (b.mode == RXR_MODE_LINES && (t % 3u) == 2u) continue;  // only .0/.1 are read, :902
                    if (b.indices[t] >= b.n_vertices) return rxr_fail(ctx, RXR_ERR_INVALID, "batch2d: vertex index out of range");
                }
            switch (b.mode) {
                case RXR_MODE_TRIANGLES: n_t2 += b.n_triangles; break;
                case RXR_MODE_LINES: n_l2 += b.n_triangles; break;
                case RXR_MODE_LINE_STRIP: n_l2 += b.n_vertices ? b.n_vertices - 1 : 0; break;
                default: n_l2 += b.n_vertices; break;
            }
        }
        if (use_meshes2d) {
            n_t2 = ctx->meshes2d_tris;
            n_l2 = ctx->meshes2d_prims - ctx->meshes2d_tris;
        }
        chunk_terrain.assign(f->n_chunks, -1);
        chunk_baked.resize(f->n_chunks);
        if (resident_ctex) {
            // the chunk textures are those of rxr_set_chunk_textures: one DevTexDesc per slot behind the resident ones, no texels in the frame
            const ChunkTextures &T = ctx->ctex;
            if (f->n_chunks != T.terrain.size())
                return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_upload_frame: " + std::to_string(f->n_chunks) + " chunks, but rxr_set_chunk_textures registered the textures of " +
                                                          std::to_string(T.terrain.size()) + " (register again, or remove the registration with n_chunks == 0)");
            for (const ChunkTextures::Slot &s : T.slots) local_tex.push_back(LocalTex{nullptr, s.opaque != 0});
        }
        for (uint32_t c = 0; c < f->n_chunks && resident_ctex; ++c) {
            const rxr_chunk &ck = f->chunks[c];
            const ChunkTextures &T = ctx->ctex;
            if (ck.terrain_texture || ck.n_shader_textures)
                return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_upload_frame: chunk " + std::to_string(c) + " carries its own terrain_texture / shader_textures while rxr_set_chunk_textures holds a registration (they must be NULL / 0)");
            if (ck.n_occluders && !ck.occluders) return rxr_fail(ctx, RXR_ERR_INVALID, "chunk: NULL occluders");
            n_occ_total += ck.n_occluders;
            if ((uint64_t)ck.program_base + ck.n_programs > ctx->programs.size())
                return rxr_fail(ctx, RXR_ERR_INVALID, "chunk: program range exceeds the programs set with rxr_set_shaders");
            if (T.terrain[c] >= 0) {
                if (ck.size == 0) return rxr_fail(ctx, RXR_ERR_INVALID, "chunk: size 0 with a terrain texture (the reference divides by it, chunk.rs:138)");
                chunk_terrain[c] = (int32_t)(n_res_tex + (uint32_t)T.terrain[c]);
            }
            for (uint32_t k = T.shader_first[c]; k < T.shader_first[c + 1]; ++k)
                chunk_baked[c].push_back(T.shader_slots[k] >= 0 ? (int32_t)(n_res_tex + (uint32_t)T.shader_slots[k]) : -1);
        }
        for (uint32_t c = 0; c < f->n_chunks && !resident_ctex; ++c) {
            const rxr_chunk &ck = f->chunks[c];
            if (ck.n_occluders && !ck.occluders) return rxr_fail(ctx, RXR_ERR_INVALID, "chunk: NULL occluders");
            n_occ_total += ck.n_occluders;
            if ((uint64_t)ck.program_base + ck.n_programs > ctx->programs.size())
                return rxr_fail(ctx, RXR_ERR_INVALID, "chunk: program range exceeds the programs set with rxr_set_shaders");
            if (ck.n_shader_textures && !ck.shader_textures) return rxr_fail(ctx, RXR_ERR_INVALID, "chunk: NULL shader_textures");
            if (ck.terrain_texture && ck.terrain_texture->rgba) {
                if (ck.size == 0) return rxr_fail(ctx, RXR_ERR_INVALID, "chunk: size 0 with a terrain texture (the reference divides by it, chunk.rs:138)");
                if ((chunk_terrain[c] = add_local(*ck.terrain_texture)) == -2) return rxr_fail(ctx, RXR_ERR_INVALID, "chunk: bad terrain texture size");
            }
            chunk_baked[c].assign(ck.n_shader_textures, -1);
            for (uint32_t k = 0; k < ck.n_shader_textures; ++k)
                if (ck.shader_textures[k].rgba && (chunk_baked[c][k] = add_local(ck.shader_textures[k])) == -2)
                    return rxr_fail(ctx, RXR_ERR_INVALID, "chunk: bad shader texture size");
        }
        if (local_texels >= (1ull << 31)) return rxr_fail(ctx, RXR_ERR_INVALID, "chunk textures too large");
        return RXR_OK;
    }

    void lay_out() {
        // (a streamed frame's pools were laid out for the capacities announced before projection: the arrays sit densely at their front)
        BlobCursor take = streamed ? layout_prefix(n_b3, S.total_cap_v, S.total_cap_t, L) : layout_prefix(n_b3, n_v3, n_t3, L);
        with_tri_info = !use_meshes && n_t3 > 0 && n_t3 <= RXR_TRI_INFO_MAX;
        L.off_tinfo = take(with_tri_info ? n_t3 * sizeof(uint2) : 0);
        // (not a streamed hand-over: its arrays may have left for the device out of the caller's page-locked memory, never read here)
        host_setup = ctx->host_setup_on && ctx->small_mode == 2u && !use_meshes && !streamed && n_t3 > 0 && n_t3 <= RXR_STAGE_TRIS;
        if (host_setup) {  // (no other frame's blob changes)
            L.off_host_setup = take(n_t3 * sizeof(TriSetup));
            L.off_host_shade = take(n_t3 * sizeof(TriShade));
        }
        // host-projected 3D batches: per batch the pixels the reference draws it in (rxr_ref_tile_span), to which make_setup clips the pixel
        // boxes of its triangles.  Needed for a batch whose bounding-box arithmetic the reference's per-tile test cannot be trusted with
        // (rxr_device.h), and for EVERY batch of a frame whose raster grid is narrowed to row spans (spans_active, decided below from the same
        // rectangles): a triangle counted into a bin outside its row's span leaves that bin non-zero -- no workgroup hands it back -- and an
        // ordinary box can end short of its triangles too (`x + width` rounds below the maximum; a caller's box that does not enclose them)
        if (!use_meshes)
            for (uint32_t i = 0; i < n_b3 && !any_risky3d; ++i) {
                const rxr_batch3d &b = f->batches3d[i];
                any_risky3d = b.has_bounding_box && b.n_triangles > 0 && rxr_box_is_risky(b.bounding_box[0], b.bounding_box[1], b.bounding_box[2], b.bounding_box[3]);
            }
        with_clip3d = any_risky3d || (!use_meshes && (f->flags & RXR_FLAG_D3_ACTIVE) && f->tile_size > 0);  // (a superset of spans_active)
        L.off_clip3d = take(with_clip3d ? n_b3 * sizeof(uint4) : 0);
        L.off_lights = take(f->n_lights * sizeof(rxr_light));
        L.off_lights_fast = take(f->n_lights * sizeof(LightFast));
        L.off_occ = take(n_occ_total * sizeof(rxr_occluder));
        L.off_ld = take(f->n_linedefs * sizeof(rxr_linedef));
        L.off_chunks = take(f->n_chunks * sizeof(ChunkRange));
        L.off_tdesc = take((n_res_tex + local_tex.size()) * sizeof(DevTexDesc));
        L.off_ltex = take(local_texels * 4);
        L.off_b2 = take(n_b2 * sizeof(DevBatch));
        L.off_p2 = take((n_t2 + n_l2) * sizeof(Prim2D));
        L.off_bg = take(f->background_kind == RXR_BG_HOST_PIXELS ? (size_t)f->width * f->height * 4 : 0);
        L.total = take.o;
    }

    int reserve() {
        int rc;
        ctx->last_blob_tail = L.total - L.off_tinfo;
        if ((rc = rxr_ensure_stage(ctx, L.total)) != RXR_OK) return rc;
        if ((rc = rxr_ensure(ctx, ctx->d_frame, L.total)) != RXR_OK) return rc;
        // the staging blob may still be in flight from the previous upload, and the previous frame's renders -- possibly on
        // the caller's stream -- still read the frame blob and the scratch buffers
        ut_validated = ut_ms();
        // (a streamed frame: rxr_stream_begin has waited for the previous frame; what runs now are this frame's own transfers)
        if (!streamed && (rc = rxr_quiesce(ctx)) != RXR_OK) return rc;
        ut_quiesced = ut_ms();
        st = (uint8_t *)ctx->h_stage;
        b3 = (DevBatch *)(st + L.off_b3);
        base = (uint32_t *)(st + L.off_base);
        clip3d = with_clip3d ? (uint4 *)(st + L.off_clip3d) : nullptr;
        return RXR_OK;
    }

    // texel source, program, baked texture and the flags that follow from them, for one 3D batch header
    // (src/rasterizer.rs:1101-1304).  `keep` comes in as the box test and goes out false when nothing of the
    // batch can ever be written.
    int classify3d(DevBatch &d, const rxr_source &source, int32_t chunk, int32_t shader, uint32_t list, bool &keep, const char *what) {
        const bool opacity_list = list == RXR_LIST_CHUNK_OPACITY;
        d.program_plus1 = program_of(shader, chunk);
        d.baked_plus1 = 0;
        // chunk.shader_textures.get(shader_index) comes first, and only in the opaque pass (:1226-1267)
        if (!opacity_list && shader >= 0 && chunk >= 0 && (size_t)shader < chunk_baked[chunk].size() && chunk_baked[chunk][shader] >= 0) {
            d.baked_plus1 = (uint32_t)chunk_baked[chunk][shader] + 1u;
            d.program_plus1 = 0;
        }
        bool prog_runs = d.program_plus1 && ctx->programs[d.program_plus1 - 1].shade_entry != 0xFFFFFFFFu;
        const bool prog_opacity = prog_runs && (ctx->programs[d.program_plus1 - 1].flags & PG_WRITES_OPACITY);
        if (keep && prog_runs && (ctx->programs[d.program_plus1 - 1].flags & PG_WRITES_EMISSIVE)) emissive_writer_3d = true;
        if (keep && !opacity_list && !(prog_runs && (ctx->programs[d.program_plus1 - 1].flags & PG_ASSIGNS_EMISSIVE))) opaque_without_emissive = true;
        if (!prog_runs) d.program_plus1 = 0;
        if (prog_runs) d.flags |= DB_HAS_PROGRAM;
        if (!keep) return RXR_OK;
        bool alpha_varies = false, alpha_never_255 = false;
        if (source.kind == RXR_SOURCE_TERRAIN && chunk >= 0) {  // chunk.sample_terrain_texture, :1189-1191
            if (chunk_terrain[chunk] >= 0) {
                d.tex = chunk_terrain[chunk];
                d.flags |= DB_TERRAIN;
                alpha_varies = !tex_opaque(d.tex);
            } else {
                d.tex = -1;
                d.pixel = 0;  // no terrain texture: [0,0,0,0], chunk.rs:150
                alpha_never_255 = true;
            }
        } else {
            int rc2 = resolve_source(ctx, source, true, chunk, f->animation_frame, d.tex, d.pixel);
            if (rc2 != RXR_OK) return rxr_fail(ctx, rc2, std::string(what) + ": texture tile index out of range or tile without textures (the reference panics)");
            if (d.tex >= 0) alpha_varies = !tex_opaque(d.tex);
            else alpha_never_255 = (d.pixel >> 24) != 255u;
        }
        if (d.baked_plus1) {  // the baked texel replaces colour AND alpha (:1253-1262)
            alpha_varies = !tex_opaque((int32_t)d.baked_plus1 - 1);
            alpha_never_255 = false;
        }
        if (opacity_list) return RXR_OK;  // the opacity pass writes unconditionally (:1678-1682)
        if (prog_opacity) {
            d.flags |= DB_FULL_ALPHA;
            vis_programs = true;
        } else if (alpha_never_255) {
            keep = false;  // encoded alpha != 255: never written (:1408)
        } else if (alpha_varies) {
            // a plain texture's alpha needs the uv only; terrain texels need the world position, baked textures replace the source
            d.flags |= ((d.flags & DB_TERRAIN) || d.baked_plus1) ? DB_FULL_ALPHA : DB_ALPHA_TEST;
        }
        return RXR_OK;
    }

    int headers3d_host() {
        size_t vcur = 0, tcur = 0;
        for (uint32_t i = 0; i < f->n_batches3d; ++i) {
            const rxr_batch3d &b = f->batches3d[i];
            DevBatch d{};
            d.vert_base = (uint32_t)vcur;
            d.tri_base = (uint32_t)tcur;
            d.n_tris = b.n_triangles;
            d.n_verts = b.n_vertices;
            d.flags = b.clipped_normals ? DB_HAS_NORMALS : 0u;
            d.mode = edgeless3d == 1 ? b.cull_mode : 0u;  // (3D batches without Edges records: the cull mode make_setup builds them under)
            // batch-level box reject, rasterizer.rs:978-983, evaluated against the whole screen
            bool keep = b.has_bounding_box && b.n_triangles > 0;
            if (keep) {
                const float *bb = b.bounding_box;
                keep = bb[0] < W && (bb[0] + bb[2]) > 0.0f && bb[1] < H && (bb[1] + bb[3]) > 0.0f;
            }
            if (int rc = header3d(d, b, b.ambient_color, keep, "batch3d"); rc != RXR_OK) return rc;
            if (clip3d) clip3d[i] = make_uint4(0u, f->width, 0u, f->height);  // (a skipped batch's triangles get no pixel box at all)
            if (keep) {
                uint32_t x0 = 0, x1 = 0, y0 = 0, y1 = 0;
                rxr_ref_tile_span(b.bounding_box[1], b.bounding_box[3], f->height, f->tile_size, 0.0f, y0, y1);
                rxr_ref_tile_span(b.bounding_box[0], b.bounding_box[2], f->width, f->tile_size, 0.0f, x0, x1);
                if (y0 < y1) {
                    content_y0 = std::min(content_y0, y0);
                    content_y1 = std::max(content_y1, y1);
                    add_span(x0, x1, y0, y1);
                }
                if (clip3d) clip3d[i] = make_uint4(x0, x1, y0, y1);  // (empty when the reference draws the batch nowhere)
            }
            b3[i] = d;
            base[i] = (uint32_t)tcur;
            vcur += b.n_vertices;
            tcur += b.n_triangles;
        }
        base[f->n_batches3d] = (uint32_t)tcur;
        if (with_tri_info) {  // (batch, vert_base) per triangle: k_setup3d of a small frame looks its batch up instead of searching for it
            uint2 *ti = (uint2 *)(st + L.off_tinfo);
            for (uint32_t i = 0; i < f->n_batches3d; ++i)
                for (uint32_t t = 0; t < f->batches3d[i].n_triangles; ++t) ti[b3[i].tri_base + t] = make_uint2(i, b3[i].vert_base);
        }
        return RXR_OK;
    }

    int copy_arrays() {
        // the arrays themselves: independent per batch (offsets are in the headers just written), through the host worker pool --
        // 124 MB for the 1 M-triangle grid, which one thread copies in about as long as the GPU takes for forty frames
        // Large frames (the 1 M-triangle grid: 124 MB): the copy into pinned memory and the host->device copy are pipelined.  The
        // batches are cut into groups of consecutive batches of ~8 MB; the workers copy batch after batch, and the calling thread ships
        // the five array ranges of a group (vertices, uvs, normals, indices, edges: contiguous per group in each pool) as soon as the
        // group's last batch has landed -- the PCIe transfer of group g runs under the copies of the groups behind it.  Measured
        // (profiles/r03/c5_e2e_breakdown.jsonl): the whole call 14.1 -> 10.6 ms together with the wider worker pool (the hand-over alone 2.6 ms
        // either way on 64 threads: what the pipeline hides is the transfer, 124 MB at 50 GB/s).  RXR_UPLOAD_PIPELINE=0 keeps one copy at the end.
        const size_t big_bytes = n_v3 * 36 + n_t3 * 52;
        static const bool pipeline_off = getenv("RXR_UPLOAD_PIPELINE") && getenv("RXR_UPLOAD_PIPELINE")[0] == '0';
        if (!streamed && !use_meshes && !pipeline_off && big_bytes >= (32u << 20) && f->n_batches3d >= 8) {
            size_t target = std::max<size_t>(8u << 20, big_bytes / 8);  // (few, large transfers: every hipMemcpyAsync costs the calling thread ~20 us)
            if (const char *gs = getenv("RXR_UPLOAD_GROUP_MB")) target = std::max<size_t>(1u << 20, (size_t)atol(gs) << 20);
            group_of.resize(f->n_batches3d);
            groups.reset(new ShipGroup[f->n_batches3d]);
            size_t acc = 0;
            for (uint32_t i = 0; i < f->n_batches3d; ++i) {
                if (i == 0 || acc >= target) {
                    ShipGroup &g = groups[n_groups_ship++];
                    g.v0 = g.v1 = b3[i].vert_base;
                    g.t0 = g.t1 = b3[i].tri_base;
                    acc = 0;
                }
                ShipGroup &g = groups[n_groups_ship - 1];
                g.v1 += f->batches3d[i].n_vertices;
                g.t1 += f->batches3d[i].n_triangles;
                g.left.store(g.left.load(std::memory_order_relaxed) + 1u, std::memory_order_relaxed);
                group_of[i] = (uint32_t)(n_groups_ship - 1);
                acc += (size_t)f->batches3d[i].n_vertices * 36 + (size_t)f->batches3d[i].n_triangles * 52;
            }
        }
        ctx->last_upload_streamed = streamed ? (S.pinned ? 2 : 1) : 0;
        if (streamed) {
            arrays_shipped = true;  // ... since rxr_stream_batch3d
            if (!S.pinned && S.copy_next.load() < S.n) {
                // batches retired by the last hand-over calls and not copied yet: through the pool, one claim per job
                std::atomic<bool> ok{true};
                rxr_parallel::run(S.n - S.copy_next.load(), n_v3 + n_t3, [this, &ok](size_t) {
                    if (!rxr_stream_copy_some(ctx, 1u)) ok.store(false);
                });
                if (!ok.load() || S.failed.load()) return rxr_fail(ctx, RXR_ERR_HIP, "rxr_upload_frame: " + (S.err.empty() ? std::string("a streamed batch could not be shipped") : S.err));
            }
        } else if (n_groups_ship) {
            hipError_t ship_err = hipSuccess;
            arrays_shipped = rxr_parallel::run_with(f->n_batches3d, n_v3 + n_t3, [this](size_t i) { copy_batch(i); }, [this, &ship_err]() { ship_err = ship_groups(); });
            if (!arrays_shipped) {  // (a pool of one thread: copy, then one transfer at the end as for small frames)
                n_groups_ship = 0;
                for (size_t i = 0; i < f->n_batches3d; ++i) copy_batch(i);
            }
            if (ship_err != hipSuccess) return rxr_fail(ctx, RXR_ERR_HIP, std::string("rxr_upload_frame: hipMemcpyAsync: ") + hipGetErrorString(ship_err));
        } else {
            rxr_parallel::run(f->n_batches3d, n_v3 + n_t3, [this](size_t i) { copy_batch(i); });
        }
        return RXR_OK;
    }

    int headers3d_meshes() {
        // headers of the device-projected batches + the per-frame half of DevMesh (view * model, frustum reject)
        rvek::Mat4 view{}, proj{};
        memcpy(view.m, f->view, 64);
        memcpy(proj.m, f->projection, 64);
        const rvek::Mat4 pv_m = proj * view;
        std::vector<DevMesh> dm(ctx->meshes.size());
        for (uint32_t i = 0; i < n_b3; ++i) {
            const HostMesh &h = ctx->meshes[i];
            rvek::Mat4 model{};
            memcpy(model.m, f->mesh_transforms ? f->mesh_transforms + 16 * (size_t)i : h.transform, 64);
            const rvek::Mat4 mvp = pv_m * model;             // batch3d.rs:490
            const rvek::Mat4 view_model = view * model;      // :555
            const bool rejected = h.has_vertices && frustum_rejects(mvp, h);  // :493-552
            dm[i] = h.dev;
            dm[i].rejected = rejected ? 1u : 0u;
            memcpy(dm[i].view_model, view_model.m, 64);

            DevBatch d{};
            d.vert_base = h.dev.vout_base;
            d.tri_base = h.dev.tout_base;
            d.n_tris = 3u * h.dev.n_tris;
            d.n_verts = h.dev.n_verts + 4u * h.dev.n_tris;
            d.flags = DB_HAS_NORMALS;  // meshes with triangles must carry normals (batch3d.rs:605)
            bool keep = !rejected && h.dev.n_tris > 0;       // the box reject itself happens on the device (dev_bbox)
            if (int rc = header3d(d, h, h.ambient, keep, "mesh"); rc != RXR_OK) return rc;
            b3[i] = d;
            base[i] = h.dev.tout_base;
        }
        base[n_b3] = (uint32_t)ctx->mesh_tris_out;
        n_t3 = ctx->mesh_tris_out;
        // the per-frame DevMesh array goes straight into the projection scratch (tiny: 96 B per mesh)
        if (n_b3) HIPCHK(ctx, hipMemcpyAsync((uint8_t *)ctx->d_proj_misc.p + ctx->pp_off_meshes, dm.data(), dm.size() * sizeof(DevMesh),
                                             hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));  // `dm` is a stack-lifetime source
        return RXR_OK;
    }

    void write_lights_chunks_textures() {
        if (f->n_lights) memcpy(st + L.off_lights, f->lights, f->n_lights * sizeof(rxr_light));
        for (uint32_t i = 0; i < f->n_lights; ++i) light_fast_record(f->lights[i], f->hash_anim, *reinterpret_cast<LightFast *>(st + L.off_lights_fast + i * sizeof(LightFast)));
        {
            rxr_occluder *oc = (rxr_occluder *)(st + L.off_occ);
            if (f->n_occluders) memcpy(oc, f->occluders, f->n_occluders * sizeof(rxr_occluder));
            ChunkRange *cr = (ChunkRange *)(st + L.off_chunks);
            size_t cur = f->n_occluders;
            for (uint32_t c = 0; c < f->n_chunks; ++c) {
                cr[c] = ChunkRange{};
                cr[c].occ_first = (uint32_t)cur;
                cr[c].occ_count = f->chunks[c].n_occluders;
                cr[c].terrain_tex = chunk_terrain[c];
                cr[c].origin_x = f->chunks[c].origin[0];
                cr[c].origin_y = f->chunks[c].origin[1];
                if (chunk_terrain[c] >= 0) {
                    const int64_t wdt = (int32_t)(resident_ctex ? ctx->ctex.slots[(uint32_t)chunk_terrain[c] - n_res_tex].w : f->chunks[c].terrain_texture->width);
                    cr[c].pixels_per_tile = (int32_t)(wdt / f->chunks[c].size);  // `texture.width as i32 / self.size`, chunk.rs:138
                }
                if (f->chunks[c].n_occluders) memcpy(oc + cur, f->chunks[c].occluders, f->chunks[c].n_occluders * sizeof(rxr_occluder));
                cur += f->chunks[c].n_occluders;
            }
        }
        if (f->n_linedefs) memcpy(st + L.off_ld, f->linedefs, f->n_linedefs * sizeof(rxr_linedef));
        // texture descriptor table of the frame: the resident textures, then this frame's chunk textures
        DevTexDesc *td = (DevTexDesc *)(st + L.off_tdesc);
        if (n_res_tex) memcpy(td, ctx->h_tex.data(), n_res_tex * sizeof(DevTexDesc));
        size_t texel = 0;
        for (size_t k = 0; k < local_tex.size() && resident_ctex; ++k) {  // (texels: the resident pool, RasterParams.frame_texels)
            const ChunkTextures::Slot &s = ctx->ctex.slots[k];
            td[n_res_tex + k] = DevTexDesc{};
            td[n_res_tex + k].offset = s.offset;
            td[n_res_tex + k].w = s.w;
            td[n_res_tex + k].h = s.h;
            td[n_res_tex + k].all_opaque = (s.opaque ? 1u : 0u) | 2u;
        }
        for (size_t k = 0; k < local_tex.size() && !resident_ctex; ++k) {
            const rxr_texture &t = *local_tex[k].t;
            DevTexDesc &e = td[n_res_tex + k];
            e.offset = (uint32_t)texel;
            e.w = t.width;
            e.h = t.height;
            e.all_opaque = (local_tex[k].opaque ? 1u : 0u) | 2u;
            memcpy(st + L.off_ltex + texel * 4, t.rgba, (size_t)t.width * t.height * 4);
            texel += (size_t)t.width * t.height;
        }
    }

    int headers2d() {
        int rc;
        DevBatch *b2 = (DevBatch *)(st + L.off_b2);
        p2 = (Prim2D *)(st + L.off_p2);
        if (use_meshes2d) {
            // device-projected 2D batches: the headers only -- the box reject, the Edges and the Prim2D records are the device's
            // (k_proj2d_*, rxr_project.hip); a batch that turns out to be off screen gets empty pixel boxes there
            for (uint32_t i = 0; i < n_b2; ++i) {
                const rxr_ctx::HostMesh2D &h = ctx->meshes2d[i];
                if ((rc = header2d(b2[i], h, h.n_tris, h.n_verts, true, "mesh2d: tile without textures (the reference panics when the batch is on screen)")) != RXR_OK) return rc;
            }
            p2cur = ctx->meshes2d_prims;
            t2cur = ctx->meshes2d_tris;
        }
        for (uint32_t i = 0; i < f->n_batches2d; ++i) {
            const rxr_batch2d &b = f->batches2d[i];
            // batch-level box reject with pad 0.5, rasterizer.rs:594-600, against the whole screen
            bool keep = b.has_bounding_box != 0;
            if (keep) {
                const float *bb = b.bounding_box;
                const float pad = 0.5f;
                keep = bb[0] < W + pad && (bb[0] + bb[2]) > 0.0f - pad && bb[1] < H + pad && (bb[1] + bb[3]) > 0.0f - pad;
            }
            if ((rc = header2d(b2[i], b, b.n_triangles, b.n_vertices, keep, "batch2d: tile without textures (the reference panics)")) != RXR_OK) return rc;
            if (!keep) continue;
            const size_t p2_first = p2cur;
            if (b.mode == RXR_MODE_TRIANGLES) {
                for (uint32_t t = 0; t < b.n_triangles; ++t) {
                    p2[p2cur++] = prim2d_triangle(b, i, t, W, H);
                    ++t2cur;
                }
            } else {
                const uint8_t white[4] = {255, 255, 255, 255};
                uint32_t color = pack_px(b.source.kind == RXR_SOURCE_PIXEL ? b.source.pixel : white);  // :911-915
                const bool by_index = b.mode == RXR_MODE_LINES;  // (else a strip or a loop over the vertices in order)
                const uint32_t n_seg = by_index ? b.n_triangles : (b.mode == RXR_MODE_LINE_STRIP ? (b.n_vertices ? b.n_vertices - 1u : 0u) : b.n_vertices);
                for (uint32_t k = 0; k < n_seg; ++k, ++p2cur) {
                    const uint32_t ia = by_index ? b.indices[3 * (size_t)k] : k, ib = by_index ? b.indices[3 * (size_t)k + 1] : (k + 1u) % b.n_vertices;
                    if (!prim2d_segment(b, i, ia, ib, color, f, p2[p2cur])) return rxr_fail(ctx, RXR_ERR_UNSUPPORTED, "batch2d: line end point NaN or beyond +-2^30");
                }
            }
            if (rxr_box_is_risky(b.bounding_box[0], b.bounding_box[1], b.bounding_box[2], b.bounding_box[3])) clip_prims_to_batch_tiles(b, f, p2 + p2_first, p2 + p2cur);
        }
        if (f->background_kind == RXR_BG_HOST_PIXELS) memcpy(st + L.off_bg, f->background_pixels, (size_t)f->width * f->height * 4);
        return RXR_OK;
    }

    int size_scratch() {
        int rc;
        const uint32_t tiles_y_all = (f->height + RXR_TILE_H - 1) / RXR_TILE_H;
        tiles_x = (f->width + RXR_TILE_W - 1) / RXR_TILE_W;
        n_bins = (size_t)tiles_x * tiles_y_all;
        n_blocks = (size_t)((tiles_x + 3u) / 4u) * ((tiles_y_all + 3u) / 4u);  // k_blockscan's blocks of 4 x 4 bins
        if ((rc = rxr_ensure(ctx, ctx->d_tri_setup, (n_t3 ? n_t3 : 1) * sizeof(TriSetup))) != RXR_OK) return rc;
        if ((rc = rxr_ensure(ctx, ctx->d_tri_shade, (n_t3 ? n_t3 : 1) * sizeof(TriShade))) != RXR_OK) return rc;
        n_groups = (n_t3 + RXR_BLOCKSCAN_GROUP - 1) / RXR_BLOCKSCAN_GROUP;  // (their bin-range unions live behind the boxes)
        if ((rc = rxr_ensure(ctx, ctx->d_tri_box, ((n_t3 ? n_t3 : 1) + n_groups + 1) * sizeof(uint2))) != RXR_OK) return rc;
        n_chunks = (n_bins + RXR_SCAN_CHUNK - 1) / RXR_SCAN_CHUNK + 1;
        // bin_count lives in its OWN buffer: the invariant "all-zero between launches" (k_raster hands every
        // bin back cleared) must hold for whatever frame size comes next, so nothing else may share it
        // (behind the bin counts: k_blockscan's group counts per block of 4 x 4 bins, zero between launches like them)
        if ((rc = ensure_zeroed(ctx, ctx->d_bin_count, (n_bins + 1 + n_blocks) * sizeof(uint32_t))) != RXR_OK) return rc;
        if ((rc = rxr_ensure(ctx, ctx->d_bins, (2 * (n_bins + 1) + 2 * n_chunks + 8) * sizeof(uint32_t))) != RXR_OK) return rc;
        // (the large list doubles as k_blockscan's per-block group lists: the two are never used by the same launch)
        if ((rc = rxr_ensure(ctx, ctx->d_large, std::max<size_t>(n_t3 ? n_t3 : 1, n_blocks * RXR_BLOCKSCAN_BLOCK_GROUPS + n_groups + 1) * sizeof(uint32_t))) != RXR_OK) return rc;
        // 2D binning scratch (used only when the frame has more than RXR_STAGE_TRIS 2D primitives)
        binned2d = p2cur > RXR_STAGE_TRIS;
        if (binned2d) {
            if ((rc = ensure_zeroed(ctx, ctx->d_bin2d_count, (n_bins + 1) * sizeof(uint32_t))) != RXR_OK) return rc;
            if ((rc = rxr_ensure(ctx, ctx->d_bins2d, (2 * (n_bins + 1) + 2 * n_chunks + 8) * sizeof(uint32_t))) != RXR_OK) return rc;
            if ((rc = rxr_ensure(ctx, ctx->d_large2d, p2cur * sizeof(uint32_t))) != RXR_OK) return rc;
            size_t want2d = ctx->list_floor ? ctx->list_floor : std::max<size_t>(1u << 18, p2cur * 8);
            // k_blockscan2d: every bin its own run of RXR_BLOCKSCAN_CAP slots, lists in submission order (no sort per tile)
            bool on = true;
            if (const char *bs = getenv("RXR_BLOCKSCAN2D")) on = bs[0] != '0';
            ctx->blockscan2d_off = !(on && !ctx->list_floor && p2cur * n_blocks <= RXR_BLOCKSCAN_MAX_WORK / 4u &&
                                     (size_t)n_bins * RXR_BLOCKSCAN_CAP <= (64u << 20)) ||
                                   ctx->blockscan2d_bad.has(p2cur, n_bins);
            if (!ctx->blockscan2d_off) want2d = std::max<size_t>(want2d, (size_t)n_bins * RXR_BLOCKSCAN_CAP);
            if (want2d > ctx->list2d_capacity) {
                if ((rc = rxr_ensure(ctx, ctx->d_list2d, want2d * sizeof(uint32_t))) != RXR_OK) return rc;
                ctx->list2d_capacity = (uint32_t)std::min<size_t>(ctx->d_list2d.cap / sizeof(uint32_t), 0xFFFFFFF0u);
            }
        }
        if ((rc = ensure_zeroed(ctx, ctx->d_counters, 4 * CNT_WORDS * sizeof(uint32_t))) != RXR_OK) return rc;  // 2 sets for 3D, 2 for 2D
        size_t want_list = ctx->list_floor ? ctx->list_floor : std::max<size_t>(1u << 20, n_t3 * 4);
        // mid-sized scenes: k_blockscan gives every bin its own run of slots (not with a list floor: that knob exists to make the
        // general pipeline's lists overflow in tests)
        ctx->blockscan_cap = RXR_BLOCKSCAN_CAP;  // (both knobs are read per upload: tests and A-B runs switch them on a live context)
        ctx->blockscan_enabled = true;
        if (const char *bs = getenv("RXR_BLOCKSCAN")) ctx->blockscan_enabled = bs[0] != '0';
        if (const char *bc = getenv("RXR_BLOCKSCAN_CAP")) {  // tests: few slots per bin make ordinary meshes overflow them
            const long v = atol(bc);
            if (v > 0 && v <= 4096) ctx->blockscan_cap = (uint32_t)v;
        }
        // (frames beyond 8K x 8K tiles: fewer slots per bin keep k_blockscan inside its list budget -- their bins are thinner too; a bin that
        // overflows sends the frame through the general pipeline as ever)
        if (!getenv("RXR_BLOCKSCAN_CAP"))
            while (ctx->blockscan_cap > 64u && (size_t)n_bins * ctx->blockscan_cap > (64u << 20)) ctx->blockscan_cap /= 2u;
        ctx->blockscan_off = !(ctx->blockscan_enabled && !ctx->list_floor && n_t3 > RXR_STAGE_TRIS &&
                               (n_groups > RXR_BLOCKSCAN_SCATTER_GROUPS || n_groups * n_blocks <= RXR_BLOCKSCAN_MAX_WORK) &&
                               (size_t)n_bins * ctx->blockscan_cap <= (64u << 20));
        if (!ctx->blockscan_off && ctx->blockscan_bad.has(n_t3, n_bins)) ctx->blockscan_off = true;
        if (!ctx->blockscan_off) want_list = std::max<size_t>(want_list, (size_t)n_bins * ctx->blockscan_cap);
        if (want_list > ctx->list_capacity) {
            if ((rc = rxr_ensure(ctx, ctx->d_list, want_list * sizeof(uint32_t))) != RXR_OK) return rc;
            ctx->list_capacity = (uint32_t)std::min<size_t>(ctx->d_list.cap / sizeof(uint32_t), 0xFFFFFFF0u);
        }
        if ((rc = rxr_ensure(ctx, ctx->d_fb, (size_t)f->width * f->height * 4)) != RXR_OK) return rc;
        return RXR_OK;
    }

    // The set-up records of a small host-projected frame, by the function that defines them (rxr_tri_records, rxr_device.h): what
    // k_setup3d would write for the band [0, height), from the same values -- the arrays, headers, descriptors, the triangle table and
    // the clip rectangles as the earlier phases have put them into the staging blob, indexed the way make_setup indexes them on the
    // device.  A triangle that can never produce a pixel (invisible edge record, skipped batch) keeps an all-zero record, as there.
    // Needs to know whether the frame takes row spans (content_rows_and_spans): every pixel box is then clipped to its batch's tiles.
    void build_setup_records() {
        TriSetup *ts = (TriSetup *)(st + L.off_host_setup);
        TriShade *th = (TriShade *)(st + L.off_host_shade);
        memset(ts, 0, n_t3 * sizeof(TriSetup));
        memset(th, 0, n_t3 * sizeof(TriShade));
        HostSetupSource src{};
        src.pv = (const float *)(st + L.off_pv);
        src.uv = (const float *)(st + L.off_uv);
        src.nrm = (const float *)(st + L.off_nrm);
        src.idx = (const uint32_t *)(st + L.off_idx);
        src.edges = st + L.off_edges;
        src.edgeless = edgeless3d == 1;
        src.tri_info = (const uint32_t *)(st + L.off_tinfo);
        src.batches = b3;
        src.tex = (const DevTexDesc *)(st + L.off_tdesc);
        src.clip = (any_risky3d || ctx->spans_active) ? (const uint32_t *)clip3d : nullptr;  // (RasterParams.batch_clip3d != NULL)
        src.sample_mode = f->sample_mode;
        src.width = f->width;
        src.height = f->height;
        // ... and, from the records just written, the tile rows that anything 3D can reach (rxr_tri_tile_rows: the kernel's own tile
        // reject, asked of whole tile rows): the union over all triangles, opacity-list batches included, as one range.  The pixel boxes
        // of triangles clipped at the near plane are clamped to the whole height and a 2D primitive anywhere pins the content rows; only
        // the edge functions know that the rows above a room's walls are empty.  k_raster[_rl] skip the 3D passes of a workgroup
        // outside the range (raster_tile).  Not with a brush preview (it paints missed pixels, :435-458), not for 2D-only frames
        // (nothing looks); RXR_D3_ROWS=0 (read per upload) switches it off for A-B runs and tests.  Nothing is kept across uploads.
        const bool d3_rows = !(getenv("RXR_D3_ROWS") && atoi(getenv("RXR_D3_ROWS")) == 0) && (f->flags & RXR_FLAG_D3_ACTIVE) && !f->has_brush_preview;
        uint32_t r0 = 0xFFFFFFFFu, r1 = 0u;
        for (size_t t = 0; t < n_t3; ++t) {
            rxr_host_tri_records(src, t, ts[t], th[t]);
            if (d3_rows) rxr_union_tile_rows(ts[t], f->width, RXR_TILE_H, r0, r1);
        }
        if (d3_rows) {
            ctx->d3_trow0 = r0 < r1 ? r0 : 0u;  // (no triangle reaches anything: the empty range)
            ctx->d3_trow1 = r0 < r1 ? r1 : 0u;
        }
    }

    int ship_blob() {
        if (arrays_shipped) {
            // the projected arrays [off_pv, off_tinfo) left while they were being copied; what surrounds them follows
            HIPCHK(ctx, hipMemcpyAsync(ctx->d_frame.p, st, L.off_pv, hipMemcpyHostToDevice, ctx->stream));
            HIPCHK(ctx, hipMemcpyAsync((uint8_t *)ctx->d_frame.p + L.off_tinfo, st + L.off_tinfo, L.total - L.off_tinfo, hipMemcpyHostToDevice, ctx->stream));
        } else {
            HIPCHK(ctx, hipMemcpyAsync(ctx->d_frame.p, st, L.total, hipMemcpyHostToDevice, ctx->stream));
        }
        return RXR_OK;
    }

    // tiles outside the union of the 2D pixel boxes skip the 2D pass without touching memory; the union also belongs to the content rows
    // and the row spans (once per upload: before content_rows_and_spans, wherever that runs)
    void fold_d2_box() {
        if (d2_folded) return;
        d2_folded = true;
        uint32_t bx0 = 0xFFFFu, bx1 = 0, by0 = 0xFFFFu, by1 = 0;
        for (size_t i = 0; i < (use_meshes2d ? 0 : p2cur); ++i) {  // (device-projected: the records do not exist yet -- RasterParams.d2_box_dev)
            uint32_t a = p2[i].bx & 0xFFFFu, b = p2[i].bx >> 16, c = p2[i].by & 0xFFFFu, d = p2[i].by >> 16;
            if (a < b && c < d) {
                bx0 = std::min(bx0, a); bx1 = std::max(bx1, b); by0 = std::min(by0, c); by1 = std::max(by1, d);
            }
        }
        d2_box[0] = bx0; d2_box[1] = bx1; d2_box[2] = by0; d2_box[3] = by1;
        if (by0 < by1) {  // (the 2D pass only ever writes inside its primitives' pixel boxes)
            content_y0 = std::min(content_y0, by0);
            content_y1 = std::max(content_y1, std::min(by1, f->height));
            add_span(bx0, std::min(bx1, f->width), by0, std::min(by1, f->height));
        }
    }

    int fill_raster_params() {
        RasterParams &P = ctx->P;
        memset(&P, 0, sizeof(P));
        P.width = f->width;
        P.height = f->height;
        P.tiles_x = tiles_x;
        P.flags = f->flags;
        P.fwidth = W;
        P.fheight = H;
        memcpy(P.inv_view, f->inverse_view, 64);
        memcpy(P.inv_proj, f->inverse_projection, 64);
        P.ndc_sx = (float)(2.0 / (double)W);  // (the frame size is validated: 1 .. 32768)
        P.ndc_sy = (float)(-2.0 / (double)H);
        memcpy(P.cam, f->camera_pos, 12);
        memcpy(P.translationd2, f->translationd2, 8);
        P.scaled2 = f->scaled2;
        P.hash_anim = f->hash_anim;
        P.sample_mode = f->sample_mode;
        P.background_color = pack_px(f->background_color);
        P.background_kind = f->background_kind;
        memcpy(P.bg_grid, f->background_grid, 16);
        P.has_brush = f->has_brush_preview ? 1u : 0u;
        memcpy(P.brush_pos, f->brush_position, 12);
        P.brush_radius = f->brush_radius;
        P.brush_falloff = f->brush_falloff;
        memcpy(P.ambient, f->ambient, 16);
        memcpy(P.sun_dir, f->sun_dir, 12);
        P.day_factor = f->day_factor;
        P.n_tris3d = (uint32_t)n_t3;
        P.d3_trow0 = ctx->d3_trow0;  // (build_setup_records, or all rows)
        P.d3_trow1 = ctx->d3_trow1;
        P.n_batches3d = n_b3;
        P.n_lights = f->n_lights;
        P.n_occluders = f->n_occluders;
        P.any_occluders = n_occ_total ? 1u : 0u;
        P.n_linedefs = f->n_linedefs;
        P.n_prims2d = (uint32_t)p2cur;
        P.binned2d = binned2d ? 1u : 0u;
        // the 2D pass runs after the 3D passes on the SAME Execution (rasterizer.rs:310, :501): `normal` and `opacity.x` are
        // assigned by every 3D fragment and never by the 2D loop, `hitpoint.z` by every 3D fragment that runs a program
        if (any_3d_visible && (f->flags & RXR_FLAG_D3_ACTIVE) && (reads_2d & (PF_NORMAL | PF_OPACITY)))
            return rxr_fail(ctx, RXR_ERR_UNSUPPORTED, "a 2D batch's program reads normal / opacity, which in the reference hold whatever the tile's last 3D fragment left there");
        if (any_3d_program && (f->flags & RXR_FLAG_D3_ACTIVE) && (reads_2d & PF_HITPOINT))
            return rxr_fail(ctx, RXR_ERR_UNSUPPORTED, "a 2D batch's program reads hitpoint while 3D batches run programs: hitpoint.z would hold the tile's last 3D program fragment's");
        // `emissive` is only ever written by SetEmissive and never reset by the raster loops: every opaque 3D fragment adds whatever
        // the last SetEmissive executed in its TILE left behind (rasterizer.rs:310, :1323, :1394) -- a function of the tile size and of
        // the traversal order, which a per-fragment evaluation cannot (and should not) reproduce.  A frame is accepted when that
        // state cannot be observed: no program of a 3D batch on screen writes emissive, or EVERY opaque 3D batch on screen runs a
        // program that assigns emissive itself on every path before the fragment reads it.
        if (emissive_writer_3d && opaque_without_emissive && (f->flags & RXR_FLAG_D3_ACTIVE))
            return rxr_fail(ctx, RXR_ERR_UNSUPPORTED,
                        "a 3D batch's program writes emissive while another opaque 3D batch of the frame does not assign it on every path: in the "
                        "reference that batch's fragments would add the emissive of whichever fragment ran before them in the tile");
        ctx->frame_uses_programs = uses_programs;
        P.vm_code = (const uint32_t *)ctx->d_vm_code.p;
        // (the brush preview and the grid background are editor-only: they live in the levels with the chunk paths so that k_raster does not
        // carry them -- merely compiling the grid shader into it cost the bench frame 9 % more VALU instructions in SGPR spills)
        const bool editor_paths = (P.has_brush && (f->flags & RXR_FLAG_D3_ACTIVE)) || f->background_kind == RXR_BG_GRID;
        P.kernel_level = std::max<uint32_t>(ctx->min_kernel_level, uses_programs ? KL_VM : ((uses_chunk_tex || editor_paths) ? KL_CHUNK : KL_COMMON));
        ctx->frame_needs_chunk_paths = uses_chunk_tex || editor_paths || ctx->min_kernel_level >= KL_CHUNK;  // (rxr_jit_launch: JIT_PLAIN otherwise)
        P.plain_programs = (!ctx->frame_needs_chunk_paths && !getenv("RXR_NO_PLAIN_PROGRAMS")) ? 1u : 0u;
        {
            // RXR_LIGHT_MATH (read per frame; rxr_set_light_math sets the context's own default): "exact" -- the light loop in the
            // reference's correctly rounded operations; "relaxed" -- point lights through rsq / rcp products, within the 1-per-channel
            // tolerance of lit 3D fragments (shade3d_lights<LV, true>; Level::Common and Level::Chunk)
            const char *lm = getenv("RXR_LIGHT_MATH");
            P.relaxed_lights = lm ? (lm[0] == 'r' ? 1u : 0u) : (ctx->relaxed_lights ? 1u : 0u);
            // the fused point-light term multiplies where the reference branches (a light out of range contributes intensity * 0): with an
            // infinite or NaN intensity, colour, position or range that is NaN where the reference adds nothing -- and so it is with FINITE
            // parameters whose product overflows (colour -3e38 x flicker 3e38 = inf, times the 0 of an out-of-range fragment: found by
            // tools/fuzz_special2.py, seed 1036).  Such frames -- no real scene has them -- take the exact loop, which skips and branches
            // like the reference (light.rs:535-552): every factor of the fused term must stay below 1e9 in magnitude (their product below 1e36).
            for (uint32_t i = 0; i < f->n_lights && P.relaxed_lights; ++i) {
                const rxr_light &l = f->lights[i];
                const float v[] = {l.intensity, l.color[0], l.color[1], l.color[2], l.position[0], l.position[1], l.position[2], l.start_distance, l.end_distance, l.flicker};
                for (float x : v)
                    if (!(std::fabs(x) <= 1.0e9f)) P.relaxed_lights = 0u;
            }
            // RXR_LIGHT_PREFIX=0 (read per upload: tests, A-B runs): the relaxed kernels send every light through their general loop
            const char *lp = getenv("RXR_LIGHT_PREFIX");
            P.flags = (P.flags & ~RPF_LIGHT_PREFIX) | ((lp && atoi(lp) == 0) ? 0u : RPF_LIGHT_PREFIX);
            P.rl_flip_guard = 1e-4f;
            if (const char *fg = getenv("RXR_RL_FLIP_GUARD")) {  // tests: a large guard sends every wave down the exact normal sequences
                const float v = (float)atof(fg);
                if (v >= 1e-4f) P.rl_flip_guard = v;
            }
        }
        if (P.kernel_level == KL_VM && uses_programs && ctx->programs_static) P.kernel_level = KL_VM_S;  // k_raster_vm_s: wave-uniform stack pointer
        // k_raster_vm_sv: ... and no program decides whether an opaque fragment is written, so the visibility loop is the one of
        // k_raster_chunk, without a call of the interpreter in it
        if (P.kernel_level == KL_VM_S && !vis_programs && !getenv("RXR_VM_VIS_CALLS")) P.kernel_level = KL_VM_SV;
        else if (P.kernel_level == KL_VM && uses_programs && !vis_programs && !getenv("RXR_VM_VIS_CALLS")) P.kernel_level = KL_VM_V;  // k_raster_vm_v
        P.programs = (const DevProgram *)ctx->d_programs.p;
        P.patterns = (const DevPattern *)ctx->d_patterns.p;
        P.pattern_data = (const float *)ctx->d_pattern_data.p;
        P.palette = (const float *)ctx->d_palette.p;
        P.n_programs = (uint32_t)ctx->programs.size();
        P.n_patterns = ctx->n_patterns;
        P.n_normal_patterns = ctx->n_normal_patterns;
        P.n_palette = ctx->n_palette;
        P.vm_fault = ctx->d_host_status + HS_VM_FAULT;
        P.staircase_overflow = ctx->d_host_status + HS_STAIRCASE;
        P.time = f->time;
        fold_d2_box();
        memcpy(P.d2_box, d2_box, sizeof(P.d2_box));
        P.d2_box_dev = use_meshes2d ? ctx->PP2.d2_box : nullptr;  // (the device builds these records: their boxes are not known here)
        P.list2d_capacity = ctx->list2d_capacity;
        P.any_lights = f->n_lights ? 1u : 0u;
        P.has_opacity = has_opacity ? 1u : 0u;
        {
            // frames in which row mode has to work around some candidates (rxr_kernels.hip SPLITR): a kept batch of the opaque pass whose
            // fragments need their texel's alpha, or -- under an opacity pass -- one that carries a profile id
            bool split = false;
            const DevBatch *hb = (const DevBatch *)(st + L.off_b3);
            for (uint32_t i = 0; i < n_b3 && !split; ++i) {
                if (hb[i].flags & (DB_SKIP | DB_OPACITY_LIST)) continue;
                split = (hb[i].flags & (DB_ALPHA_TEST | DB_FULL_ALPHA)) != 0 || (has_opacity && (hb[i].flags & DB_HAS_PROFILE));
            }
            P.split_rounds = ((split && !getenv("RXR_NO_SPLIT_ROUNDS")) || getenv("RXR_FORCE_SPLIT_ROUNDS")) ? 1u : 0u;   // (the variables: A-B runs, tests)
        }
        P.list_capacity = ctx->list_capacity;
        uint8_t *d = (uint8_t *)ctx->d_frame.p;
        P.pv = (const float4 *)(d + L.off_pv);
        P.uv = (const float2 *)(d + L.off_uv);
        P.nrm = (const float *)(d + L.off_nrm);
        P.idx = (const uint32_t *)(d + L.off_idx);
        P.edges = (const rxr_edges *)(d + L.off_edges);
        P.edge_vis3d = edgeless3d == 1 ? (const uint32_t *)(d + L.off_edges) : nullptr;  // (the same pool, a word per triangle instead of a record)
        P.batches3d = (const DevBatch *)(d + L.off_b3);
        P.batch_tri_base = (const uint32_t *)(d + L.off_base);
        P.tri_info = with_tri_info ? (const uint2 *)(d + L.off_tinfo) : nullptr;
        P.batch_clip3d = any_risky3d ? (const uint4 *)(d + L.off_clip3d) : nullptr;   // (and when the frame takes row spans: clip_to_spans)
        P.ref_tile = f->tile_size;
        P.tri_setup = (TriSetup *)ctx->d_tri_setup.p;
        P.tri_shade = (TriShade *)ctx->d_tri_shade.p;
        P.tri_box = (uint2 *)ctx->d_tri_box.p;
        P.group_rng = P.tri_box + (n_t3 ? n_t3 : 1);
        P.blk_cnt = (uint32_t *)ctx->d_bin_count.p + n_bins + 1;
        P.blk_grp = (uint32_t *)ctx->d_large.p;
        P.blockscan_scatter = n_groups > RXR_BLOCKSCAN_SCATTER_GROUPS ? 1u : 0u;
        P.blk_wide_base = (uint32_t)(n_blocks * RXR_BLOCKSCAN_BLOCK_GROUPS);
        P.bin_count = (uint32_t *)ctx->d_bin_count.p;
        carve_bins(ctx->d_bins.p, n_bins, n_chunks, P.bin_offset, P.bin_cursor, P.chunk_tot, P.chunk_base);
        P.host_status = ctx->d_host_status;
        P.bin_list = (uint32_t *)ctx->d_list.p;
        P.large_list = (uint32_t *)ctx->d_large.p;
        P.counters = (uint32_t *)ctx->d_counters.p;
        P.lights = (const rxr_light *)(d + L.off_lights);
        P.lights_fast = (const LightFast *)(d + L.off_lights_fast);
        P.occluders = (const rxr_occluder *)(d + L.off_occ);
        P.linedefs = (const rxr_linedef *)(d + L.off_ld);
        P.chunks = (const ChunkRange *)(d + L.off_chunks);
        P.batches2d = (const DevBatch *)(d + L.off_b2);
        P.prim2d = (const Prim2D *)(d + L.off_p2);
        if (binned2d) {
            P.bin2d_count = (uint32_t *)ctx->d_bin2d_count.p;
            carve_bins(ctx->d_bins2d.p, n_bins, n_chunks, P.bin2d_offset, P.bin2d_cursor, P.chunk2d_tot, P.chunk2d_base);
            P.bin2d_list = (uint32_t *)ctx->d_list2d.p;
            P.large2d_list = (uint32_t *)ctx->d_large2d.p;
            P.host_status2d = ctx->d_host_status + CNT_WORDS;
        }
        P.texels = (const uint32_t *)ctx->d_texels.p;
        P.tex = (const DevTexDesc *)(d + L.off_tdesc);
        P.frame_texels = resident_ctex ? (const uint32_t *)ctx->ctex.pool.p : (const uint32_t *)(d + L.off_ltex);
        P.bg_pixels = (const uint32_t *)(d + L.off_bg);
        ctx->frame_uses_meshes2d = use_meshes2d;
        if (use_meshes2d) {
            Project2DParams &PP2 = ctx->PP2;
            PP2.has_matrix = ctx->has_matrix2d ? 1u : 0u;
            memcpy(PP2.m, ctx->matrix2d, sizeof(PP2.m));
            PP2.width = W;
            PP2.height = H;
            PP2.ref_tile = f->tile_size;
            PP2.out = (Prim2D *)(d + L.off_p2);
        }
        ctx->frame_uses_meshes = use_meshes;
        if (use_meshes) {
            // the raster pre-pass reads the pools the projection kernels write
            ProjectParams &PP = ctx->PP;
            memcpy(PP.projection, f->projection, 64);
            PP.width = W;
            PP.height = H;
            PP.meshes = (const DevMesh *)((uint8_t *)ctx->d_proj_misc.p + ctx->pp_off_meshes);
            P.pv = PP.pv;
            P.uv = PP.uv;
            P.nrm = PP.nrm;
            P.idx = PP.idx;
            P.edges = PP.edges;
            P.edge_vis3d = nullptr;
            P.dev_bbox = PP.bbox;
            P.mesh_live = PP.mesh_live;
            // the set-up builds the Edges records itself (k_proj_edges fused into make_setup): RXR_PROJ_FUSED_EDGES=0 keeps the pool
            static const bool fused_edges = !(getenv("RXR_PROJ_FUSED_EDGES") && atoi(getenv("RXR_PROJ_FUSED_EDGES")) == 0);
            PP.edges_in_setup = fused_edges ? 1u : 0u;
            P.pm_meshes = fused_edges ? PP.meshes : nullptr;
            P.pm_edge_vis = fused_edges ? PP.edge_vis : nullptr;
        }
        return RXR_OK;
    }

    int content_rows_and_spans() {
        int rc;
        const bool has_brush = f->has_brush_preview != 0;  // (RasterParams.has_brush)
        fold_d2_box();
        // Known content rows: host-projected batches only (the device-projected ones have their boxes on the device), 3D mode (the miss
        // colour is then the constant [0,0,0,255], :420-461; in 2D mode the background is evaluated per pixel), no brush preview (it paints
        // missed pixels, :435-458).  RXR_CONTENT_ROWS=0 switches the clamp off (A-B runs, tests).
        const bool content_clamp = !(getenv("RXR_CONTENT_ROWS") && atoi(getenv("RXR_CONTENT_ROWS")) == 0);  // (read per upload: tests switch it on a live context)
        ctx->content_known = content_clamp && !use_meshes && !use_meshes2d && (f->flags & RXR_FLAG_D3_ACTIVE) && !has_brush && f->tile_size > 0;
        ctx->content_row0 = std::min(content_y0, content_y1);
        ctx->content_row1 = content_y1;
        ctx->spans_active = false;
        if (ctx->content_known && spans_fit() && ctx->content_row0 < ctx->content_row1 && row_spans_on()) {
            const uint32_t r0 = ctx->content_row0 / RXR_TILE_H, r1 = std::min((ctx->content_row1 + RXR_TILE_H - 1u) / RXR_TILE_H, n_tile_rows);
            if ((rc = ship_row_spans(r0, r1, false, ctx->spans_active)) != RXR_OK) return rc;
        }
        // Device-projected 3D meshes: their boxes are made on the device, frame by frame -- the table goes there holding what is known here
        // (the pixel box of a host-projected 2D pass) and k_spans_from_meshes completes it behind the projections (render_impl).  The grid is not narrowed
        // (nothing here knows by how much); the workgroups outside the spans leave at once.  Large frames only: what a dense one pays is the
        // table's kernel, a fill launch that finds nothing to fill and the look-up in front of every tile.
        ctx->dev_spans = false;
        if (content_clamp && use_meshes && (f->flags & RXR_FLAG_D3_ACTIVE) && !has_brush && f->tile_size > 0 && spans_fit() && n_b3 &&
            n_b3 <= rxr_span_meshes_max() && (size_t)n_tile_rows * n_tile_cols >= 4u * content_min_tiles() && row_spans_on()) {
            if ((rc = ship_row_spans(0u, 0u, true, ctx->dev_spans)) != RXR_OK) return rc;
        }
        return RXR_OK;
    }

    // a frame under row spans: every triangle inside its batch's tiles, so that the bins it is counted into lie in the spans (behind
    // fill_raster_params AND content_rows_and_spans, whichever order they ran in)
    void clip_to_spans() {
        if (ctx->spans_active) ctx->P.batch_clip3d = (const uint4 *)((uint8_t *)ctx->d_frame.p + L.off_clip3d);
    }
};

}  // namespace

extern "C" int rxr_upload_frame(rxr_ctx *ctx, const rxr_frame *f) {
    if (!ctx) return RXR_ERR_INVALID;
    if (!f) return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_upload_frame: frame is NULL");
    if (ctx->group) return rxr_group_upload_frame(ctx, f);
    if (f->abi_version != RXR_ABI_VERSION) return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_upload_frame: abi_version mismatch");
    if (f->width == 0 || f->height == 0 || f->width > 32768 || f->height > 32768)
        return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_upload_frame: width/height must be in 1..32768");
    if (f->tile_size == 0) return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_upload_frame: tile_size 0 (step_by(0) panics in the reference)");
    if ((f->n_batches3d && !f->batches3d) || (f->n_batches2d && !f->batches2d) || (f->n_lights && !f->lights) ||
        (f->n_occluders && !f->occluders) || (f->n_linedefs && !f->linedefs) || (f->n_chunks && !f->chunks))
        return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_upload_frame: NULL array with non-zero count");
    if (f->background_kind > RXR_BG_GRID) return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_upload_frame: unknown background_kind");
    if (f->background_kind == RXR_BG_HOST_PIXELS && !f->background_pixels)
        return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_upload_frame: RXR_BG_HOST_PIXELS without background_pixels");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    ctx->has_frame = false;
    ctx->host_records = false;
    ctx->d3_trow0 = 0u;  // (all rows, until build_setup_records says otherwise)
    ctx->d3_trow1 = 0xFFFFFFFFu;
    // Were this frame's 3D batches handed over while they were projected (rxr_stream_begin / rxr_stream_batch3d)?  Then their arrays
    // are in the blob already, or on their way.  Anything that does not match -- a batch missing, other arrays than the ones streamed,
    // a failure on the way -- and the frame takes the plain path below from scratch.
    FrameStream &S = ctx->fstream;
    bool streamed = S.active && !S.failed.load() && !(f->use_meshes & 1u) && f->n_batches3d == S.n && S.handed.load() == S.n;
    if (S.active && streamed) {
        std::lock_guard<std::mutex> lk(S.mu);
        streamed = S.next == S.n;
        for (uint32_t i = 0; i < S.n && streamed; ++i) {
            const rxr_batch3d &b = f->batches3d[i];
            const FrameStream::Rec &R = S.rec[i];
            streamed = b.projected_vertices == R.pv && b.clipped_uvs == R.uv && b.clipped_normals == R.nrm && b.clipped_indices == R.idx &&
                       (b.edges ? (const void *)b.edges : (const void *)b.edge_visible) == R.edges && (!b.n_triangles || (b.edges ? 0 : 1) == S.edgeless.load()) &&
                       b.n_vertices == R.nv && b.n_triangles == R.nt;
        }
    }
    if (S.active && !streamed) HIPCHK(ctx, hipStreamSynchronize(ctx->stream));  // (transfers of the abandoned stream still read the staging memory)
    S.active = false;
    static const bool e2e_timing = getenv("RXR_E2E_TIMING") != nullptr;  // diagnostics (tools/e2e_probe.py)
    FrameBuild B(ctx, f, streamed);
    int rc;
    if ((rc = B.validate_and_count()) != RXR_OK) return rc;
    B.lay_out();
    if (streamed && B.L.total > S.blob_capacity) {
        // what follows the arrays does not fit the room rxr_stream_begin left: a reallocation would lose what has been shipped.  The plain
        // path from scratch (rare: the frame's lights / 2D primitives / chunk textures more than doubled against the previous frame).
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        ctx->last_blob_tail = B.L.total - B.L.off_tinfo;
        S.failed.store(1);
        return rxr_upload_frame(ctx, f);
    }
    if ((rc = B.reserve()) != RXR_OK) return rc;
    if ((rc = B.headers3d_host()) != RXR_OK) return rc;
    B.ut_headers = B.ut_ms();
    if ((rc = B.copy_arrays()) != RXR_OK) return rc;
    B.ut_arrays = B.ut_ms();
    if (B.use_meshes && (rc = B.headers3d_meshes()) != RXR_OK) return rc;
    B.write_lights_chunks_textures();
    if ((rc = B.headers2d()) != RXR_OK) return rc;
    if ((rc = B.size_scratch()) != RXR_OK) return rc;
    // (a frame whose set-up records are built here has to know first whether it takes row spans: the records go out with the blob)
    if (B.host_setup) {
        if ((rc = B.content_rows_and_spans()) != RXR_OK) return rc;
        B.build_setup_records();
    }
    if ((rc = B.ship_blob()) != RXR_OK) return rc;
    if ((rc = B.fill_raster_params()) != RXR_OK) return rc;
    if (e2e_timing)
        fprintf(stderr, "rxr_e2e_timing upload: validate+size %.3f, wait for the previous frame %.3f, headers %.3f, arrays (copy + ship) %.3f, rest %.3f ms\n", B.ut_validated,
                B.ut_quiesced - B.ut_validated, B.ut_headers - B.ut_quiesced, B.ut_arrays - B.ut_headers, B.ut_ms() - B.ut_arrays);
    ctx->n_tris2d = (uint32_t)B.t2cur;
    if (!B.host_setup && (rc = B.content_rows_and_spans()) != RXR_OK) return rc;
    B.clip_to_spans();
    ctx->host_records = B.host_setup;
    ctx->off_host_setup = B.L.off_host_setup;
    ctx->off_host_shade = B.L.off_host_shade;
    ctx->has_frame = true;
    ctx->rendered = false;
    ctx->upload_ordered_on = nullptr;
    return RXR_OK;
}
