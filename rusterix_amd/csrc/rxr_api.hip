// rxr_api.hip -- implementation of the C ABI declared in include/rxr.h (host side, compiled by hipcc).
//
// One rxr_ctx == one HIP device == one process (multi-GPU hosts run one process per GPU and gather
// the rendered row bands with RCCL, see rusterix_amd/distributed.py).
//
// This file: the context's life cycle, the resident textures / meshes / programs (with the shader flattener) and the debug hooks.
// The frame hand-over (rxr_upload_frame, rxr_stream_*) lives in rxr_upload.hip, rendering, synchronize, download and profiling in
// rxr_render.hip, multi-device handles in rxr_multi.hip, ray picking in rxr_intersect.hip.  There is no CPU fallback anywhere in this file.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <memory>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "rxr_debug.h"
#include "rxr_mesh_resize.h"
#include "rxr_query.h"

thread_local LaunchTimes *rxr_launch_times = nullptr;  // rxr_launch.h: the profiling slot of the render this thread is queueing
extern "C" void rxr_launch_proj_static(const ProjectParams *P, hipStream_t s);
extern "C" void rxr_launch_mesh_check(const MeshUpdateArgs *A, uint32_t n, hipStream_t s);
extern "C" void rxr_launch_mesh_commit(const MeshUpdateArgs *A, uint32_t n, hipStream_t s);
extern "C" void rxr_launch_mesh_resize_check(const MeshResizeCheckArgs *A, uint32_t n, hipStream_t s);
extern "C" void rxr_launch_mesh_repack(const MeshRepackArgs *A, hipStream_t s);
extern "C" void rxr_launch_proj_edges(const ProjectParams *P, hipStream_t s);
extern "C" void rxr_launch_setup(const RasterParams *P, hipStream_t s);
extern "C" void rxr_launch_selftest_math(uint64_t seed, uint32_t blocks, uint32_t iters, unsigned long long *mismatch, hipStream_t s);

namespace {

thread_local std::string g_create_error;

}  // namespace

int rxr_fail(rxr_ctx *ctx, int code, const std::string &msg) {
    if (ctx) ctx->err = msg;
    else g_create_error = msg;
    return code;
}

// Nothing this context has queued may still be running when the host rewrites the pinned staging blob, the frame blob is
// overwritten by the next host->device copy, or a scratch buffer is reallocated.  Renders issued through
// rxr_render_rows_to / rxr_render_stripes_to run on the CALLER's stream (ctx->last_stream): that one is waited for as well.
int rxr_quiesce(rxr_ctx *ctx) {
    if (ctx->last_stream && ctx->last_stream != ctx->stream) HIPCHK(ctx, hipStreamSynchronize(ctx->last_stream));
    if (ctx->copy_stream) HIPCHK(ctx, hipStreamSynchronize(ctx->copy_stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    for (QueryLane &q : ctx->lane)  // a device query on the caller's stream (rxr_ctx.h: Q_*) reads resident data and its scratch
        if (q.pending) {
            HIPCHK(ctx, hipEventSynchronize(q.ev));
            q.pending = false;
        }
    ctx->bake_jobs_used = 0;  // (every queued bake has run: the ring of program lists starts over)
    return RXR_OK;
}

int rxr_ensure(rxr_ctx *ctx, DevBuf &b, size_t bytes) {
    if (bytes <= b.cap) return RXR_OK;
    if (b.p) {
        int rc = rxr_quiesce(ctx);
        if (rc != RXR_OK) return rc;
        HIPCHK(ctx, hipFree(b.p));
        b.p = nullptr;
        b.cap = 0;
    }
    size_t cap = bytes + bytes / 4 + 4096;
    hipError_t e = hipMalloc(&b.p, cap);
    if (e != hipSuccess) return rxr_fail(ctx, RXR_ERR_OOM, std::string("hipMalloc: ") + hipGetErrorString(e));
    b.cap = cap;
    return RXR_OK;
}

int rxr_ensure_stage(rxr_ctx *ctx, size_t bytes) {
    if (bytes <= ctx->h_stage_cap) return RXR_OK;
    if (ctx->h_stage) {
        int rc = rxr_quiesce(ctx);
        if (rc != RXR_OK) return rc;
        HIPCHK(ctx, hipHostFree(ctx->h_stage));
        ctx->h_stage = nullptr;
        ctx->h_stage_cap = 0;
    }
    size_t cap = bytes + bytes / 4 + 4096;
    hipError_t e = hipHostMalloc(&ctx->h_stage, cap, hipHostMallocDefault);
    if (e != hipSuccess) return rxr_fail(ctx, RXR_ERR_OOM, std::string("hipHostMalloc: ") + hipGetErrorString(e));
    ctx->h_stage_cap = cap;
    return RXR_OK;
}

extern "C" {

int rxr_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char *rxr_last_error(const rxr_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int rxr_create(rxr_ctx **out, int device_id) {
    if (!out) return rxr_fail(nullptr, RXR_ERR_INVALID, "rxr_create: out is NULL");
    *out = nullptr;
    int n = rxr_device_count();
    if (n <= 0) return rxr_fail(nullptr, RXR_ERR_NO_DEVICE, "rxr_create: no HIP device visible (there is no CPU fallback)");
    if (device_id < 0 || device_id >= n) return rxr_fail(nullptr, RXR_ERR_NO_DEVICE, "rxr_create: device id out of range");
    rxr_ctx *ctx = new rxr_ctx();
    ctx->device = device_id;
    hipError_t e = hipSetDevice(device_id);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreate(&ctx->ev0);
    if (e == hipSuccess) e = hipEventCreate(&ctx->ev1);
    if (e == hipSuccess) e = hipEventCreate(&ctx->ev2);
    if (e == hipSuccess) e = hipEventCreate(&ctx->ev_upload);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->ev_render, hipEventDisableTiming);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking);
    for (hipEvent_t &ev : ctx->ev_band)
        if (e == hipSuccess) e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    if (e == hipSuccess) e = hipHostMalloc((void **)&ctx->h_counters, HS_WORDS * sizeof(uint32_t), hipHostMallocDefault);
    if (e == hipSuccess) e = hipHostMalloc((void **)&ctx->h_row_spans, 2u * RXR_MAX_TILE_ROWS * sizeof(uint2), hipHostMallocDefault);  // (second half: the table as the device completed it, rxr_render_download)
    if (e != hipSuccess) {
        std::string msg = std::string("rxr_create: ") + hipGetErrorString(e);
        rxr_destroy(ctx);
        return rxr_fail(nullptr, RXR_ERR_HIP, msg);
    }
    memset(ctx->h_counters, 0, HS_WORDS * sizeof(uint32_t));
    if (const char *sm = getenv("RXR_SMALL_MODE")) {
        if (sm[0] >= '0' && sm[0] <= '2') ctx->small_mode = (uint32_t)(sm[0] - '0');
    }
    if (const char *hs = getenv("RXR_HOST_SETUP")) ctx->host_setup_on = hs[0] != '0';  // tests / A-B runs: 0 keeps the k_setup3d launch of small frames
    if (const char *lf = getenv("RXR_LIST_CAPACITY_FLOOR")) {  // tests: a small floor makes ordinary scenes overflow their bin lists
        const long v = atol(lf);
        if (v > 0) ctx->list_floor = (size_t)v;
    }
    if (const char *kl = getenv("RXR_MIN_KERNEL_LEVEL")) {  // A-B runs: render with k_raster_chunk (1) / k_raster_vm (2) regardless
        if (kl[0] >= '0' && kl[0] - '0' <= (int)KL_VM) ctx->min_kernel_level = (uint32_t)(kl[0] - '0');
    }
    if (hipHostGetDevicePointer((void **)&ctx->d_host_status, ctx->h_counters, 0) != hipSuccess) ctx->d_host_status = ctx->h_counters;
    *out = ctx;
    return RXR_OK;
}

int rxr_set_light_math(rxr_ctx *ctx, int mode) {
    if (!ctx) return rxr_fail(nullptr, RXR_ERR_INVALID, "rxr_set_light_math: ctx is NULL");
    if (mode != RXR_LIGHT_MATH_EXACT && mode != RXR_LIGHT_MATH_RELAXED) return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_set_light_math: mode must be RXR_LIGHT_MATH_EXACT or RXR_LIGHT_MATH_RELAXED");
    if (ctx->group) {
        for (int i = 0; i < rxr_member_count(ctx); ++i) rxr_member(ctx, i)->relaxed_lights = mode == RXR_LIGHT_MATH_RELAXED;
    }
    ctx->relaxed_lights = mode == RXR_LIGHT_MATH_RELAXED;
    return RXR_OK;
}

void rxr_destroy(rxr_ctx *ctx) {
    if (ctx && !ctx->group && ctx->fstream.table) {
        (void)hipSetDevice(ctx->device);
        (void)hipHostFree(ctx->fstream.table);
        ctx->fstream.table = nullptr;
    }
    if (!ctx) return;
    if (ctx->group) {
        rxr_group_destroy(ctx);
        return;
    }
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)rxr_quiesce(ctx);
    DevBuf *bufs[] = {&ctx->d_stripes, &ctx->d_obj, &ctx->d_obj_alt, &ctx->d_mesh_check, &ctx->d_mirror_scratch, &ctx->d_proj_out, &ctx->d_proj_misc, &ctx->d_tex, &ctx->d_texels, &ctx->d_frame, &ctx->d_tri_setup, &ctx->d_tri_shade, &ctx->d_tri_box, &ctx->d_bin_count, &ctx->d_bins, &ctx->d_bin2d_count, &ctx->d_bins2d,
                      &ctx->d_list2d, &ctx->d_large2d,
                      &ctx->d_list, &ctx->d_large, &ctx->d_counters, &ctx->d_fb,
                      &ctx->d_vm_code, &ctx->d_programs, &ctx->d_patterns, &ctx->d_pattern_data, &ctx->d_palette,
                      &ctx->d_isect_tris, &ctx->d_isect_misc, &ctx->d_isect_keys, &ctx->d_accel_tris, &ctx->d_accel_perm, &ctx->d_accel_nodes, &ctx->d_accel_stats, &ctx->d_accel_scratch, &ctx->d_refresh_table, &ctx->d_refresh_verify, &ctx->d_trace_scene, &ctx->d_trace_paths, &ctx->d_trace_keys,
                      &ctx->d_bake_jobs, &ctx->d_bake_fault,
                      &ctx->d_terrain_cells, &ctx->d_terrain_tex, &ctx->d_terrain_texels, &ctx->d_terrain_weights,
                      &ctx->d_heights, &ctx->d_heights_tk, &ctx->d_heights_mask, &ctx->d_pheights, &ctx->d_pheights_mask, &ctx->d_flatten, &ctx->d_gen, &ctx->d_excl, &ctx->d_excl_scratch, &ctx->d_tiles, &ctx->d_nrm_scratch, &ctx->ctex.pool, &ctx->ctex.flags};
    for (DevBuf *b : bufs)
        if (b->p) (void)hipFree(b->p);
    for (QueryLane &q : ctx->lane) {
        if (q.io.p) (void)hipFree(q.io.p);
        if (q.ev) (void)hipEventDestroy(q.ev);
    }
    rxr_jit_drop(ctx);
    if (ctx->h_stage) (void)hipHostFree(ctx->h_stage);
    if (ctx->h_counters) (void)hipHostFree(ctx->h_counters);
    if (ctx->h_row_spans) (void)hipHostFree(ctx->h_row_spans);
    if (ctx->d_row_spans.p) (void)hipFree(ctx->d_row_spans.p);
    if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
    if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
    if (ctx->ev2) (void)hipEventDestroy(ctx->ev2);
    if (ctx->ev_upload) (void)hipEventDestroy(ctx->ev_upload);
    if (ctx->ev_render) (void)hipEventDestroy(ctx->ev_render);
    for (hipEvent_t e : ctx->ev_repack)
        if (e) (void)hipEventDestroy(e);
    if (ctx->h_bake_fault) (void)hipHostFree(ctx->h_bake_fault);
    if (ctx->h_bake_jobs) (void)hipHostFree(ctx->h_bake_jobs);
    for (hipEvent_t ev : ctx->ev_band)
        if (ev) (void)hipEventDestroy(ev);
    if (ctx->copy_stream) {
        (void)hipStreamSynchronize(ctx->copy_stream);
        (void)hipStreamDestroy(ctx->copy_stream);
    }
    for (ProfSlot &p : ctx->prof)
        for (hipEvent_t e : p.ev)
            if (e) (void)hipEventDestroy(e);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

int rxr_set_textures(rxr_ctx *ctx, const rxr_tile *static_tiles, uint32_t n_static, const rxr_tile *dynamic_tiles,
                     uint32_t n_dynamic) {
    if (!ctx) return RXR_ERR_INVALID;
    if ((n_static && !static_tiles) || (n_dynamic && !dynamic_tiles)) return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_set_textures: NULL tile array");
    if (ctx->group) return rxr_group_set_textures(ctx, static_tiles, n_static, dynamic_tiles, n_dynamic);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    {
        int qrc = rxr_quiesce(ctx);  // a render (possibly on the caller's stream) may still read the old texels
        if (qrc != RXR_OK) return qrc;
    }
    ctx->trace_set = false;  // (rxr_trace.hip: its mesh records name textures of the old set)
    ctx->h_tex.clear();
    ctx->tiles_static.clear();
    ctx->tiles_dynamic.clear();
    size_t texels = 0;
    auto scan = [&](const rxr_tile *tiles, uint32_t n, std::vector<TileRange> &out) -> int {
        for (uint32_t i = 0; i < n; ++i) {
            TileRange r{(uint32_t)ctx->h_tex.size(), tiles[i].n_textures};
            if (tiles[i].n_textures && !tiles[i].textures) return RXR_ERR_INVALID;
            for (uint32_t k = 0; k < tiles[i].n_textures; ++k) {
                const rxr_texture &t = tiles[i].textures[k];
                if (!t.rgba || t.width == 0 || t.height == 0 || t.width > 32768 || t.height > 32768) return RXR_ERR_INVALID;
                DevTexDesc d{};
                d.offset = (uint32_t)texels;
                d.w = t.width;
                d.h = t.height;
                bool opaque = true;
                const uint8_t *p = t.rgba;
                size_t n_px = (size_t)t.width * t.height;
                for (size_t q = 0; q < n_px; ++q)
                    if (p[q * 4 + 3] != 255) {
                        opaque = false;
                        break;
                    }
                d.all_opaque = opaque ? 1u : 0u;
                ctx->h_tex.push_back(d);
                texels += align_up(n_px, 4);
                if (texels >= (1ull << 32)) return RXR_ERR_INVALID;
            }
            out.push_back(r);
        }
        return RXR_OK;
    };
    if (scan(static_tiles, n_static, ctx->tiles_static) != RXR_OK || scan(dynamic_tiles, n_dynamic, ctx->tiles_dynamic) != RXR_OK)
        return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_set_textures: bad texture (NULL data, zero or oversized extent)");

    size_t desc_bytes = ctx->h_tex.size() * sizeof(DevTexDesc);
    size_t bytes = texels * 4;
    int rc;
    if ((rc = rxr_ensure(ctx, ctx->d_tex, desc_bytes ? desc_bytes : 16)) != RXR_OK) return rc;
    if ((rc = rxr_ensure(ctx, ctx->d_texels, bytes ? bytes : 16)) != RXR_OK) return rc;
    if ((rc = rxr_ensure_stage(ctx, bytes + desc_bytes + 64)) != RXR_OK) return rc;
    // stage texels then descriptors
    uint8_t *st = (uint8_t *)ctx->h_stage;
    size_t ti = 0;
    auto stage = [&](const rxr_tile *tiles, uint32_t n) {
        for (uint32_t i = 0; i < n; ++i)
            for (uint32_t k = 0; k < tiles[i].n_textures; ++k) {
                const rxr_texture &t = tiles[i].textures[k];
                memcpy(st + (size_t)ctx->h_tex[ti].offset * 4, t.rgba, (size_t)t.width * t.height * 4);
                ++ti;
            }
    };
    stage(static_tiles, n_static);
    stage(dynamic_tiles, n_dynamic);
    if (bytes) HIPCHK(ctx, hipMemcpyAsync(ctx->d_texels.p, st, bytes, hipMemcpyHostToDevice, ctx->stream));
    if (desc_bytes) {
        memcpy(st + bytes, ctx->h_tex.data(), desc_bytes);
        HIPCHK(ctx, hipMemcpyAsync(ctx->d_tex.p, st + bytes, desc_bytes, hipMemcpyHostToDevice, ctx->stream));
    }
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return RXR_OK;
}

// the layout of the object blob (d_obj): the packed pools, the three prefix arrays and the registration's static DevMesh table
struct ObjLayout {
    size_t off_v, off_i, off_uv, off_n, off_pv, off_pt, off_po, off_dm, total;
};
static ObjLayout obj_layout(size_t n_meshes, size_t vin, size_t tin) {
    BlobCursor take;
    ObjLayout L;
    L.off_v = take(vin * 16), L.off_i = take(tin * 12), L.off_uv = take(vin * 8), L.off_n = take(vin * 12);
    L.off_pv = take((n_meshes + 1) * 4), L.off_pt = take((n_meshes + 1) * 4), L.off_po = take((n_meshes + 1) * 4);
    L.off_dm = take(n_meshes * sizeof(DevMesh));
    L.total = take.o;
    return L;
}

// what a registration needs behind its object blob `d_obj` (laid out by L, its copy or kernel queued on `s`): the output pools and the
// projection's scratch for these totals, zeroed; ctx->PP; the static originals (k_proj_static).  Shared by rxr_set_meshes and
// rxr_resize_meshes, so that the two leave the same state.
static int proj_pools(rxr_ctx *ctx, uint32_t n_meshes, size_t vin, size_t tin, size_t vout, size_t tout, const ObjLayout &L, void *d_obj, hipStream_t s) {
    int rc;
    // ---- output pools (the arrays k_setup3d reads) + scratch ----
    BlobCursor take;
    const size_t q_vs = take(vout * 16), q_pv = take(vout * 16), q_uv = take(vout * 8), q_nrm = take(vout * 12);
    const size_t q_idx = take(tout * 12), q_edges = take(tout * sizeof(rxr_edges));
    const size_t out_total = take.o;
    if ((rc = rxr_ensure(ctx, ctx->d_proj_out, out_total)) != RXR_OK) return rc;
    HIPCHK(ctx, hipMemsetAsync(ctx->d_proj_out.p, 0, out_total, s));  // indices 0 / edges invisible until written
    take.o = 0;
    const size_t n_chunks = (tin + 1 + RXR_PROJ_SCAN_CHUNK - 1) / RXR_PROJ_SCAN_CHUNK + 1;
    const size_t m_evis = take(tin + 1), m_app = take((tin + 1) * 8), m_ct = take(n_chunks * 8), m_cb = take(n_chunks * 8);
    const size_t m_ticket = take(16), m_bbox = take((size_t)n_meshes * sizeof(DevBBox));
    const size_t m_dm = take((size_t)n_meshes * sizeof(DevMesh));
    const size_t m_live = take((size_t)n_meshes * sizeof(uint32_t));
    if ((rc = rxr_ensure(ctx, ctx->d_proj_misc, take.o)) != RXR_OK) return rc;
    HIPCHK(ctx, hipMemsetAsync(ctx->d_proj_misc.p, 0, take.o, s));
    ctx->pp_off_meshes = m_dm;
    ctx->obj_off_meshes = L.off_dm;

    ProjectParams &PP = ctx->PP;
    memset(&PP, 0, sizeof(PP));
    PP.n_meshes = n_meshes;
    PP.n_verts_in = (uint32_t)vin;
    PP.n_tris_in = (uint32_t)tin;
    PP.n_tris_out = (uint32_t)tout;
    uint8_t *d = (uint8_t *)d_obj, *q = (uint8_t *)ctx->d_proj_out.p, *mm = (uint8_t *)ctx->d_proj_misc.p;
    PP.meshes = (const DevMesh *)(d + L.off_dm);  // static copy; replaced by the per-frame array at render time
    PP.vin_prefix = (const uint32_t *)(d + L.off_pv);
    PP.tin_prefix = (const uint32_t *)(d + L.off_pt);
    PP.tout_prefix = (const uint32_t *)(d + L.off_po);
    PP.obj_verts = (const float4 *)(d + L.off_v);
    PP.obj_idx = (const uint32_t *)(d + L.off_i);
    PP.obj_uvs = (const float2 *)(d + L.off_uv);
    PP.obj_normals = (const float *)(d + L.off_n);
    PP.view_verts = (float4 *)(q + q_vs);
    PP.pv = (float4 *)(q + q_pv);
    PP.uv = (float2 *)(q + q_uv);
    PP.nrm = (float *)(q + q_nrm);
    PP.idx = (uint32_t *)(q + q_idx);
    PP.edges = (rxr_edges *)(q + q_edges);
    PP.edge_vis = (uint8_t *)(mm + m_evis);
    PP.append = (AppendCount *)(mm + m_app);
    PP.chunk_tot = (AppendCount *)(mm + m_ct);
    PP.chunk_base = (AppendCount *)(mm + m_cb);
    PP.ticket = (uint32_t *)(mm + m_ticket);
    PP.bbox = (DevBBox *)(mm + m_bbox);
    PP.mesh_live = (uint32_t *)(mm + m_live);
    rxr_launch_proj_static(&PP, s);
    HIPCHK(ctx, hipGetLastError());
    return RXR_OK;
}

int rxr_set_meshes(rxr_ctx *ctx, const rxr_mesh3d *meshes, uint32_t n_meshes) {
    if (!ctx) return RXR_ERR_INVALID;
    if (n_meshes && !meshes) return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_set_meshes: NULL mesh array");
    if (ctx->group) return rxr_group_set_meshes(ctx, meshes, n_meshes);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    {
        int qrc = rxr_quiesce(ctx);
        if (qrc != RXR_OK) return qrc;
    }
    ctx->meshes.clear();
    ctx->has_frame = false;
    ctx->meshes_valid = false;  // (rxr_intersect.hip: until this call completes)
    ctx->isect_ready = false;
    ctx->refresh_named.clear();   // (meshes pending a ranged refresh: the next query takes the full path)
    ctx->refresh_pending = 0;
    ctx->trace_set = false;
    size_t vin = 0, tin = 0, vout = 0, tout = 0;
    for (uint32_t i = 0; i < n_meshes; ++i) {
        const rxr_mesh3d &m = meshes[i];
        if (m.n_vertices && (!m.vertices || !m.uvs)) return rxr_fail(ctx, RXR_ERR_INVALID, "mesh: NULL vertex arrays");
        if (m.n_triangles && !m.indices) return rxr_fail(ctx, RXR_ERR_INVALID, "mesh: NULL indices");
        if (m.n_triangles && !m.normals)
            return rxr_fail(ctx, RXR_ERR_INVALID, "mesh without normals (clip_and_project panics at batch3d.rs:605)");
        if (m.cull_mode > RXR_CULL_BACK) return rxr_fail(ctx, RXR_ERR_INVALID, "mesh: bad cull mode");
        for (size_t t = 0; t < (size_t)m.n_triangles * 3u; ++t)
            if (m.indices[t] >= m.n_vertices) return rxr_fail(ctx, RXR_ERR_INVALID, "mesh: vertex index out of range");
        HostMesh h{};
        h.dev.vin_base = (uint32_t)vin;
        h.dev.tin_base = (uint32_t)tin;
        h.dev.n_verts = m.n_vertices;
        h.dev.n_tris = m.n_triangles;
        h.dev.vout_base = (uint32_t)vout;
        h.dev.tout_base = (uint32_t)tout;
        h.dev.cull_mode = m.cull_mode;
        memcpy(h.transform, m.transform_3d, 64);
        // object-space AABB with f32::min / f32::max semantics (batch3d.rs:494-507)
        for (int k = 0; k < 3; ++k) {
            h.aabb_lo[k] = INFINITY;
            h.aabb_hi[k] = -INFINITY;
        }
        for (uint32_t v = 0; v < m.n_vertices; ++v)
            for (int k = 0; k < 3; ++k) {
                h.aabb_lo[k] = std::fmin(h.aabb_lo[k], m.vertices[4 * (size_t)v + k]);
                h.aabb_hi[k] = std::fmax(h.aabb_hi[k], m.vertices[4 * (size_t)v + k]);
            }
        h.has_vertices = m.n_vertices > 0;
        h.repeat_mode = m.repeat_mode;
        h.source = m.source;
        memcpy(h.ambient, m.ambient_color, 12);
        h.shader = m.shader;
        h.has_profile_id = m.has_profile_id;
        h.profile_id = m.profile_id;
        h.list = m.list;
        h.chunk = m.chunk;
        ctx->meshes.push_back(h);
        vin += m.n_vertices;
        tin += m.n_triangles;
        vout += (size_t)m.n_vertices + 4 * (size_t)m.n_triangles;
        tout += 3 * (size_t)m.n_triangles;
    }
    if (vout >= (1ull << 31) || tout >= (1ull << 31)) return rxr_fail(ctx, RXR_ERR_INVALID, "meshes too large (>= 2^31 output slots)");
    ctx->mesh_verts_out = vout;
    ctx->mesh_tris_out = tout;

    // ---- object-space pools + static prefix arrays: one staging blob, one copy ----
    const ObjLayout L = obj_layout(n_meshes, vin, tin);
    const size_t off_v = L.off_v, off_i = L.off_i, off_uv = L.off_uv, off_n = L.off_n, off_pv = L.off_pv, off_pt = L.off_pt, off_po = L.off_po, off_dm = L.off_dm;
    const size_t obj_total = L.total;
    int rc;
    if ((rc = rxr_ensure_stage(ctx, obj_total)) != RXR_OK) return rc;
    if ((rc = rxr_ensure(ctx, ctx->d_obj, obj_total)) != RXR_OK) return rc;
    uint8_t *st = (uint8_t *)ctx->h_stage;
    uint32_t *pv = (uint32_t *)(st + off_pv), *pt = (uint32_t *)(st + off_pt), *po = (uint32_t *)(st + off_po);
    DevMesh *dm = (DevMesh *)(st + off_dm);
    for (uint32_t i = 0; i < n_meshes; ++i) {
        const rxr_mesh3d &m = meshes[i];
        const HostMesh &h = ctx->meshes[i];
        pv[i] = h.dev.vin_base;
        pt[i] = h.dev.tin_base;
        po[i] = h.dev.tout_base;
        dm[i] = h.dev;
        if (m.n_vertices) {
            memcpy(st + off_v + (size_t)h.dev.vin_base * 16, m.vertices, (size_t)m.n_vertices * 16);
            memcpy(st + off_uv + (size_t)h.dev.vin_base * 8, m.uvs, (size_t)m.n_vertices * 8);
            if (m.normals) memcpy(st + off_n + (size_t)h.dev.vin_base * 12, m.normals, (size_t)m.n_vertices * 12);
            else memset(st + off_n + (size_t)h.dev.vin_base * 12, 0, (size_t)m.n_vertices * 12);
        }
        if (m.n_triangles) memcpy(st + off_i + (size_t)h.dev.tin_base * 12, m.indices, (size_t)m.n_triangles * 12);
    }
    pv[n_meshes] = (uint32_t)vin;
    pt[n_meshes] = (uint32_t)tin;
    po[n_meshes] = (uint32_t)tout;
    HIPCHK(ctx, hipMemcpyAsync(ctx->d_obj.p, st, obj_total, hipMemcpyHostToDevice, ctx->stream));

    if ((rc = proj_pools(ctx, n_meshes, vin, tin, vout, tout, L, ctx->d_obj.p, ctx->stream)) != RXR_OK) return rc;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->meshes_valid = true;
    return RXR_OK;
}

// ---- rxr_update_meshes: registered meshes' geometry replaced in place (kernels: rxr_project.hip) ------------------------------
// what both forms refuse before anything is queued, but for their pointers; bytes[4]: the arrays' sizes
// (against_registration false: rxr_resize_meshes, whose strides bound the NEW counts -- the check kernel compares those)
static int update_check(rxr_ctx *ctx, const char *who, const uint32_t *mesh_indices, uint32_t n, uint32_t vstride, uint32_t tstride, size_t bytes[4],
                        bool against_registration = true) {
    const std::string w = who;
    if (!ctx->meshes_valid) return rxr_fail(ctx, RXR_ERR_INVALID, w + ": no valid registration (the last rxr_set_meshes failed)");
    if (!mesh_indices) return rxr_fail(ctx, RXR_ERR_INVALID, w + ": NULL mesh_indices");
    // (the sizes depend on n and the strides alone: refused before anything is read)
    const size_t per[4] = {8, (size_t)vstride * 16, (size_t)tstride * 12, (size_t)vstride * 12};
    for (int i = 0; i < 4; ++i)
        if (__builtin_mul_overflow((size_t)n, per[i], &bytes[i])) return rxr_fail(ctx, RXR_ERR_INVALID, w + ": the arrays' sizes overflow");
    if (n > ctx->meshes.size())
        return rxr_fail(ctx, RXR_ERR_INVALID, w + ": " + std::to_string(n) + " meshes named, " + std::to_string(ctx->meshes.size()) + " are registered (no such mesh, or one named twice)");
    std::vector<uint8_t> named(ctx->meshes.size(), 0);
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t m = mesh_indices[i];
        const std::string at = w + ": mesh_indices[" + std::to_string(i) + "] = " + std::to_string(m);
        if (m >= ctx->meshes.size()) return rxr_fail(ctx, RXR_ERR_INVALID, at + ": no such mesh (" + std::to_string(ctx->meshes.size()) + " are registered)");
        if (named[m]) return rxr_fail(ctx, RXR_ERR_INVALID, at + ": named twice");
        named[m] = 1;
        if (!against_registration) continue;
        const DevMesh &M = ctx->meshes[m].dev;
        if (M.n_verts > vstride) return rxr_fail(ctx, RXR_ERR_INVALID, at + ": vertex_stride " + std::to_string(vstride) + " is below its " + std::to_string(M.n_verts) + " vertices");
        if (M.n_tris > tstride) return rxr_fail(ctx, RXR_ERR_INVALID, at + ": triangle_stride " + std::to_string(tstride) + " is below its " + std::to_string(M.n_tris) + " triangles");
    }
    return RXR_OK;
}

// both phases on `s` over DEVICE arrays; the streams are idle (rxr_quiesce) and stay so until this returns
static int update_run(rxr_ctx *ctx, const char *who, const uint32_t *mesh_indices, uint32_t n, const uint32_t *counts, const float *vertices,
                      const uint32_t *indices, const float *normals, uint32_t vstride, uint32_t tstride, hipStream_t s) {
    int rc = rxr_ensure(ctx, ctx->d_mesh_check, (size_t)n * sizeof(MeshCheckRec));
    if (rc != RXR_OK) return rc;
    const ProjectParams &PP = ctx->PP;
    MeshUpdateArgs A{};
    A.meshes = (const DevMesh *)((const uint8_t *)ctx->d_obj.p + ctx->obj_off_meshes);
    A.vstride = vstride;
    A.tstride = tstride;
    A.obj_verts = const_cast<float4 *>(PP.obj_verts);
    A.obj_idx = const_cast<uint32_t *>(PP.obj_idx);
    A.obj_normals = const_cast<float *>(PP.obj_normals);
    A.nrm = PP.nrm;
    A.idx = PP.idx;
    auto each_launch = [&](void (*launch)(const MeshUpdateArgs *, uint32_t, hipStream_t)) -> int {
        for (uint32_t c0 = 0; c0 < n; c0 += RXR_MESH_UPDATE_LAUNCH) {
            const uint32_t nc = std::min(n - c0, RXR_MESH_UPDATE_LAUNCH);
            memcpy(A.mesh, mesh_indices + c0, (size_t)nc * sizeof(uint32_t));
            A.counts = counts + 2 * (size_t)c0;
            A.vertices = vertices + (size_t)c0 * vstride * 4;
            A.indices = indices + (size_t)c0 * tstride * 3;
            A.normals = normals + (size_t)c0 * vstride * 3;
            A.rec = (MeshCheckRec *)ctx->d_mesh_check.p + c0;
            launch(&A, nc, s);
            HIPCHK(ctx, hipGetLastError());
        }
        return RXR_OK;
    };
    // phase 1: nothing is written but the records
    if ((rc = each_launch(rxr_launch_mesh_check)) != RXR_OK) return rc;
    std::vector<MeshCheckRec> rec(n);
    HIPCHK(ctx, hipMemcpyAsync(rec.data(), ctx->d_mesh_check.p, (size_t)n * sizeof(MeshCheckRec), hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    for (uint32_t i = 0; i < n; ++i) {
        if (!rec[i].status) continue;
        const DevMesh &M = ctx->meshes[mesh_indices[i]].dev;
        std::string why;
        if (rec[i].status & MESH_UPD_BAD_VERTS) why = "its vertex count differs from the registered " + std::to_string(M.n_verts);
        else if (rec[i].status & MESH_UPD_BAD_TRIS) why = "its triangle count differs from the registered " + std::to_string(M.n_tris);
        else why = "triangle " + std::to_string(rec[i].bad_triangle) + " has a vertex index that is not below its " + std::to_string(M.n_verts) + " vertices";
        return rxr_fail(ctx, RXR_ERR_INVALID, std::string(who) + ": mesh_indices[" + std::to_string(i) + "] = " + std::to_string(mesh_indices[i]) + ": " + why +
                                                  " (nothing was changed; register again with rxr_set_meshes)");
    }
    // phase 2
    if ((rc = each_launch(rxr_launch_mesh_commit)) != RXR_OK) return rc;
    HIPCHK(ctx, hipStreamSynchronize(s));
    for (uint32_t i = 0; i < n; ++i) {
        HostMesh &h = ctx->meshes[mesh_indices[i]];
        memcpy(h.aabb_lo, rec[i].lo, 12);
        memcpy(h.aabb_hi, rec[i].hi, 12);
    }
    if (ctx->refresh_mode == RXR_RAY_REFRESH_RANGED && ctx->isect_ready) {
        // the records stay; the next pick rewrites the named meshes' (rxr_set_ray_refresh; without records there is nothing to keep)
        ctx->refresh_named.resize(ctx->meshes.size(), 0);
        for (uint32_t i = 0; i < n; ++i) {
            uint8_t &named = ctx->refresh_named[mesh_indices[i]];
            ctx->refresh_pending += named ? 0u : 1u;
            named = 1;
        }
    } else {
        ctx->isect_ready = false;  // (the next pick builds its records again, as after rxr_set_meshes)
    }
    ctx->has_frame = false;    // (the resident frame's cull decisions and row spans came from the old boxes)
    return RXR_OK;
}

int rxr_update_meshes(rxr_ctx *ctx, const uint32_t *mesh_indices, uint32_t n, const uint32_t *counts, const float *vertices, const uint32_t *indices,
                      const float *normals, uint32_t vertex_stride, uint32_t triangle_stride) {
    if (!ctx) return RXR_ERR_INVALID;
    if (ctx->group) return rxr_group_update_meshes(ctx, mesh_indices, n, counts, vertices, indices, normals, vertex_stride, triangle_stride);
    if (!n) return RXR_OK;
    size_t bytes[4];
    int rc = update_check(ctx, "rxr_update_meshes", mesh_indices, n, vertex_stride, triangle_stride, bytes);
    if (rc != RXR_OK) return rc;
    const void *arrays[4] = {counts, vertices, indices, normals};
    for (int i = 0; i < 4; ++i)
        if (bytes[i] && !arrays[i]) return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_update_meshes: NULL array");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if ((rc = rxr_quiesce(ctx)) != RXR_OK) return rc;   // renders and picks read the pools
    QueryLane &lane = ctx->lane[Q_MESH_UPDATE];
    QueryIO io{ctx, lane};
    // (an array of 0 bytes -- a stride of 0, every named mesh empty -- is not staged; the kernels never read it)
    const unsigned i_c = io.in(counts, bytes[0]), i_v = io.in(bytes[1] ? vertices : nullptr, bytes[1]), i_i = io.in(bytes[2] ? indices : nullptr, bytes[2]),
                   i_n = io.in(bytes[3] ? normals : nullptr, bytes[3]);
    if ((rc = io.upload()) != RXR_OK) return rc;
    rc = update_run(ctx, "rxr_update_meshes", mesh_indices, n, io.dev<uint32_t>(i_c), io.dev<float>(i_v), io.dev<uint32_t>(i_i), io.dev<float>(i_n), vertex_stride,
                    triangle_stride, ctx->stream);
    if (rc != RXR_OK) (void)hipStreamSynchronize(ctx->stream);   // (the caller's arrays have been read before the call returns)
    return rc;
}

int rxr_update_meshes_to(rxr_ctx *ctx, const uint32_t *mesh_indices, uint32_t n, const uint32_t *dev_counts, const float *dev_vertices,
                         const uint32_t *dev_indices, const float *dev_normals, uint32_t vertex_stride, uint32_t triangle_stride, void *hip_stream) {
    if (!ctx) return RXR_ERR_INVALID;
    if (ctx->group) return rxr_fail(ctx, RXR_ERR_UNSUPPORTED, "rxr_update_meshes_to on a multi-device context: device pointers and streams belong to ONE device (use rxr_member)");
    if (!n) return RXR_OK;
    size_t bytes[4];
    int rc = update_check(ctx, "rxr_update_meshes_to", mesh_indices, n, vertex_stride, triangle_stride, bytes);
    if (rc != RXR_OK) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const struct {
        const void *p;
        const char *name;
    } arrays[4] = {{dev_counts, "dev_counts"}, {dev_vertices, "dev_vertices"}, {dev_indices, "dev_indices"}, {dev_normals, "dev_normals"}};
    for (int i = 0; i < 4; ++i) {
        if (!bytes[i]) continue;   // (strides of 0: every named mesh is empty, the array is not looked at)
        if (!arrays[i].p || ((uintptr_t)arrays[i].p & 3u))
            return rxr_fail(ctx, RXR_ERR_INVALID, std::string("rxr_update_meshes_to: ") + arrays[i].name + " must be 4-byte aligned device memory");
        if (!rxr_on_device(ctx, arrays[i].p, bytes[i]))
            return rxr_fail(ctx, RXR_ERR_INVALID, std::string("rxr_update_meshes_to: ") + arrays[i].name + " is not device memory of the context's device (or is too small)");
    }
    if ((rc = rxr_quiesce(ctx)) != RXR_OK) return rc;   // renders and picks read the pools
    return update_run(ctx, "rxr_update_meshes_to", mesh_indices, n, dev_counts, dev_vertices, dev_indices, dev_normals, vertex_stride, triangle_stride,
                      hip_stream ? (hipStream_t)hip_stream : ctx->stream);
}

// ---- rxr_resize_meshes: registered meshes whose counts change (kernels: rxr_project.hip; the layout arithmetic: rxr_mesh_resize.h) --------
// Over DEVICE arrays on `s`; the streams are idle (rxr_quiesce) and stay so until this returns.  Three steps: the check kernel and its
// records (a refusal changes nothing); the new layout, on the host in O(registered meshes); the new object blob built in d_obj_alt from
// d_obj and the caller's arrays, the output pools as rxr_set_meshes makes them, and only then the swap.
static int resize_run(rxr_ctx *ctx, const char *who, const uint32_t *mesh_indices, uint32_t n, const uint32_t *counts, const float *vertices, const float *uvs,
                      const uint32_t *indices, const float *normals, uint32_t vstride, uint32_t tstride, hipStream_t s) {
    int rc = rxr_ensure(ctx, ctx->d_mesh_check, (size_t)n * sizeof(MeshResizeRec));
    if (rc != RXR_OK) return rc;
    MeshResizeCheckArgs C{};
    C.counts = counts;
    C.vertices = vertices;
    C.indices = indices;
    C.vstride = vstride;
    C.tstride = tstride;
    C.rec = (MeshResizeRec *)ctx->d_mesh_check.p;
    rxr_launch_mesh_resize_check(&C, n, s);
    HIPCHK(ctx, hipGetLastError());
    std::vector<MeshResizeRec> rec(n);
    HIPCHK(ctx, hipMemcpyAsync(rec.data(), ctx->d_mesh_check.p, (size_t)n * sizeof(MeshResizeRec), hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    const std::string w = who;
    auto at = [&](uint32_t i) { return w + ": mesh_indices[" + std::to_string(i) + "] = " + std::to_string(mesh_indices[i]) + ": "; };
    const char *unchanged = " (nothing was changed)";
    for (uint32_t i = 0; i < n; ++i) {
        if (!rec[i].status) continue;
        std::string why;
        if (rec[i].status & MESH_RSZ_BAD_VSTRIDE) why = "its " + std::to_string(rec[i].n_verts) + " vertices exceed vertex_stride " + std::to_string(vstride);
        else if (rec[i].status & MESH_RSZ_BAD_TSTRIDE) why = "its " + std::to_string(rec[i].n_tris) + " triangles exceed triangle_stride " + std::to_string(tstride);
        else why = "triangle " + std::to_string(rec[i].bad_triangle) + " has a vertex index that is not below its " + std::to_string(rec[i].n_verts) + " vertices";
        return rxr_fail(ctx, RXR_ERR_INVALID, at(i) + why + unchanged);
    }
    // the new layout
    const uint32_t n_meshes = (uint32_t)ctx->meshes.size();
    std::vector<uint32_t> all_counts(2 * (size_t)n_meshes), slot(n_meshes, 0xFFFFFFFFu), bases(4 * (size_t)n_meshes);
    for (uint32_t m = 0; m < n_meshes; ++m) {
        all_counts[2 * (size_t)m] = ctx->meshes[m].dev.n_verts;
        all_counts[2 * (size_t)m + 1] = ctx->meshes[m].dev.n_tris;
    }
    for (uint32_t i = 0; i < n; ++i) {
        slot[mesh_indices[i]] = i;
        all_counts[2 * (size_t)mesh_indices[i]] = rec[i].n_verts;
        all_counts[2 * (size_t)mesh_indices[i] + 1] = rec[i].n_tris;
    }
    uint64_t totals[4];
    const size_t reached = rxr_resize_bases(all_counts.data(), n_meshes, bases.data(), totals);
    if (reached != n_meshes) {
        // the old registration fitted, so a named mesh at or before `reached` grew: the last of them is the one the message names
        uint32_t i = 0xFFFFFFFFu;
        for (uint32_t k = 0; k < n; ++k)
            if (mesh_indices[k] <= reached && (i == 0xFFFFFFFFu || mesh_indices[k] > mesh_indices[i])) i = k;
        if (i == 0xFFFFFFFFu) i = 0;
        return rxr_fail(ctx, RXR_ERR_INVALID, at(i) + "with its " + std::to_string(rec[i].n_verts) + " vertices and " + std::to_string(rec[i].n_tris) +
                                                  " triangles the meshes are too large (>= 2^31 output slots at mesh " + std::to_string(reached) + ")" + unchanged);
    }
    const size_t vin = totals[0], tin = totals[1], vout = totals[2], tout = totals[3];

    // ---- accepted.  The small tables go through the staging blob; the new pools are built next to the old ones ----
    const HostMesh &last = ctx->meshes[n_meshes - 1];   // (n >= 1 named meshes passed update_check: there is one)
    const ObjLayout L = obj_layout(n_meshes, vin, tin), L0 = obj_layout(n_meshes, (size_t)last.dev.vin_base + last.dev.n_verts, (size_t)last.dev.tin_base + last.dev.n_tris);
    BlobCursor take;
    take.o = L.total;
    const size_t off_src = take((size_t)n_meshes * 8);
    const size_t blob_total = take.o, tables = blob_total - L.off_pv;
    if ((rc = rxr_ensure_stage(ctx, tables)) != RXR_OK) return rc;
    if ((rc = rxr_ensure(ctx, ctx->d_obj_alt, blob_total)) != RXR_OK) return rc;   // (a failure here: the old registration stays in use)
    uint8_t *st = (uint8_t *)ctx->h_stage;   // (the staged range is [off_pv, blob_total) of the blob)
    uint32_t *pv = (uint32_t *)st, *pt = (uint32_t *)(st + (L.off_pt - L.off_pv)), *po = (uint32_t *)(st + (L.off_po - L.off_pv)), *src = (uint32_t *)(st + (off_src - L.off_pv));
    DevMesh *dm = (DevMesh *)(st + (L.off_dm - L.off_pv));
    for (uint32_t m = 0; m < n_meshes; ++m) {
        DevMesh d = ctx->meshes[m].dev;
        src[2 * (size_t)m] = slot[m] != 0xFFFFFFFFu ? (RXR_MESH_RESIZE_NAMED | slot[m]) : d.vin_base;   // (the OLD bases)
        src[2 * (size_t)m + 1] = slot[m] != 0xFFFFFFFFu ? 0u : d.tin_base;
        d.vin_base = bases[4 * (size_t)m], d.tin_base = bases[4 * (size_t)m + 1], d.vout_base = bases[4 * (size_t)m + 2], d.tout_base = bases[4 * (size_t)m + 3];
        d.n_verts = all_counts[2 * (size_t)m], d.n_tris = all_counts[2 * (size_t)m + 1];
        pv[m] = d.vin_base, pt[m] = d.tin_base, po[m] = d.tout_base;
        dm[m] = d;
    }
    pv[n_meshes] = (uint32_t)vin, pt[n_meshes] = (uint32_t)tin, po[n_meshes] = (uint32_t)tout;
    uint8_t *d0 = (uint8_t *)ctx->d_obj.p, *d1 = (uint8_t *)ctx->d_obj_alt.p;
    HIPCHK(ctx, hipMemcpyAsync(d1 + L.off_pv, ctx->h_stage, tables, hipMemcpyHostToDevice, s));
    MeshRepackArgs R{};
    R.n_meshes = n_meshes, R.n_verts = (uint32_t)vin, R.n_tris = (uint32_t)tin;
    R.meshes = (const DevMesh *)(d1 + L.off_dm);
    R.vin_prefix = (const uint32_t *)(d1 + L.off_pv), R.tin_prefix = (const uint32_t *)(d1 + L.off_pt);
    R.source = (const uint32_t *)(d1 + off_src);
    R.old_verts = (const uint4 *)(d0 + L0.off_v), R.old_idx = (const uint32_t *)(d0 + L0.off_i);
    R.old_uvs = (const uint2 *)(d0 + L0.off_uv), R.old_normals = (const uint32_t *)(d0 + L0.off_n);
    R.vertices = (const uint32_t *)vertices, R.uvs = (const uint32_t *)uvs, R.indices = indices, R.normals = (const uint32_t *)normals;
    R.vstride = vstride, R.tstride = tstride;
    R.new_verts = (uint4 *)(d1 + L.off_v), R.new_idx = (uint32_t *)(d1 + L.off_i);
    R.new_uvs = (uint2 *)(d1 + L.off_uv), R.new_normals = (uint32_t *)(d1 + L.off_n);
    for (hipEvent_t &e : ctx->ev_repack)
        if (!e) HIPCHK(ctx, hipEventCreate(&e));
    HIPCHK(ctx, hipEventRecord(ctx->ev_repack[0], s));
    rxr_launch_mesh_repack(&R, s);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipEventRecord(ctx->ev_repack[1], s));
    ctx->repack_bytes = (uint64_t)vin * 36 + (uint64_t)tin * 12;

    // from here on as rxr_set_meshes: no valid registration until the call completes
    ctx->has_frame = false;
    ctx->meshes_valid = false;
    ctx->isect_ready = false;
    ctx->refresh_named.clear();
    ctx->refresh_pending = 0;
    ctx->trace_set = false;
    if ((rc = proj_pools(ctx, n_meshes, vin, tin, vout, tout, L, d1, s)) != RXR_OK) return rc;
    HIPCHK(ctx, hipStreamSynchronize(s));
    std::swap(ctx->d_obj, ctx->d_obj_alt);
    ctx->mesh_verts_out = vout;
    ctx->mesh_tris_out = tout;
    for (uint32_t m = 0; m < n_meshes; ++m) {
        HostMesh &h = ctx->meshes[m];
        h.dev.vin_base = bases[4 * (size_t)m], h.dev.tin_base = bases[4 * (size_t)m + 1], h.dev.vout_base = bases[4 * (size_t)m + 2], h.dev.tout_base = bases[4 * (size_t)m + 3];
        h.dev.n_verts = all_counts[2 * (size_t)m], h.dev.n_tris = all_counts[2 * (size_t)m + 1];
        if (slot[m] != 0xFFFFFFFFu) {
            memcpy(h.aabb_lo, rec[slot[m]].lo, 12);
            memcpy(h.aabb_hi, rec[slot[m]].hi, 12);
            h.has_vertices = h.dev.n_verts > 0;
        }
    }
    ctx->meshes_valid = true;
    return RXR_OK;
}

int rxr_resize_meshes(rxr_ctx *ctx, const uint32_t *mesh_indices, uint32_t n, const uint32_t *counts, const float *vertices, const float *uvs,
                      const uint32_t *indices, const float *normals, uint32_t vertex_stride, uint32_t triangle_stride) {
    if (!ctx) return RXR_ERR_INVALID;
    if (ctx->group) return rxr_group_resize_meshes(ctx, mesh_indices, n, counts, vertices, uvs, indices, normals, vertex_stride, triangle_stride);
    if (!n) return RXR_OK;
    size_t bytes[4];
    int rc = update_check(ctx, "rxr_resize_meshes", mesh_indices, n, vertex_stride, triangle_stride, bytes, false);
    if (rc != RXR_OK) return rc;
    const void *arrays[4] = {counts, vertices, indices, normals};
    for (int i = 0; i < 4; ++i)
        if (bytes[i] && !arrays[i]) return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_resize_meshes: NULL array");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if ((rc = rxr_quiesce(ctx)) != RXR_OK) return rc;   // renders and picks read the pools
    QueryLane &lane = ctx->lane[Q_MESH_UPDATE];
    QueryIO io{ctx, lane};
    const size_t uv_bytes = uvs ? bytes[1] / 2 : 0;
    const unsigned i_c = io.in(counts, bytes[0]), i_v = io.in(bytes[1] ? vertices : nullptr, bytes[1]), i_u = io.in(uv_bytes ? uvs : nullptr, uv_bytes),
                   i_i = io.in(bytes[2] ? indices : nullptr, bytes[2]), i_n = io.in(bytes[3] ? normals : nullptr, bytes[3]);
    if ((rc = io.upload()) != RXR_OK) return rc;
    rc = resize_run(ctx, "rxr_resize_meshes", mesh_indices, n, io.dev<uint32_t>(i_c), io.dev<float>(i_v), io.dev<float>(i_u), io.dev<uint32_t>(i_i), io.dev<float>(i_n),
                    vertex_stride, triangle_stride, ctx->stream);
    if (rc != RXR_OK) (void)hipStreamSynchronize(ctx->stream);   // (the caller's arrays have been read before the call returns)
    return rc;
}

int rxr_resize_meshes_to(rxr_ctx *ctx, const uint32_t *mesh_indices, uint32_t n, const uint32_t *dev_counts, const float *dev_vertices, const float *dev_uvs,
                         const uint32_t *dev_indices, const float *dev_normals, uint32_t vertex_stride, uint32_t triangle_stride, void *hip_stream) {
    if (!ctx) return RXR_ERR_INVALID;
    if (ctx->group) return rxr_fail(ctx, RXR_ERR_UNSUPPORTED, "rxr_resize_meshes_to on a multi-device context: device pointers and streams belong to ONE device (use rxr_member)");
    if (!n) return RXR_OK;
    size_t bytes[4];
    int rc = update_check(ctx, "rxr_resize_meshes_to", mesh_indices, n, vertex_stride, triangle_stride, bytes, false);
    if (rc != RXR_OK) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const struct {
        const void *p;
        const char *name;
        size_t bytes;
        bool optional;
    } arrays[5] = {{dev_counts, "dev_counts", bytes[0], false}, {dev_vertices, "dev_vertices", bytes[1], false}, {dev_uvs, "dev_uvs", bytes[1] / 2, true},
                   {dev_indices, "dev_indices", bytes[2], false}, {dev_normals, "dev_normals", bytes[3], false}};
    for (int i = 0; i < 5; ++i) {
        if (!arrays[i].bytes || (arrays[i].optional && !arrays[i].p)) continue;   // (strides of 0: the array is not looked at; no uvs: [0, 0])
        if (!arrays[i].p || ((uintptr_t)arrays[i].p & 3u))
            return rxr_fail(ctx, RXR_ERR_INVALID, std::string("rxr_resize_meshes_to: ") + arrays[i].name + " must be 4-byte aligned device memory");
        if (!rxr_on_device(ctx, arrays[i].p, arrays[i].bytes))
            return rxr_fail(ctx, RXR_ERR_INVALID, std::string("rxr_resize_meshes_to: ") + arrays[i].name + " is not device memory of the context's device (or is too small)");
    }
    if ((rc = rxr_quiesce(ctx)) != RXR_OK) return rc;   // renders and picks read the pools
    return resize_run(ctx, "rxr_resize_meshes_to", mesh_indices, n, dev_counts, dev_vertices, bytes[1] ? dev_uvs : nullptr, dev_indices, dev_normals, vertex_stride,
                      triangle_stride, hip_stream ? (hipStream_t)hip_stream : ctx->stream);
}

// tools/mesh_resize_bench.py: the stream time of the last accepted resize's k_mesh_repack, the time of one device-to-device copy of
// the bytes it wrote (old blob -> spare blob, after a warm-up copy: the yardstick of a memory-bound kernel) and that byte count
int rxr_debug_resize_repack(rxr_ctx *ctx, float *us2, uint64_t *bytes) {
    if (!ctx || ctx->group || !us2 || !bytes) return RXR_ERR_INVALID;
    if (!ctx->ev_repack[1] || !ctx->meshes_valid) return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_debug_resize_repack: no accepted resize yet");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc = rxr_quiesce(ctx);
    if (rc != RXR_OK) return rc;
    float ms = 0.0f;
    HIPCHK(ctx, hipEventElapsedTime(&ms, ctx->ev_repack[0], ctx->ev_repack[1]));
    us2[0] = ms * 1000.0f;
    const size_t n = std::min<size_t>({(size_t)ctx->repack_bytes, ctx->d_obj.cap, ctx->d_obj_alt.cap});
    *bytes = n;
    us2[1] = 0.0f;
    if (!n) return RXR_OK;
    hipEvent_t e0, e1;   // (the repack's own pair keeps its times)
    HIPCHK(ctx, hipEventCreate(&e0));
    HIPCHK(ctx, hipEventCreate(&e1));
    hipError_t e = hipMemcpyAsync(ctx->d_obj_alt.p, ctx->d_obj.p, n, hipMemcpyDeviceToDevice, ctx->stream);
    if (e == hipSuccess) e = hipEventRecord(e0, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(ctx->d_obj_alt.p, ctx->d_obj.p, n, hipMemcpyDeviceToDevice, ctx->stream);
    if (e == hipSuccess) e = hipEventRecord(e1, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    HIPCHK(ctx, e);
    us2[1] = ms * 1000.0f;
    return RXR_OK;
}

// tests / tools: the object-space pools as the context holds them, whole: totals[2] = vertices, triangles; the arrays (each may be
// NULL) take min(total, capacity) items of vertices [4], uvs [2], indices [3], normals [3]
int rxr_debug_object_pools(rxr_ctx *ctx, uint64_t *totals, float *vertices, float *uvs, uint32_t *indices, float *normals, uint64_t capacity_vertices,
                           uint64_t capacity_triangles) {
    if (!ctx || ctx->group || !totals) return RXR_ERR_INVALID;
    if (!ctx->meshes_valid) return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_debug_object_pools: no valid registration");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc = rxr_quiesce(ctx);
    if (rc != RXR_OK) return rc;
    const ProjectParams &PP = ctx->PP;
    totals[0] = ctx->meshes.empty() ? 0 : PP.n_verts_in;
    totals[1] = ctx->meshes.empty() ? 0 : PP.n_tris_in;
    const size_t nv = (size_t)std::min<uint64_t>(totals[0], capacity_vertices), nt = (size_t)std::min<uint64_t>(totals[1], capacity_triangles);
    if (vertices && nv) HIPCHK(ctx, hipMemcpy(vertices, PP.obj_verts, nv * 16, hipMemcpyDeviceToHost));
    if (uvs && nv) HIPCHK(ctx, hipMemcpy(uvs, PP.obj_uvs, nv * 8, hipMemcpyDeviceToHost));
    if (normals && nv) HIPCHK(ctx, hipMemcpy(normals, PP.obj_normals, nv * 12, hipMemcpyDeviceToHost));
    if (indices && nt) HIPCHK(ctx, hipMemcpy(indices, PP.obj_idx, nt * 12, hipMemcpyDeviceToHost));
    return RXR_OK;
}

// tests: the layout arithmetic of rxr_resize_meshes (rxr_mesh_resize.h) as the library compiled it
uint32_t rxr_debug_resize_bases(const uint32_t *counts, uint32_t n, uint32_t *bases, uint64_t *totals) {
    return (uint32_t)rxr_resize_bases(counts, n, bases, totals);
}

int rxr_mesh_bounds(rxr_ctx *ctx, uint32_t mesh_index, float lo[3], float hi[3]) {
    if (!ctx) return RXR_ERR_INVALID;
    if (ctx->group) return rxr_as_member0(ctx, [&](rxr_ctx *m) { return rxr_mesh_bounds(m, mesh_index, lo, hi); });
    if (!lo || !hi) return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_mesh_bounds: NULL output");
    if (!ctx->meshes_valid || mesh_index >= ctx->meshes.size()) return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_mesh_bounds: no such mesh");
    memcpy(lo, ctx->meshes[mesh_index].aabb_lo, 12);
    memcpy(hi, ctx->meshes[mesh_index].aabb_hi, 12);
    return RXR_OK;
}

// Not part of include/rxr.h: device memory of the context for a host layer that links no HIP runtime of its own (the C++ mirror's
// Scene::rebuild_terrain_meshes builds chunk meshes into it and hands them to rxr_update_meshes_to).  At least `bytes`, 256-byte
// aligned, owned by the context and valid until the next call asks for more (which waits for queued work first) or rxr_destroy; NULL
// on failure or on a multi-device handle.
void *rxr_mirror_scratch(rxr_ctx *ctx, size_t bytes) {
    if (!ctx || ctx->group) return nullptr;
    if (hipSetDevice(ctx->device) != hipSuccess) return nullptr;
    if (rxr_ensure(ctx, ctx->d_mirror_scratch, bytes ? bytes : 16) != RXR_OK) return nullptr;
    return ctx->d_mirror_scratch.p;
}

// ... and a few words of it read back: waits for what the context's stream has queued, then copies.  RXR_OK or a negative rxr_status.
int rxr_mirror_read(rxr_ctx *ctx, void *host, const void *dev, size_t bytes) {
    if (!ctx || ctx->group || !host || !dev) return RXR_ERR_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return RXR_OK;
}

// ---- the 2D half of the device-side projection (row N1): Batch2D::project's inputs, registered once ---------------------------
int rxr_set_meshes2d(rxr_ctx *ctx, const rxr_mesh2d *meshes, uint32_t n_meshes) {
    if (!ctx) return RXR_ERR_INVALID;
    if (n_meshes && !meshes) return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_set_meshes2d: NULL mesh array");
    if (ctx->group) return rxr_group_set_meshes2d(ctx, meshes, n_meshes);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    {
        int qrc = rxr_quiesce(ctx);
        if (qrc != RXR_OK) return qrc;
    }
    // A call that fails half way must leave an EMPTY registration, never a partial list beside the previous call's device data
    // (round-3 advisor finding: a later frame with use_meshes bit 1 would have built batch headers from the partial list while the
    // projection kernels still named the old mesh indices): everything that describes the registration is reset before the first check.
    ctx->meshes2d.clear();
    ctx->meshes2d_prims = 0;
    ctx->meshes2d_tris = 0;
    ctx->PP2 = Project2DParams{};
    ctx->has_frame = false;
    struct EmptyOnFailure {
        rxr_ctx *c;
        bool ok = false;
        ~EmptyOnFailure() {
            if (!ok) {
                c->meshes2d.clear();
                c->meshes2d_prims = c->meshes2d_tris = 0;
                c->PP2 = Project2DParams{};
            }
        }
    } registration{ctx};
    size_t vin = 0, prims = 0, tris = 0;
    for (uint32_t i = 0; i < n_meshes; ++i) {
        const rxr_mesh2d &m = meshes[i];
        if (m.n_vertices && (!m.vertices || !m.uvs)) return rxr_fail(ctx, RXR_ERR_INVALID, "mesh2d: NULL vertex arrays");
        if (m.n_triangles && !m.indices) return rxr_fail(ctx, RXR_ERR_INVALID, "mesh2d: NULL indices");
        if (m.mode > RXR_MODE_LINE_LOOP) return rxr_fail(ctx, RXR_ERR_INVALID, "mesh2d: bad mode");
        if (m.mode == RXR_MODE_TRIANGLES || m.mode == RXR_MODE_LINES)
            for (size_t t = 0; t < (size_t)m.n_triangles * 3u; ++t) {
                if (m.mode == RXR_MODE_LINES && (t % 3u) == 2u) continue;  // only .0/.1 are read, :902
                if (m.indices[t] >= m.n_vertices) return rxr_fail(ctx, RXR_ERR_INVALID, "mesh2d: vertex index out of range");
            }
        rxr_ctx::HostMesh2D h{};
        h.vin_base = (uint32_t)vin;
        h.n_verts = m.n_vertices;
        h.n_tris = m.n_triangles;
        switch (m.mode) {
            case RXR_MODE_TRIANGLES: h.n_prims = m.n_triangles; tris += m.n_triangles; break;
            case RXR_MODE_LINES: h.n_prims = m.n_triangles; break;
            case RXR_MODE_LINE_STRIP: h.n_prims = m.n_vertices ? m.n_vertices - 1 : 0; break;
            default: h.n_prims = m.n_vertices; break;
        }
        h.prim_base = (uint32_t)prims;
        h.mode = m.mode;
        h.repeat_mode = m.repeat_mode;
        h.receives_light = m.receives_light;
        h.source = m.source;
        h.shader = m.shader;
        h.chunk = m.chunk;
        ctx->meshes2d.push_back(h);
        vin += m.n_vertices;
        prims += h.n_prims;
    }
    if (vin >= (1ull << 31) || prims >= (1ull << 30)) return rxr_fail(ctx, RXR_ERR_INVALID, "2D meshes too large");
    BlobCursor take;
    const size_t off_v = take(vin * 8), off_uv = take(vin * 8), off_src = take(prims * sizeof(Prim2DSrc)), off_pv = take((n_meshes + 1) * 4),
                 off_dm = take((size_t)n_meshes * sizeof(DevMesh2D));
    const size_t total = take.o;
    int rc;
    if ((rc = rxr_ensure_stage(ctx, total)) != RXR_OK) return rc;
    if ((rc = rxr_ensure(ctx, ctx->d_obj2d, total)) != RXR_OK) return rc;
    uint8_t *st = (uint8_t *)ctx->h_stage;
    uint32_t *pv = (uint32_t *)(st + off_pv);
    DevMesh2D *dm = (DevMesh2D *)(st + off_dm);
    Prim2DSrc *src = (Prim2DSrc *)(st + off_src);
    for (uint32_t i = 0; i < n_meshes; ++i) {
        const rxr_mesh2d &m = meshes[i];
        const rxr_ctx::HostMesh2D &h = ctx->meshes2d[i];
        pv[i] = h.vin_base;
        const uint8_t white[4] = {255, 255, 255, 255};
        dm[i] = DevMesh2D{h.vin_base, h.n_verts, h.mode, pack_px(m.source.kind == RXR_SOURCE_PIXEL ? m.source.pixel : white)};  // :911-915
        if (m.n_vertices) {
            memcpy(st + off_v + (size_t)h.vin_base * 8, m.vertices, (size_t)m.n_vertices * 8);
            memcpy(st + off_uv + (size_t)h.vin_base * 8, m.uvs, (size_t)m.n_vertices * 8);
        }
        Prim2DSrc *q = src + h.prim_base;
        if (m.mode == RXR_MODE_TRIANGLES)
            for (uint32_t t = 0; t < m.n_triangles; ++t) q[t] = Prim2DSrc{i, m.indices[3 * (size_t)t], m.indices[3 * (size_t)t + 1], m.indices[3 * (size_t)t + 2]};
        else if (m.mode == RXR_MODE_LINES)
            for (uint32_t t = 0; t < m.n_triangles; ++t) q[t] = Prim2DSrc{i, m.indices[3 * (size_t)t], m.indices[3 * (size_t)t + 1], 0u};
        else if (m.mode == RXR_MODE_LINE_STRIP)
            for (uint32_t k = 0; k + 1 < m.n_vertices; ++k) q[k] = Prim2DSrc{i, k, k + 1u, 0u};
        else
            for (uint32_t k = 0; k < m.n_vertices; ++k) q[k] = Prim2DSrc{i, k, (k + 1u) % m.n_vertices, 0u};
    }
    pv[n_meshes] = (uint32_t)vin;
    HIPCHK(ctx, hipMemcpyAsync(ctx->d_obj2d.p, st, total, hipMemcpyHostToDevice, ctx->stream));
    take.o = 0;
    const size_t m_bbox = take((size_t)n_meshes * sizeof(DevBBox)), m_box = take(16);
    if ((rc = rxr_ensure(ctx, ctx->d_proj2d_misc, take.o)) != RXR_OK) return rc;
    Project2DParams &PP = ctx->PP2;
    memset(&PP, 0, sizeof(PP));
    PP.n_meshes = n_meshes;
    PP.n_verts = (uint32_t)vin;
    PP.n_prims = (uint32_t)prims;
    uint8_t *d = (uint8_t *)ctx->d_obj2d.p, *mm = (uint8_t *)ctx->d_proj2d_misc.p;
    PP.meshes = (const DevMesh2D *)(d + off_dm);
    PP.vin_prefix = (const uint32_t *)(d + off_pv);
    PP.obj_verts = (const float2 *)(d + off_v);
    PP.obj_uvs = (const float2 *)(d + off_uv);
    PP.src = (const Prim2DSrc *)(d + off_src);
    PP.bbox = (DevBBox *)(mm + m_bbox);
    PP.d2_box = (uint32_t *)(mm + m_box);
    PP.bad_line = ctx->d_host_status + HS_BAD_LINE2D;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->meshes2d_prims = prims;
    ctx->meshes2d_tris = tris;
    registration.ok = true;
    return RXR_OK;
}

int rxr_set_projection2d(rxr_ctx *ctx, const float *mat3) {
    if (!ctx) return RXR_ERR_INVALID;
    if (ctx->group) return rxr_group_set_projection2d(ctx, mat3);
    ctx->has_matrix2d = mat3 != nullptr;
    if (mat3) memcpy(ctx->matrix2d, mat3, sizeof(ctx->matrix2d));
    return RXR_OK;
}

int rxr_read_projected_mesh(rxr_ctx *ctx, uint32_t index, uint32_t counts[2], float *projected_vertices, float *clipped_uvs,
                            float *clipped_normals, uint32_t *clipped_indices, rxr_edges *edges, float bounding_box[5],
                            uint32_t capacity_vertices, uint32_t capacity_triangles) {
    if (!ctx || !counts) return RXR_ERR_INVALID;
    if (ctx->group)
        return rxr_read_projected_mesh(rxr_member(ctx, 0), index, counts, projected_vertices, clipped_uvs, clipped_normals, clipped_indices, edges,
                                       bounding_box, capacity_vertices, capacity_triangles);
    if (index >= ctx->meshes.size()) return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_read_projected_mesh: no such mesh");
    int rc = rxr_synchronize(ctx);
    if (rc != RXR_OK) return rc;
    const DevMesh &M = ctx->meshes[index].dev;
    const ProjectParams &PP = ctx->PP;
    // appended counts of this mesh = prefix(end) - prefix(start)
    auto prefix_at = [&](uint32_t i, AppendCount &out) -> int {
        AppendCount a = 0, b = 0;
        HIPCHK(ctx, hipMemcpy(&a, PP.append + i, 8, hipMemcpyDeviceToHost));
        HIPCHK(ctx, hipMemcpy(&b, PP.chunk_base + i / RXR_PROJ_SCAN_CHUNK, 8, hipMemcpyDeviceToHost));
        out = a + b;
        return RXR_OK;
    };
    AppendCount p0 = 0, p1 = 0;
    DevMesh frame_mesh{};
    HIPCHK(ctx, hipMemcpy(&frame_mesh, (uint8_t *)ctx->d_proj_misc.p + ctx->pp_off_meshes + (size_t)index * sizeof(DevMesh), sizeof(DevMesh), hipMemcpyDeviceToHost));
    uint32_t nv = 0, nt = 0;
    if (!frame_mesh.rejected) {
        if ((rc = prefix_at(M.tin_base, p0)) != RXR_OK || (rc = prefix_at(M.tin_base + M.n_tris, p1)) != RXR_OK) return rc;
        AppendCount tot = p1 - p0;
        nv = M.n_verts + (uint32_t)(tot & 0xFFFFFFFFull);
        nt = M.n_tris + (uint32_t)(tot >> 32);
    }
    counts[0] = nv;
    counts[1] = nt;
    if (nv > capacity_vertices || nt > capacity_triangles) return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_read_projected_mesh: capacity too small");
    if (projected_vertices && nv) HIPCHK(ctx, hipMemcpy(projected_vertices, PP.pv + M.vout_base, (size_t)nv * 16, hipMemcpyDeviceToHost));
    if (clipped_uvs && nv) HIPCHK(ctx, hipMemcpy(clipped_uvs, PP.uv + M.vout_base, (size_t)nv * 8, hipMemcpyDeviceToHost));
    if (clipped_normals && nv) HIPCHK(ctx, hipMemcpy(clipped_normals, PP.nrm + 3 * (size_t)M.vout_base, (size_t)nv * 12, hipMemcpyDeviceToHost));
    if (clipped_indices && nt) HIPCHK(ctx, hipMemcpy(clipped_indices, PP.idx + 3 * (size_t)M.tout_base, (size_t)nt * 12, hipMemcpyDeviceToHost));
    if (edges && nt) {
        if (PP.edges_in_setup) {  // (the frame's set-up built its records itself: the pool is filled for this call)
            HIPCHK(ctx, hipSetDevice(ctx->device));
            rxr_launch_proj_edges(&PP, ctx->stream);
            HIPCHK(ctx, hipGetLastError());
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        }
        HIPCHK(ctx, hipMemcpy(edges, PP.edges + M.tout_base, (size_t)nt * sizeof(rxr_edges), hipMemcpyDeviceToHost));
    }
    if (bounding_box) {
        DevBBox bb{};
        HIPCHK(ctx, hipMemcpy(&bb, PP.bbox + index, sizeof(bb), hipMemcpyDeviceToHost));
        auto dec = [](uint32_t e) {
            uint32_t u = (e & 0x80000000u) ? (e ^ 0x80000000u) : ~e;
            float f;
            memcpy(&f, &u, 4);
            return f;
        };
        bounding_box[0] = frame_mesh.rejected ? 0.0f : 1.0f;
        bounding_box[1] = dec(bb.min_x);
        bounding_box[2] = dec(bb.min_y);
        bounding_box[3] = dec(bb.max_x) - dec(bb.min_x);
        bounding_box[4] = dec(bb.max_y) - dec(bb.min_y);
    }
    return RXR_OK;
}

// ---- Rusteria programs: NodeOp tree (include/rxr.h) -> jump code (rxr_device.h) ------------------
namespace {

struct Flattener {
    std::vector<uint32_t> code;
    std::vector<std::pair<size_t, uint32_t>> call_patches;  // (position of the target word, function index)
    std::vector<size_t> return_patches;                     // positions to fill with the current function's ENDFN address
    uint32_t n_functions = 0;
    bool writes_opacity = false, writes_emissive = false;
    std::string err;
    int status = RXR_OK;

    bool bad(int st, const std::string &m) {
        if (status == RXR_OK) {
            status = st;
            err = m;
        }
        return false;
    }

    // one block of the serialised tree; for_depth > 0 inside a For
    bool block(const uint32_t *w, size_t n, int for_depth, int depth) {
        if (depth > 64) return bad(RXR_ERR_INVALID, "program nested too deeply");
        size_t i = 0;
        auto need = [&](size_t k) { return i + k <= n; };
        while (i < n) {
            const uint32_t op = w[i++];
            if (op >= RXR_NODE_COUNT) return bad(RXR_ERR_INVALID, "unknown NodeOp opcode");
            switch (op) {
                case RXR_NODE_LOAD_GLOBAL:
                case RXR_NODE_STORE_GLOBAL:
                case RXR_NODE_LOAD_LOCAL:
                case RXR_NODE_STORE_LOCAL:
                    if (!need(1)) return bad(RXR_ERR_INVALID, "truncated program");
                    code.push_back(op);
                    code.push_back(w[i++]);
                    break;
                case RXR_NODE_GET_COMPONENTS:
                case RXR_NODE_SET_COMPONENTS: {
                    if (!need(1)) return bad(RXR_ERR_INVALID, "truncated program");
                    uint32_t k = w[i++];
                    if (!need(k)) return bad(RXR_ERR_INVALID, "truncated program");
                    if (k > 12) return bad(RXR_ERR_UNSUPPORTED, "swizzle with more than 12 components");
                    uint32_t enc = k;
                    for (uint32_t j = 0; j < k; ++j) enc |= (w[i + j] > 2u ? 3u : w[i + j]) << (4u + 2u * j);
                    i += k;
                    code.push_back(op == RXR_NODE_GET_COMPONENTS ? (uint32_t)VM_GETC : (uint32_t)VM_SETC);
                    code.push_back(enc);
                    break;
                }
                case RXR_NODE_IF: {
                    if (!need(3)) return bad(RXR_ERR_INVALID, "truncated program");
                    const uint32_t tl = w[i], he = w[i + 1], el = w[i + 2];
                    i += 3;
                    if (!need((size_t)tl + el)) return bad(RXR_ERR_INVALID, "truncated program");
                    code.push_back(VM_JZ);
                    const size_t jz = code.size();
                    code.push_back(0);
                    if (!block(w + i, tl, for_depth, depth + 1)) return false;
                    i += tl;
                    if (he) {
                        code.push_back(VM_JMP);
                        const size_t jend = code.size();
                        code.push_back(0);
                        code[jz] = (uint32_t)code.size();
                        if (!block(w + i, el, for_depth, depth + 1)) return false;
                        code[jend] = (uint32_t)code.size();
                    } else {
                        code[jz] = (uint32_t)code.size();
                    }
                    i += el;
                    break;
                }
                case RXR_NODE_FOR: {  // execution.rs:251-278
                    if (!need(4)) return bad(RXR_ERR_INVALID, "truncated program");
                    const uint32_t l[4] = {w[i], w[i + 1], w[i + 2], w[i + 3]};
                    i += 4;
                    if (!need((size_t)l[0] + l[1] + l[2] + l[3])) return bad(RXR_ERR_INVALID, "truncated program");
                    const uint32_t *init = w + i, *cond = init + l[0], *incr = cond + l[1], *body = incr + l[2];
                    i += (size_t)l[0] + l[1] + l[2] + l[3];
                    code.push_back(VM_FOR_ENTER);
                    if (!block(init, l[0], for_depth + 1, depth + 1)) return false;
                    code.push_back(VM_FOR_TRUNC);
                    const uint32_t top = (uint32_t)code.size();
                    if (!block(cond, l[1], for_depth + 1, depth + 1)) return false;
                    code.push_back(VM_FOR_COND);
                    const size_t jexit = code.size();
                    code.push_back(0);
                    code.push_back(VM_FOR_TRUNC);
                    if (!block(body, l[3], for_depth + 1, depth + 1)) return false;
                    code.push_back(VM_FOR_TRUNC);
                    if (!block(incr, l[2], for_depth + 1, depth + 1)) return false;
                    code.push_back(VM_FOR_TRUNC);
                    code.push_back(VM_JMP);
                    code.push_back(top);
                    code[jexit] = (uint32_t)code.size();
                    code.push_back(VM_FOR_EXIT);
                    break;
                }
                case RXR_NODE_PUSH:
                    if (!need(3)) return bad(RXR_ERR_INVALID, "truncated program");
                    // peephole: a constant followed by a component-wise binary operation becomes one instruction
                    // ("tos = tos op c"), the commonest pair in compiled expressions
                    if (i + 3 < n) {
                        const uint32_t nx = w[i + 3];
                        int fused = -1;
                        switch (nx) {
                            case RXR_NODE_ADD: fused = VM_BINC_ADD; break;
                            case RXR_NODE_SUB: fused = VM_BINC_SUB; break;
                            case RXR_NODE_MUL: fused = VM_BINC_MUL; break;
                            case RXR_NODE_DIV: fused = VM_BINC_DIV; break;
                            case RXR_NODE_MIN: fused = VM_BINC_MIN; break;
                            case RXR_NODE_MAX: fused = VM_BINC_MAX; break;
                            case RXR_NODE_MOD: fused = VM_BINC_MOD; break;
                            case RXR_NODE_LT: fused = VM_BINC_LT; break;
                            case RXR_NODE_LE: fused = VM_BINC_LE; break;
                            case RXR_NODE_GT: fused = VM_BINC_GT; break;
                            case RXR_NODE_GE: fused = VM_BINC_GE; break;
                            case RXR_NODE_EQ: fused = VM_BINC_EQ; break;
                            case RXR_NODE_NE: fused = VM_BINC_NE; break;
                            default: break;
                        }
                        if (fused >= 0) {
                            code.push_back((uint32_t)VM_BINC | ((uint32_t)fused << 8));
                            code.push_back(w[i]);
                            code.push_back(w[i + 1]);
                            code.push_back(w[i + 2]);
                            i += 4;
                            break;
                        }
                    }
                    code.push_back(op);
                    code.push_back(w[i]);
                    code.push_back(w[i + 1]);
                    code.push_back(w[i + 2]);
                    i += 3;
                    break;
                case RXR_NODE_FUNCTION_CALL: {
                    if (!need(3)) return bad(RXR_ERR_INVALID, "truncated program");
                    const uint32_t arity = w[i], total = w[i + 1], index = w[i + 2];
                    i += 3;
                    if (index >= n_functions) {  // program.user_functions[index] panics when reached
                        code.push_back(VM_FAULT);
                        code.push_back(VMF_BAD_CALL);
                        break;
                    }
                    if (total > RXR_VM_LOCALS) return bad(RXR_ERR_UNSUPPORTED, "function with more locals than the device VM holds");
                    code.push_back(VM_CALL);
                    code.push_back(arity);
                    code.push_back(total);
                    call_patches.emplace_back(code.size(), index);
                    code.push_back(0);
                    break;
                }
                case RXR_NODE_RETURN:
                    // the reference's For keeps iterating after a Return unwound its body (execution.rs:258-277):
                    // it pops the ENCLOSING frame's values as loop conditions
                    if (for_depth > 0) return bad(RXR_ERR_UNSUPPORTED, "Return inside For (the reference unwinds it incorrectly)");
                    code.push_back(VM_RETURN);
                    return_patches.push_back(code.size());
                    code.push_back(0);
                    break;
                case RXR_NODE_ALLOC:
                case RXR_NODE_ITERATE:
                case RXR_NODE_SAVE:
                    return bad(RXR_ERR_UNSUPPORTED, "Alloc / Iterate / Save (texture baking) are not part of per-fragment shading");
                case RXR_NODE_SET_EMISSIVE:
                    // `emissive` is never reset by the raster loops: every opaque 3D fragment adds whatever the LAST SetEmissive
                    // of its tile left (rasterizer.rs:1323, :1394).  Whether a frame can run such a program without that leak
                    // is decided per frame (rxr_upload_frame: every visible opaque 3D batch must assign it itself)
                    writes_emissive = true;
                    code.push_back(op);
                    break;
                case RXR_NODE_SET_OPACITY:
                    writes_opacity = true;
                    code.push_back(op);
                    break;
                default: code.push_back(op); break;
            }
        }
        return true;
    }
};

// Purity check (definite assignment).  The reference keeps ONE Execution per tile: `shade`'s locals are resized, not
// cleared (execution.rs:747), and globals are never reset, so a read that the same invocation has not written before
// sees the previous fragment's value.  A program is accepted only if every LoadLocal of `shade` and every LoadGlobal
// anywhere is definitely preceded by a store in the same invocation: stores count from their position onwards within a
// block, an If contributes what BOTH branches store, a For what its init and its first condition evaluation store;
// called functions get fresh zeroed locals (execution.rs:188) -- their global reads are checked against what is
// assigned at the call, their global stores are not credited.
struct Assigned {
    uint64_t locals = 0;
    uint32_t globals = 0;
    uint32_t fields = 0;  // PF_*: Execution fields this invocation has written so far
};


struct PurityCheck {
    const rxr_program &p;
    bool ok = true;
    uint32_t reads_unassigned = 0;  // PF_* read before this invocation wrote them
    uint32_t writes = 0;            // PF_* written anywhere in the program
    uint32_t exit_fields = ~0u;     // PF_* assigned at EVERY `Return` of shade itself (a Return leaves before the code behind it)
    std::vector<char> visiting;

    explicit PurityCheck(const rxr_program &prog) : p(prog), visiting(prog.n_functions, 0) {}

    // walks one block; `in_shade`: LoadLocal / StoreLocal refer to shade's (leaky) locals
    Assigned block(const uint32_t *w, size_t n, Assigned a, bool in_shade, int depth) {
        size_t i = 0;
        while (i < n && ok && depth < 64) {
            const uint32_t op = w[i++];
            switch (op) {
                case RXR_NODE_LOAD_LOCAL:
                    if (in_shade && (w[i] >= 64 || !((a.locals >> w[i]) & 1ull))) ok = false;
                    i += 1;
                    break;
                case RXR_NODE_STORE_LOCAL:
                    if (in_shade && w[i] < 64) a.locals |= 1ull << w[i];
                    i += 1;
                    break;
                case RXR_NODE_LOAD_GLOBAL:
                    if (w[i] >= 32 || !((a.globals >> w[i]) & 1u)) ok = false;
                    i += 1;
                    break;
                case RXR_NODE_STORE_GLOBAL:
                    if (w[i] < 32) a.globals |= 1u << w[i];  // (what a callee stores is not credited to its caller, see FunctionCall)
                    i += 1;
                    break;
                case RXR_NODE_UV: reads_unassigned |= PF_UV & ~a.fields; break;
                case RXR_NODE_ROUGHNESS: reads_unassigned |= PF_ROUGHNESS & ~a.fields; break;
                case RXR_NODE_METALLIC: reads_unassigned |= PF_METALLIC & ~a.fields; break;
                case RXR_NODE_OPACITY: reads_unassigned |= PF_OPACITY & ~a.fields; break;
                case RXR_NODE_BUMP: reads_unassigned |= PF_BUMP & ~a.fields; break;
                case RXR_NODE_NORMAL: reads_unassigned |= PF_NORMAL & ~a.fields; break;
                case RXR_NODE_HITPOINT: reads_unassigned |= PF_HITPOINT; break;
                case RXR_NODE_EMISSIVE: reads_unassigned |= PF_EMISSIVE & ~a.fields; break;
                case RXR_NODE_SET_EMISSIVE: a.fields |= PF_EMISSIVE; writes |= PF_EMISSIVE; break;
                case RXR_NODE_RETURN:
                    if (in_shade) exit_fields &= a.fields;
                    break;
                case RXR_NODE_SET_UV: a.fields |= PF_UV; writes |= PF_UV; break;
                case RXR_NODE_SET_ROUGHNESS: a.fields |= PF_ROUGHNESS; writes |= PF_ROUGHNESS; break;
                case RXR_NODE_SET_METALLIC: a.fields |= PF_METALLIC; writes |= PF_METALLIC; break;
                case RXR_NODE_SET_OPACITY: a.fields |= PF_OPACITY; writes |= PF_OPACITY; break;
                case RXR_NODE_SET_BUMP: a.fields |= PF_BUMP; writes |= PF_BUMP; break;
                case RXR_NODE_SET_NORMAL: a.fields |= PF_NORMAL; writes |= PF_NORMAL; break;
                case RXR_NODE_GET_COMPONENTS:
                case RXR_NODE_SET_COMPONENTS: i += 1 + w[i]; break;
                case RXR_NODE_PUSH: i += 3; break;
                case RXR_NODE_IF: {
                    const uint32_t tl = w[i], he = w[i + 1], el = w[i + 2];
                    i += 3;
                    Assigned t = block(w + i, tl, a, in_shade, depth + 1);
                    Assigned e = he ? block(w + i + tl, el, a, in_shade, depth + 1) : a;
                    a.locals = t.locals & e.locals;
                    a.globals = t.globals & e.globals;
                    a.fields = t.fields & e.fields;
                    i += (size_t)tl + el;
                    break;
                }
                case RXR_NODE_FOR: {
                    const uint32_t l0 = w[i], l1 = w[i + 1], l2 = w[i + 2], l3 = w[i + 3];
                    i += 4;
                    const uint32_t *init = w + i, *cond = init + l0, *incr = cond + l1, *body = incr + l2;
                    a = block(init, l0, a, in_shade, depth + 1);
                    a = block(cond, l1, a, in_shade, depth + 1);       // the condition runs at least once
                    Assigned b = block(body, l3, a, in_shade, depth + 1);
                    (void)block(incr, l2, b, in_shade, depth + 1);
                    i += (size_t)l0 + l1 + l2 + l3;
                    break;
                }
                case RXR_NODE_FUNCTION_CALL: {
                    const uint32_t index = w[i + 2];
                    i += 3;
                    if (index < p.n_functions && !visiting[index]) {
                        visiting[index] = 1;
                        Assigned callee;
                        callee.globals = a.globals;
                        callee.fields = a.fields;
                        (void)block(p.functions[index].words, p.functions[index].n_words, callee, false, depth + 1);
                        visiting[index] = 0;
                    }
                    break;
                }
                default: break;
            }
        }
        return a;
    }
};

// `assigned_at_exit`: the PF_* fields that `shade` has written itself on every path to its end (its last instruction or a Return)
bool program_is_pure(const rxr_program &p, uint32_t &reads_unassigned, uint32_t &writes, uint32_t &assigned_at_exit) {
    reads_unassigned = writes = assigned_at_exit = 0;
    if (p.shade_index < 0 || (uint32_t)p.shade_index >= p.n_functions) return true;
    PurityCheck c(p);
    c.visiting[p.shade_index] = 1;
    const Assigned end = c.block(p.functions[p.shade_index].words, p.functions[p.shade_index].n_words, Assigned{}, true, 0);
    reads_unassigned = c.reads_unassigned;
    writes = c.writes;
    assigned_at_exit = end.fields & c.exit_fields;
    return c.ok;
}

}  // namespace

namespace {

// validates every program of the set and flattens them into one code stream; no device involved.
// Returns RXR_OK or the status + message rxr_set_shaders / rxr_check_shaders report.
int flatten_programs(const rxr_shader_set *set, std::vector<uint32_t> &code, std::vector<DevProgram> &progs, std::vector<uint32_t> &field_reads,
                     std::string &err, std::vector<uint32_t> *field_writes_out = nullptr) {
    auto bad = [&](int st, const std::string &m) {
        err = m;
        return st;
    };
    if (set->n_programs && !set->programs) return bad(RXR_ERR_INVALID, "NULL program array");
    Flattener fl;
    uint32_t field_writes = 0;
    for (uint32_t pi = 0; pi < set->n_programs; ++pi) {
        const rxr_program &p = set->programs[pi];
        if (p.n_functions && !p.functions) return bad(RXR_ERR_INVALID, "NULL function array");
        for (uint32_t k = 0; k < p.n_functions; ++k)
            if (p.functions[k].n_words && !p.functions[k].words) return bad(RXR_ERR_INVALID, "NULL function body");
        DevProgram d{};
        d.shade_entry = 0xFFFFFFFFu;
        d.shade_locals = p.shade_locals;
        d.n_globals = p.n_globals;
        uint32_t ru = 0, wr = 0, at_exit = 0;
        if (p.shade_index >= 0) {
            if ((uint32_t)p.shade_index >= p.n_functions)  // program.user_functions[index] would panic on the first fragment
                return bad(RXR_ERR_INVALID, "shade_index out of range");
            if (p.n_globals > RXR_VM_GLOBALS) return bad(RXR_ERR_UNSUPPORTED, "more globals than the device VM holds");
            if (p.shade_locals > RXR_VM_LOCALS) return bad(RXR_ERR_UNSUPPORTED, "more locals than the device VM holds");
            // structural check first (lengths), so that the purity walk below cannot run off the arrays
            fl.n_functions = p.n_functions;
            fl.writes_opacity = fl.writes_emissive = false;
            fl.call_patches.clear();
            std::vector<uint32_t> entries(p.n_functions);
            for (uint32_t k = 0; k < p.n_functions; ++k) {
                entries[k] = (uint32_t)fl.code.size();
                fl.return_patches.clear();
                if (!fl.block(p.functions[k].words, p.functions[k].n_words, 0, 0)) return bad(fl.status, fl.err);
                const uint32_t endfn = (uint32_t)fl.code.size();
                fl.code.push_back(VM_ENDFN);
                for (size_t pos : fl.return_patches) fl.code[pos] = endfn;
            }
            for (auto &cp : fl.call_patches) fl.code[cp.first] = entries[cp.second];
            if (!program_is_pure(p, ru, wr, at_exit))
                return bad(RXR_ERR_UNSUPPORTED, "a local of `shade` or a global is read before this invocation wrote it (the reference would read the previous fragment's value)");
            field_writes |= wr;
            d.shade_entry = entries[p.shade_index];
            d.flags = (fl.writes_opacity ? PG_WRITES_OPACITY : 0u) | (fl.writes_emissive ? PG_WRITES_EMISSIVE : 0u) |
                      ((at_exit & PF_EMISSIVE) ? PG_ASSIGNS_EMISSIVE : 0u);
        }
        field_reads.push_back(ru);
        if (field_writes_out) field_writes_out->push_back(wr);   // PF_* this program writes anywhere (the bake's rule, rxr_bake_refusal)
        progs.push_back(d);
    }
    // uv.z, roughness.yz, metallic.yz, opacity.yz and bump are never assigned by the raster loops: once ANY program of the
    // set writes such a field, a read that its own invocation has not preceded by a write would see an earlier fragment's lanes
    for (uint32_t m : field_reads)
        if (m & field_writes & (PF_UV | PF_ROUGHNESS | PF_METALLIC | PF_OPACITY | PF_BUMP | PF_EMISSIVE))
            return bad(RXR_ERR_UNSUPPORTED, "a program reads uv / roughness / metallic / opacity / bump / emissive before writing it while a program of the set writes that field (lanes the raster loops never reset would leak between fragments)");
    for (int k = 0; k < 4; ++k) fl.code.push_back(VM_ENDFN);  // the interpreter reads one word ahead of every opcode
    if (fl.code.size() >= (1ull << 31)) return bad(RXR_ERR_INVALID, "programs too large");
    code = std::move(fl.code);
    return RXR_OK;
}

}  // namespace

// Static stack depths.  For a program without calls and without PaletteIndex (the one opcode that pushes or not depending on
// data) the depth of the value stack is a function of the program counter alone.  This pass proves it by abstract
// interpretation of the flat code (state = depth + the For-loop bases; every join must agree; every instruction must have its
// operands and its room) and writes the depth BEFORE each instruction into bits 16..23 of its opcode word.  When that works
// for every program of a set the interpreter runs with a wave-uniform stack pointer read from the code stream (rxr_vm.h,
// kernel k_raster_vm_s): the per-lane stack bookkeeping becomes scalar.  Returns false when any program stays dynamic.
static bool tag_static_depths(std::vector<uint32_t> &code, const std::vector<DevProgram> &progs) {
    struct State {
        int depth;
        std::vector<int> loops;
        bool operator==(const State &o) const { return depth == o.depth && loops == o.loops; }
    };
    std::vector<int> seen(code.size(), -1);          // index into states, per pc
    std::vector<State> states;
    std::vector<std::pair<uint32_t, State>> work;
    auto length_of = [](uint32_t op) -> uint32_t {
        switch (op) {
            case RXR_NODE_LOAD_GLOBAL: case RXR_NODE_STORE_GLOBAL: case RXR_NODE_LOAD_LOCAL: case RXR_NODE_STORE_LOCAL:
            case VM_GETC: case VM_SETC: case VM_JMP: case VM_JZ: case VM_FOR_COND: case VM_RETURN: case VM_FAULT: return 2;
            case RXR_NODE_PUSH: case VM_BINC: case VM_CALL: return 4;
            default: return 1;
        }
    };
    for (const DevProgram &p : progs) {
        if (p.shade_entry == 0xFFFFFFFFu) continue;
        work.clear();
        work.push_back({p.shade_entry, State{0, {}}});
        while (!work.empty()) {
            auto [pc, st] = work.back();
            work.pop_back();
            for (;;) {
                if (pc >= code.size()) return false;
                const uint32_t w = code[pc], op = w & 0xFFu;
                if (op == VM_ENDFN) break;  // end of `shade`: the stack is not looked at any more
                if (seen[pc] >= 0) {
                    if (!(states[(size_t)seen[pc]] == st)) return false;  // two paths arrive with different stacks
                    break;
                }
                seen[pc] = (int)states.size();
                states.push_back(st);
                if (st.depth < 0 || st.depth > 255) return false;
                const uint32_t len = length_of(op);
                if (pc + len > code.size()) return false;
                int need = 0, delta = 0;
                bool room = false;
                switch (op) {
                    case RXR_NODE_LOAD_GLOBAL: case RXR_NODE_LOAD_LOCAL: case RXR_NODE_PUSH:
                    case RXR_NODE_UV: case RXR_NODE_NORMAL: case RXR_NODE_HITPOINT: case RXR_NODE_TIME: case RXR_NODE_COLOR:
                    case RXR_NODE_ROUGHNESS: case RXR_NODE_METALLIC: case RXR_NODE_EMISSIVE: case RXR_NODE_OPACITY: case RXR_NODE_BUMP:
                        room = true; delta = 1; break;
                    case RXR_NODE_STORE_GLOBAL: case RXR_NODE_STORE_LOCAL: case RXR_NODE_PRINT:
                    case RXR_NODE_SET_UV: case RXR_NODE_SET_NORMAL: case RXR_NODE_SET_COLOR: case RXR_NODE_SET_ROUGHNESS:
                    case RXR_NODE_SET_METALLIC: case RXR_NODE_SET_OPACITY: case RXR_NODE_SET_BUMP: case RXR_NODE_SET_EMISSIVE:
                    case VM_JZ: case VM_FOR_COND:
                        need = 1; delta = -1; break;
                    case RXR_NODE_SWAP: need = 2; break;
                    case VM_GETC: case VM_BINC:
                    case RXR_NODE_LENGTH: case RXR_NODE_LENGTH2: case RXR_NODE_LENGTH3: case RXR_NODE_ABS: case RXR_NODE_SIN: case RXR_NODE_SIN1:
                    case RXR_NODE_SIN2: case RXR_NODE_COS: case RXR_NODE_COS1: case RXR_NODE_COS2: case RXR_NODE_TAN: case RXR_NODE_ATAN:
                    case RXR_NODE_NORMALIZE: case RXR_NODE_FLOOR: case RXR_NODE_CEIL: case RXR_NODE_ROUND: case RXR_NODE_FRACT:
                    case RXR_NODE_DEGREES: case RXR_NODE_RADIANS: case RXR_NODE_SQRT: case RXR_NODE_LOG: case RXR_NODE_NOT: case RXR_NODE_NEG:
                        need = 1; break;
                    case VM_SETC: case RXR_NODE_PACK2:
                    case RXR_NODE_ADD: case RXR_NODE_SUB: case RXR_NODE_MUL: case RXR_NODE_DIV: case RXR_NODE_ATAN2: case RXR_NODE_ROTATE2D:
                    case RXR_NODE_DOT: case RXR_NODE_DOT2: case RXR_NODE_DOT3: case RXR_NODE_CROSS: case RXR_NODE_MOD: case RXR_NODE_MIN:
                    case RXR_NODE_MAX: case RXR_NODE_STEP: case RXR_NODE_POW: case RXR_NODE_EQ: case RXR_NODE_NE: case RXR_NODE_LT:
                    case RXR_NODE_LE: case RXR_NODE_GT: case RXR_NODE_GE: case RXR_NODE_AND: case RXR_NODE_OR:
                    case RXR_NODE_SAMPLE: case RXR_NODE_SAMPLE_NORMAL:
                        need = 2; delta = -1; break;
                    case RXR_NODE_PACK3: case RXR_NODE_MIX: case RXR_NODE_SMOOTHSTEP: case RXR_NODE_CLAMP:
                        need = 3; delta = -2; break;
                    case RXR_NODE_CLEAR: delta = st.depth > 0 ? -1 : 0; break;
                    case RXR_NODE_DUP:
                        if (st.depth > 0) { room = true; delta = 1; }
                        break;
                    case VM_RETURN: delta = st.depth > 0 ? -1 : 0; break;   // (no calls: the function is `shade`)
                    case VM_JMP: case VM_FOR_ENTER: case VM_FOR_TRUNC: case VM_FOR_EXIT: case VM_FAULT: break;
                    default: return false;   // VM_CALL, PaletteIndex, anything unknown: dynamic
                }
                if (st.depth < need) return false;                       // a stack underflow must be reported by the dynamic interpreter
                if (room && st.depth >= (int)RXR_VM_STACK) return false;  // ... and so must an overflow
                code[pc] = (w & 0xFF00FFFFu) | ((uint32_t)st.depth << 16);
                State nx = st;
                nx.depth += delta;
                if (op == VM_FOR_ENTER) {
                    if (nx.loops.size() >= RXR_VM_LOOPS) return false;
                    nx.loops.push_back(st.depth);
                } else if (op == VM_FOR_TRUNC) {
                    if (nx.loops.empty()) return false;
                    nx.depth = std::min(nx.depth, nx.loops.back());
                } else if (op == VM_FOR_EXIT) {
                    if (nx.loops.empty()) return false;
                    nx.loops.pop_back();
                }
                if (op == VM_FAULT) break;                                // the lane stops here
                if (op == VM_JMP || op == VM_RETURN) {
                    pc = code[pc + 1];
                    st = nx;
                    continue;
                }
                if (op == VM_JZ || op == VM_FOR_COND) work.push_back({code[pc + 1], nx});
                pc += len;
                st = nx;
            }
        }
    }
    return true;
}

int rxr_check_shaders(const rxr_shader_set *set, uint32_t *code_words, char *message, uint32_t message_capacity) {
    std::vector<uint32_t> code, reads;
    std::vector<DevProgram> progs;
    std::string err;
    int rc = set ? flatten_programs(set, code, progs, reads, err) : RXR_ERR_INVALID;
    if (code_words) *code_words = (uint32_t)code.size();
    rxr_copy_message(err, message, message_capacity);
    return rc;
}

int rxr_check_bake(const rxr_shader_set *set, uint32_t program, char *message, uint32_t message_capacity) {
    std::vector<uint32_t> code, reads, writes;
    std::vector<DevProgram> progs;
    std::string err;
    int rc = set ? flatten_programs(set, code, progs, reads, err, &writes) : RXR_ERR_INVALID;
    if (rc == RXR_OK) {
        if (program >= progs.size()) {
            rc = RXR_ERR_INVALID;
            err = "program index out of range";
        } else if (progs[program].shade_entry == 0xFFFFFFFFu) {
            rc = RXR_ERR_INVALID;
            err = "the program has no shade function (shade_index -1): Chunk::add_shader bakes nothing for it";
        } else if (const char *why = rxr_bake_refusal(reads[program], writes[program])) {
            rc = RXR_ERR_UNSUPPORTED;
            err = why;
        }
    }
    rxr_copy_message(err, message, message_capacity);
    return rc;
}

int rxr_set_shaders(rxr_ctx *ctx, const rxr_shader_set *set) {
    if (!ctx) return RXR_ERR_INVALID;
    if (ctx->group) return rxr_group_set_shaders(ctx, set);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    {
        int qrc = rxr_quiesce(ctx);  // a render (possibly on the caller's stream) may still run the old programs
        if (qrc != RXR_OK) return qrc;
    }
    ctx->has_frame = false;  // the resident frame's batch headers refer to the old programs
    ctx->programs.clear();
    ctx->programs_static = false;
    ctx->program_field_reads.clear();
    ctx->program_field_writes.clear();
    ctx->n_patterns = ctx->n_normal_patterns = ctx->n_palette = 0;
    if (!set) return RXR_OK;
    if ((set->n_programs && !set->programs) || (set->n_patterns && !set->patterns) || (set->n_normal_patterns && !set->normal_patterns) ||
        (set->n_palette && !set->palette_rgb))
        return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_set_shaders: NULL array");

    // ---- validate + flatten every program into one code stream
    struct {
        std::vector<uint32_t> code;
    } fl;
    std::vector<DevProgram> progs;
    std::vector<uint32_t> field_reads, field_writes;  // per program: PF_* read before written / written anywhere
    {
        std::string err;
        int frc = flatten_programs(set, fl.code, progs, field_reads, err, &field_writes);
        if (frc != RXR_OK) return rxr_fail(ctx, frc, "rxr_set_shaders: " + err);
    }
    {
        const bool no_static = getenv("RXR_VM_NO_STATIC") != nullptr;  // A-B runs / tests: always the dynamic interpreter
        std::vector<uint32_t> tagged = fl.code;
        ctx->programs_static = !no_static && !progs.empty() && tag_static_depths(tagged, progs);
        if (ctx->programs_static) fl.code.swap(tagged);   // (a failed attempt leaves partial tags behind: keep the clean stream then)
    }

    // ---- patterns + palette
    std::vector<DevPattern> pats;
    size_t n_floats = 0;
    auto add_patterns = [&](const rxr_pattern *src, uint32_t n) -> int {
        for (uint32_t i = 0; i < n; ++i) {
            if (!src[i].rgb || src[i].width == 0 || src[i].height == 0 || src[i].width > 32768 || src[i].height > 32768) return RXR_ERR_INVALID;
            DevPattern d{};
            d.offset = (uint32_t)n_floats;
            d.w = src[i].width;
            d.h = src[i].height;
            pats.push_back(d);
            n_floats += (size_t)3 * d.w * d.h;
            if (n_floats >= (1ull << 31)) return RXR_ERR_INVALID;
        }
        return RXR_OK;
    };
    int rc;
    if ((rc = add_patterns(set->patterns, set->n_patterns)) != RXR_OK) return rxr_fail(ctx, rc, "rxr_set_shaders: bad pattern");
    if ((rc = add_patterns(set->normal_patterns, set->n_normal_patterns)) != RXR_OK) return rxr_fail(ctx, rc, "rxr_set_shaders: bad normal pattern");

    auto up = [&](DevBuf &b, const void *src, size_t bytes) -> int {
        int r = rxr_ensure(ctx, b, bytes ? bytes : 16);
        if (r != RXR_OK) return r;
        if (bytes) HIPCHK(ctx, hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, ctx->stream));
        return RXR_OK;
    };
    if ((rc = up(ctx->d_vm_code, fl.code.data(), fl.code.size() * 4)) != RXR_OK) return rc;
    if ((rc = up(ctx->d_programs, progs.data(), progs.size() * sizeof(DevProgram))) != RXR_OK) return rc;
    if ((rc = up(ctx->d_patterns, pats.data(), pats.size() * sizeof(DevPattern))) != RXR_OK) return rc;
    if ((rc = rxr_ensure(ctx, ctx->d_pattern_data, n_floats ? n_floats * 4 : 16)) != RXR_OK) return rc;
    {
        size_t k = 0;
        auto copy_pats = [&](const rxr_pattern *src, uint32_t n) -> int {
            for (uint32_t i = 0; i < n; ++i, ++k)
                HIPCHK(ctx, hipMemcpyAsync((float *)ctx->d_pattern_data.p + pats[k].offset, src[i].rgb, (size_t)12 * pats[k].w * pats[k].h,
                                           hipMemcpyHostToDevice, ctx->stream));
            return RXR_OK;
        };
        if ((rc = copy_pats(set->patterns, set->n_patterns)) != RXR_OK) return rc;
        if ((rc = copy_pats(set->normal_patterns, set->n_normal_patterns)) != RXR_OK) return rc;
    }
    std::vector<float> pal((size_t)set->n_palette * 4);
    for (uint32_t i = 0; i < set->n_palette; ++i) {
        pal[4 * i] = set->palette_rgb[3 * i];
        pal[4 * i + 1] = set->palette_rgb[3 * i + 1];
        pal[4 * i + 2] = set->palette_rgb[3 * i + 2];
        pal[4 * i + 3] = (!set->palette_present || set->palette_present[i]) ? 1.0f : 0.0f;
    }
    if ((rc = up(ctx->d_palette, pal.data(), pal.size() * 4)) != RXR_OK) return rc;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));  // the staging vectors die here
    // opt-in: the set as straight-line kernels compiled now (rxr_jit.hip); sets with calls or PaletteIndex keep the interpreter
    rxr_jit_drop(ctx);
    ctx->jit_info.clear();
    {
        // RXR_SHADER_JIT: unset / "async" -- a child process compiles while the interpreter renders (the default); "1" -- compiled when
        // first needed, the caller waits (measurements); "0" -- interpreted only
        const char *jit = getenv("RXR_SHADER_JIT");
        const char mode = jit ? jit[0] : 'a';
        ctx->jit_async = mode == 'a';
        if ((mode == '1' || mode == 'a') && !progs.empty()) {
            if ((rc = rxr_jit_build(ctx, fl.code, progs)) != RXR_OK) return rc;  // (does its own analysis: calls are covered, PaletteIndex / recursion are not)
        }
    }
    ctx->programs = std::move(progs);
    ctx->program_field_reads = std::move(field_reads);
    ctx->program_field_writes = std::move(field_writes);
    ctx->n_patterns = set->n_patterns;
    ctx->n_normal_patterns = set->n_normal_patterns;
    ctx->n_palette = set->n_palette;
    return RXR_OK;
}

int rxr_selftest_math(rxr_ctx *ctx, uint64_t n_tuples, uint64_t seed, uint64_t mismatches[RXR_MATH_KINDS]) {
    if (!ctx || !mismatches) return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_selftest_math: NULL argument");
    if (ctx->group) return rxr_selftest_math(rxr_member(ctx, 0), n_tuples, seed, mismatches);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const uint32_t iters = 256;
    uint64_t per_block = 256ull * iters;
    uint64_t blocks64 = (n_tuples + per_block - 1) / per_block;
    if (blocks64 == 0) blocks64 = 1;
    if (blocks64 > (1ull << 22)) return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_selftest_math: n_tuples too large (max 2^38)");
    unsigned long long *d = nullptr;
    HIPCHK(ctx, hipMalloc(&d, RXR_MATH_KINDS * sizeof(unsigned long long)));
    hipError_t e = hipMemsetAsync(d, 0, RXR_MATH_KINDS * sizeof(unsigned long long), ctx->stream);
    if (e == hipSuccess) {
        rxr_launch_selftest_math(seed, (uint32_t)blocks64, iters, d, ctx->stream);
        e = hipGetLastError();
    }
    unsigned long long h[RXR_MATH_KINDS] = {0};
    if (e == hipSuccess) e = hipMemcpyAsync(h, d, sizeof(h), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    (void)hipFree(d);
    if (e != hipSuccess) return rxr_fail(ctx, RXR_ERR_HIP, std::string("rxr_selftest_math: ") + hipGetErrorString(e));
    for (int k = 0; k < RXR_MATH_KINDS; ++k) mismatches[k] = h[k];
    return RXR_OK;
}

}  // extern "C"

// what the run-time compiler did with the last program set of this context (rxr_jit.hip); "" when it was not asked
// tests: how the resident frame's 3D arrays arrived -- 0 plain rxr_upload_frame, 1 streamed and copied, 2 streamed out of page-locked memory
// tests: what rxr_upload_frame found out about the resident frame's extent: out[0] = content rows known, out[1], out[2] = the rows, out[3] = row spans in use (1: from the host's boxes, 2: completed on the device)
extern "C" int rxr_debug_content(rxr_ctx *ctx, uint32_t *out) {
    if (!ctx || ctx->group || !out) return -1;
    out[0] = ctx->content_known ? 1u : 0u;
    out[1] = ctx->content_row0;
    out[2] = ctx->content_row1;
    out[3] = ctx->spans_active ? 1u : (ctx->dev_spans ? 2u : 0u);  // (2: completed on the device from the meshes' boxes)
    return 0;
}
// tests: the tile rows anything 3D of the resident frame can reach (rxr_ctx::d3_trow0 / 1; include/rxr.h)
extern "C" int rxr_debug_d3_rows(rxr_ctx *ctx, uint32_t *out) {
    if (!ctx || ctx->group || !out || !ctx->has_frame) return -1;
    out[0] = ctx->d3_trow0;
    out[1] = ctx->d3_trow1;
    return 0;
}
// tests: the scratch words the next launch assumes clear, read back after the context's streams have drained.  Checked:
//   buffer 0: every word of d_bin_count -- bin_count (rxr_device.h RasterParams.bin_count: "all-zero between launches", k_raster hands its
//             bin back) and k_blockscan's per-block group counts behind it (RasterParams.blk_cnt: "all-zero between launches: k_blockscan
//             hands it back"); the rest of the allocation is zeroed when it is made (rxr_upload_frame) and never written;
//   buffer 1: words CNT_LARGE and CNT_TICKET of the 3D counter set `parity` (render_impl: "counter set `parity` is clean (cleared by the
//             previous launch's k_scan)"; the next launch adds to those two with atomics, CNT_ENTRIES / CNT_OVERFLOW it writes before use);
//   buffer 2: the same words of the 2D set 2 + parity2d (cleared likewise by the previous 2D k_scan);
//   buffer 3: every word of d_bin2d_count (RasterParams.bin2d_count: "own zero-invariant buffer, like bin_count").
// out[0] = number of non-zero words, out[1..3] = buffer, word index, value of the first one (all 0 when clean).  A context whose last launch
// sequence was cut short (scratch_dirty) is reported as it is: its next launch restores the invariants anyway.  Finding dirt marks the
// context dirty, so that its next launch clears the buffers instead of building on them (a failed check leaves nothing behind).
extern "C" int rxr_debug_scratch(rxr_ctx *ctx, uint32_t *out) {
    if (!ctx || ctx->group || !out) return -1;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc = rxr_quiesce(ctx);
    if (rc != RXR_OK) return rc;
    out[0] = out[1] = out[2] = out[3] = 0u;
    auto scan = [&](uint32_t id, const uint32_t *dev, size_t words, uint32_t index0) -> int {
        if (!dev || !words) return RXR_OK;
        std::vector<uint32_t> h(words);
        HIPCHK(ctx, hipMemcpy(h.data(), dev, words * sizeof(uint32_t), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < words; ++i)
            if (h[i]) {
                if (!out[0]) out[1] = id, out[2] = index0 + (uint32_t)i, out[3] = h[i];
                out[0]++;
            }
        return RXR_OK;
    };
    if ((rc = scan(0, (const uint32_t *)ctx->d_bin_count.p, ctx->d_bin_count.cap / sizeof(uint32_t), 0u)) != RXR_OK) return rc;
    if (ctx->d_counters.p) {
        const uint32_t *set3 = (const uint32_t *)ctx->d_counters.p + (size_t)ctx->parity * CNT_WORDS;
        const uint32_t *set2 = (const uint32_t *)ctx->d_counters.p + (size_t)(2u + ctx->parity2d) * CNT_WORDS;
        for (uint32_t w : {(uint32_t)CNT_LARGE, (uint32_t)CNT_TICKET})
            if ((rc = scan(1, set3 + w, 1, w)) != RXR_OK) return rc;
        for (uint32_t w : {(uint32_t)CNT_LARGE, (uint32_t)CNT_TICKET})
            if ((rc = scan(2, set2 + w, 1, w)) != RXR_OK) return rc;
    }
    if ((rc = scan(3, (const uint32_t *)ctx->d_bin2d_count.p, ctx->d_bin2d_count.cap / sizeof(uint32_t), 0u)) != RXR_OK) return rc;
    if (out[0]) ctx->scratch_dirty = ctx->scratch2d_dirty = true;
    return 0;
}
// tests (host only, no device): rxr_ref_tile_span (quick == 0) / rxr_ref_tile_span_quick of n boxes [lo, lo + extent] on one axis; out: p0, p1 per box
extern "C" void rxr_debug_tile_spans(const float *lo, const float *extent, uint32_t n, uint32_t size, uint32_t ts, float pad, int quick, uint32_t *out) {
    for (uint32_t i = 0; i < n; ++i) {
        if (quick) rxr_ref_tile_span_quick(lo[i], extent[i], size, ts, pad, out[2 * i], out[2 * i + 1]);
        else rxr_ref_tile_span(lo[i], extent[i], size, ts, pad, out[2 * i], out[2 * i + 1]);
    }
}
// tests: what the last banded rxr_render_download sent over PCIe and what the host wrote itself (bytes)
extern "C" int rxr_debug_download_bytes(rxr_ctx *ctx, uint64_t *out2) {
    if (!ctx || ctx->group || !out2) return -1;
    out2[0] = ctx->last_download_bytes;
    out2[1] = ctx->last_host_fill_bytes;
    return 0;
}
// tests: the device projection's two ticket words (rxr_project.h) after the context's streams have drained: out2[0] = k_proj_scan's
// arrival counter (0 between frames: the workgroup that arrives last hands it back), out2[1] = "a triangle of the last device-projected
// frame appends" (proj_init_item clears it, clip_count_item raises it: 0 lets k_proj_scan and k_clip_emit leave at once)
extern "C" int rxr_debug_projection_ticket(rxr_ctx *ctx, uint32_t *out2) {
    if (!ctx || ctx->group || !out2 || ctx->meshes.empty() || !ctx->PP.ticket) return -1;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc = rxr_quiesce(ctx);
    if (rc != RXR_OK) return rc;
    HIPCHK(ctx, hipMemcpy(out2, ctx->PP.ticket, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return 0;
}
extern "C" int rxr_debug_stream_info(rxr_ctx *ctx) { return (ctx && !ctx->group) ? ctx->last_upload_streamed : -1; }

// tests: how many launch sequences rxr_synchronize has rendered again after a list overflow (a plain context or a member)
extern "C" uint32_t rxr_debug_rerenders(rxr_ctx *ctx) { return (ctx && !ctx->group) ? ctx->rerenders : 0u; }

// tests: the symbol name of the raster kernel of the context's most recent raster launch ("k_raster_rows_cut_rl", "k_raster_jit", ...;
// "" when the last frame launched none); a multi-device handle answers for member 0
extern "C" const char *rxr_debug_last_raster_kernel(rxr_ctx *ctx) {
    if (ctx && ctx->group) ctx = rxr_member(ctx, 0);
    return ctx ? ctx->last_raster_kernel : "";
}
// tests: what the context's most recent render did for the set-up records of a small frame: 0 nothing (no 3D pass, the fused
// mode), 1 it read the records rxr_upload_frame made on the host, 2 it launched k_setup3d; a multi-device handle answers for member 0
extern "C" uint32_t rxr_debug_last_setup_route(rxr_ctx *ctx) {
    if (ctx && ctx->group) ctx = rxr_member(ctx, 0);
    return ctx ? ctx->last_setup_route : 0u;
}
// tests: the resident host-projected frame's set-up records (n x 96 and n x 80 bytes, n = *n_tris <= capacity_tris) as k_setup3d writes them
// for the whole-frame band -- into zeroed scratch: it leaves the records of a workgroup without a drawable triangle alone -- and, when the
// frame carries them, as rxr_upload_frame made them on the host, read back from the frame blob.  Returns 1 with both pairs filled, 0 when
// the frame has no host-made records (only the device's pair is filled), a negative status otherwise (all four pointers are required).
// CLOBBERS the context's scratch records (zeroed, then whole-frame records): harmless, since every render that reads scratch launches
// k_setup3d into it first.
extern "C" int rxr_debug_setup_records(rxr_ctx *ctx, void *host_setup, void *host_shade, void *dev_setup, void *dev_shade, uint32_t capacity_tris,
                                       uint32_t *n_tris) {
    if (!ctx || ctx->group || !n_tris || !dev_setup || !dev_shade || !host_setup || !host_shade) return RXR_ERR_INVALID;
    if (!ctx->has_frame || ctx->frame_uses_meshes) return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_debug_setup_records: no host-projected frame");
    const size_t n = ctx->P.n_tris3d;
    *n_tris = (uint32_t)n;
    if (n > capacity_tris) return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_debug_setup_records: capacity too small");
    if (hipSetDevice(ctx->device) != hipSuccess || rxr_quiesce(ctx) != RXR_OK) return RXR_ERR_HIP;
    if (n) {
        RasterParams P = ctx->P;
        P.row0 = 0;
        P.row1 = P.height;
        P.tile_y0 = 0;
        P.tile_stride = 1;
        P.tiles_y = (P.height + RXR_TILE_H - 1u) / RXR_TILE_H;
        P.fused_small = 2u;
        bool ok = hipMemsetAsync(P.tri_setup, 0, n * sizeof(TriSetup), ctx->stream) == hipSuccess &&
                  hipMemsetAsync(P.tri_shade, 0, n * sizeof(TriShade), ctx->stream) == hipSuccess;
        if (ok) rxr_launch_setup(&P, ctx->stream);
        ok = ok && hipGetLastError() == hipSuccess;
        ok = ok && hipMemcpyAsync(dev_setup, P.tri_setup, n * sizeof(TriSetup), hipMemcpyDeviceToHost, ctx->stream) == hipSuccess;
        ok = ok && hipMemcpyAsync(dev_shade, P.tri_shade, n * sizeof(TriShade), hipMemcpyDeviceToHost, ctx->stream) == hipSuccess;
        if (ok && ctx->host_records) {
            ok = ok && hipMemcpyAsync(host_setup, (uint8_t *)ctx->d_frame.p + ctx->off_host_setup, n * sizeof(TriSetup), hipMemcpyDeviceToHost, ctx->stream) == hipSuccess;
            ok = ok && hipMemcpyAsync(host_shade, (uint8_t *)ctx->d_frame.p + ctx->off_host_shade, n * sizeof(TriShade), hipMemcpyDeviceToHost, ctx->stream) == hipSuccess;
        }
        if (!(hipStreamSynchronize(ctx->stream) == hipSuccess && ok)) return rxr_fail(ctx, RXR_ERR_HIP, "rxr_debug_setup_records: a HIP call failed");
    }
    return ctx->host_records ? 1 : 0;
}
extern "C" const char *rxr_debug_jit_info(rxr_ctx *ctx) {
    if (!ctx) return "";
    if (ctx->group) return rxr_member(ctx, 0) ? rxr_member(ctx, 0)->jit_info.c_str() : "";
    return ctx->jit_info.c_str();
}

// device-free half of the run-time compiler, for tests without a GPU: validates + flattens the set like rxr_check_shaders, generates
// the C++ of its programs (copied to `source`, truncated to its capacity) and, with compile != 0, runs hiprtc for gfx950.
// Returns RXR_OK, the validation status, or RXR_ERR_UNSUPPORTED with the reason in `message` when the set is not covered.
extern "C" int rxr_debug_jit_generate(const rxr_shader_set *set, int compile, char *source, uint32_t source_capacity, char *message, uint32_t message_capacity) {
    std::vector<uint32_t> code, reads;
    std::vector<DevProgram> progs;
    std::string err, gen;
    auto say = [&](const std::string &m) {
        if (message && message_capacity) snprintf(message, message_capacity, "%s", m.c_str());
    };
    say("");
    int rc = set ? flatten_programs(set, code, progs, reads, err) : RXR_ERR_INVALID;
    if (rc != RXR_OK) {
        say(err);
        return rc;
    }
    if (progs.empty()) {
        say("no programs");
        return RXR_ERR_UNSUPPORTED;
    }
    if (!rxr_jit_generate(code, progs, gen, err)) {
        say(err);
        return RXR_ERR_UNSUPPORTED;
    }
    if (source && source_capacity) snprintf(source, source_capacity, "%s", gen.c_str());
    if (compile) {
        std::vector<char> obj;
        double seconds = 0.0;
        double total = 0.0;
        size_t bytes = 0;
        for (int level : jit_level_number) {  // (the three levels rxr_jit_launch may ask for)
            if (!rxr_jit_compile(gen, "gfx950", level, obj, seconds, err)) {
                say(err);
                return RXR_ERR_HIP;
            }
            total += seconds;
            bytes += obj.size();
        }
        seconds = total;
        char m[96];
        snprintf(m, sizeof m, "compiled in %.2f s, %zu bytes", seconds, bytes);
        say(m);
    }
    return RXR_OK;
}

// ---- rendering, rxr_synchronize, download, profiling ---------------------------------------------
// A file of its own, but ONE translation unit with this one: tools/sanitize_cpu.sh builds the host side of the library from a fixed list
// of sources, this file among them, and its library has to load -- every other file calls rxr_synchronize.
#include "rxr_render.hip"
