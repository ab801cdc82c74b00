// rxr_ctx.h -- the context object behind the C ABI (private to the host files: rxr_api.hip, rxr_upload.hip, rxr_multi.hip, rxr_intersect.hip).
//
// A plain context is one HIP device: its streams, the resident textures / meshes / programs, the frame blob and the
// device scratch.  A multi-device context (rxr_create_multi) is a handle whose `group` lists one plain context per
// device plus one host worker thread per member; it owns no device memory itself (rxr_multi.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdlib>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "rxr_device.h"
#include "rxr_launch.h"
#include "rxr_project.h"

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
};
// One device query's lane (rxr_query.h): its calls run on whichever stream the caller names, ordered among themselves by `ev`
struct QueryLane {
    hipEvent_t ev = nullptr;   // recorded behind the last call's launches (on whichever stream they ran)
    bool pending = false;      // ... and not yet waited for (rxr_quiesce)
    DevBuf io;                 // the blocking form's device copies of the caller's host arrays (QueryIO)
};
// The lanes of rxr_ctx::lane.  rxr_quiesce waits for every one -- a call queued on the caller's stream may still be reading what
// the lane's comment names -- and rxr_destroy releases every one
enum : uint32_t {
    Q_ISECT,     // rxr_intersect_to: the meshes and its scratch
    Q_BAKE,      // rxr_bake_shaders_to: the programs and its job list
    Q_TERRAIN,   // rxr_bake_terrain_to: the resident terrain
    Q_HEIGHTS,   // rxr_terrain_hits_to: the resident heights
    Q_MESH,      // rxr_terrain_meshes_to: the resident heights and their presence mask
    Q_GEN,       // rxr_generated_heights_to / rxr_generated_grids_to: the resident generator records
    Q_MESH_UPDATE,   // rxr_update_meshes: the staged copies of the caller's host arrays (both forms block; the lane orders nothing else)
    Q_CHUNK_TEX,     // rxr_set_chunk_textures / rxr_update_chunk_textures: the staged copies of the caller's host texels (all forms block)
    Q_EXCL,          // rxr_generated_meshes_to: the resident generator records, the resident excluded sectors and the call scratch
    Q_TRACE,         // rxr_trace_to: the trace scene, the path state and its keys (it takes Q_ISECT as well: the triangle records)
    Q_NORMALS,       // rxr_vertex_normals_to: the general route's scratch (face normals, corner keys, the sort's own)
    Q_FLATTEN,       // rxr_flatten_terrain_to: the resident flatten ops; it WRITES the processed heights, so it waits for Q_HEIGHTS and
                     // Q_MESH as well, and picks and mesh builds that read the processed grid wait for it
    Q_LANES
};
#define RXR_MAX_TILE_ROWS 2048u   // frames of at most 32768 rows

struct TileRange {
    uint32_t first, n;
};

// host-side record of one registered mesh (rxr_set_meshes)
struct HostMesh {
    DevMesh dev;              // static part (bases, counts, cull mode); view_model / rejected are per frame
    float transform[16];
    float aabb_lo[3], aabb_hi[3];
    bool has_vertices;
    uint32_t repeat_mode;
    rxr_source source;
    float ambient[3];
    int32_t shader;
    uint32_t has_profile_id, profile_id, list;
    int32_t chunk;
};

// one sampled render of the rxr_profile_begin ring: a (start, stop) event pair per launched kernel (rxr_launch.h)
using ProfSlot = LaunchTimes;

// one render launch sequence.  Band mode: rows [row0,row1), stride 1.  Stripe mode: every `stride`-th
// 16-row stripe from `first`, into a compact buffer (compact) or at its place in a whole frame (!compact).
struct RenderSpec {
    uint32_t row0, row1;
    uint32_t tile_y0, tile_stride, tiles_y;
    bool compact, external;
};

// pinned host words the device writes (rxr_ctx.h_counters): [0, CNT_WORDS) 3D bins, [CNT_WORDS, 2 CNT_WORDS) 2D bins,
// then the words below.  The overflow flags and the maxima are STICKY: the device only ever sets / raises them, the host
// clears them in rxr_synchronize after both streams have drained.
enum : uint32_t {
    HS_VM_FAULT = 2 * CNT_WORDS,        // a non-zero VMF_* code if any fragment's program faulted
    HS_STAIRCASE = 2 * CNT_WORDS + 1,   // != 0: a pixel's opacity staircase (rxr_kernels.hip front_insert) had to drop an entry
    HS_BAD_LINE2D = 2 * CNT_WORDS + 2,  // != 0: device-projected 2D batches: a visible segment's end point lies beyond +-2^30 (k_proj2d_prims)
    HS_WORDS = 2 * CNT_WORDS + 4,
};
// inside a set of CNT_WORDS host words: CNT_ENTRIES = entries of the LAST launch, CNT_OVERFLOW = sticky flag,
// CNT_LARGE (unused by the host otherwise) = the largest entry count seen by a launch that overflowed
#define HS_MAX_ENTRIES CNT_LARGE

struct rxr_group;

// Resident chunk textures (rxr_set_chunk_textures, rxr_chunk_tex.hip): what chunk.terrain_texture / chunk.shader_textures are while a
// registration is held.  slots[i]: size, place in the pool (texels from its start, a multiple of four: 16 bytes) and the flag "every
// texel has alpha 255" as k_chunk_tex_commit last computed it; terrain / shader_first / shader_slots: the caller's maps, copied.
struct ChunkTextures {
    struct Slot { uint32_t w, h, offset, opaque; };
    bool set = false;
    std::vector<Slot> slots;
    std::vector<int32_t> terrain;          // [n_chunks] slot or -1
    std::vector<uint32_t> shader_first;    // [n_chunks + 1]
    std::vector<int32_t> shader_slots;     // slot or -1
    DevBuf pool;                           // the texels
    DevBuf flags;                          // one word per source of the call in flight (k_chunk_tex_commit)
    uint32_t launches = 0;                 // k_chunk_tex_commit launches of the last call (rxr_debug_chunk_tex_launches)
};

// Streaming hand-over of a large frame's projected 3D batches (rxr_stream_begin / rxr_stream_batch3d, include/rxr.h): the host
// hands batch i over from whatever thread projected it; batches are RETIRED in index order (which fixes their dense offsets in
// the vertex / triangle pools, i.e. the submission order the depth tie-break needs), copied into the pinned staging blob by the
// retiring thread and shipped to the device per group of consecutive batches -- all while later batches are still being projected.
struct FrameStream {
    bool active = false;
    uint32_t n = 0;
    struct Rec {
        const float *pv, *uv, *nrm;
        const uint32_t *idx;
        const void *edges;        // rxr_edges records, or (S.edgeless) the uint32 `visible` words
        uint32_t nv, nt;
        size_t v0, t0;
        const void *dev[5];  // pinned mode: the DEVICE addresses of pv, uv, nrm, idx, edges (hipPointerGetAttributes: for memory registered with
                             // hipHostRegister they need not equal the host addresses; the pull kernel reads through these)
    };
    std::vector<Rec> rec;
    std::vector<uint32_t> cap_v, cap_t;
    std::unique_ptr<std::atomic<uint8_t>[]> done;
    std::unique_ptr<std::atomic<uint32_t>[]> group_left;
    uint32_t group_size = 1, n_groups = 0;
    std::mutex mu;       // retirement: next / vcur / tcur
    std::mutex ship_mu;  // the HIP calls of a group's transfers
    uint32_t next = 0;                      // batches [0, next) are retired (under mu)
    std::atomic<uint32_t> retired{0};       // ... the same, readable without the lock
    std::atomic<uint32_t> copy_next{0};     // copy mode: batches [0, copy_next) have been claimed for their copy into pinned memory
    size_t vcur = 0, tcur = 0;
    size_t total_cap_v = 0, total_cap_t = 0;
    size_t off_pv = 0, off_uv = 0, off_nrm = 0, off_idx = 0, off_edges = 0, off_after = 0;  // the blob's layout up to the end of the edges
    size_t blob_capacity = 0;  // staging / device blob bytes that exist without a reallocation
    // pinned mode (rxr_stream_begin_pinned): no host copy; per group a table of (source, destination, bytes) in pinned memory and one
    // k_gather_host launch that pulls the arrays over PCIe
    bool pinned = false;
    struct GatherEntry {
        const void *src;
        uint64_t dst_off;       // bytes from the blob's start
        uint32_t bytes, first_piece;
    };
    GatherEntry *table = nullptr;   // pinned, 5 entries per batch
    size_t table_cap = 0;
    std::atomic<uint32_t> handed{0};
    std::atomic<int> failed{0};
    std::atomic<int> edgeless{-1};  // -1 until the first batch with triangles arrives; then 1: batches come without Edges records (ABI 5), 0: with
    size_t tri5() const { return edgeless.load() == 1 ? sizeof(uint32_t) : sizeof(rxr_edges); }  // bytes per triangle in the fifth pool
    std::string err;     // (under mu)
};

struct rxr_ctx {
    int device = 0;
    rxr_group *group = nullptr;          // != nullptr: multi-device handle (every other member below is unused)
    hipStream_t stream = nullptr;
    uint32_t prof_stride = 1, prof_calls = 0;  // rxr_profile_stride: every prof_stride-th render records events
    hipStream_t copy_stream = nullptr;   // rxr_rasterize: downloads of finished bands overlap the rendering of the next ones
    hipEvent_t ev_band[8] = {};
    std::string err;

    // textures
    DevBuf d_tex, d_texels;
    std::vector<DevTexDesc> h_tex;
    std::vector<TileRange> tiles_static, tiles_dynamic;
    ChunkTextures ctex;              // rxr_set_chunk_textures

    // frame blob
    void *h_stage = nullptr;
    size_t h_stage_cap = 0;
    DevBuf d_frame;
    size_t last_blob_tail = 0;       // bytes of the last frame blob behind the projected arrays (rxr_stream_begin leaves room for twice that)
    DevBuf d_tri_setup, d_tri_shade, d_tri_box, d_bin_count, d_bins, d_list, d_large, d_counters, d_fb;
    DevBuf d_bin2d_count, d_bins2d, d_list2d, d_large2d;
    DevBuf d_stripes;                // multi-device member: this device's stripes, compact (rxr_multi.hip)
    uint32_t list2d_capacity = 0, parity2d = 0;
    uint32_t *h_counters = nullptr;  // pinned, HS_WORDS; written by the device through d_host_status
    uint32_t *d_host_status = nullptr;
    uint32_t list_capacity = 0;
    size_t list_floor = 0;           // RXR_LIST_CAPACITY_FLOOR (tests): initial size of the bin lists instead of the generous default
    uint32_t parity = 0;             // counter set of the next launch
    bool scratch_dirty = false;      // a pre-pass was queued without its raster launch
    bool scratch2d_dirty = false;
    uint32_t min_kernel_level = KL_COMMON;   // RXR_MIN_KERNEL_LEVEL (tuning)
    // run-time compiled kernels of the current program set (rxr_jit.hip; opt-in RXR_SHADER_JIT=1), else null: the interpreter runs
    // (one module per JitSlot, compiled when the first frame that needs it is launched; jit_source: the generated
    // programs of the current set, empty when the set is not covered)
    void *jit_module[N_JIT_SLOTS] = {nullptr, nullptr, nullptr}, *jit_fn[N_JIT_SLOTS] = {nullptr, nullptr, nullptr};
    void *jit_fn_cut[N_JIT_SLOTS] = {nullptr, nullptr, nullptr};   // k_raster_jit_cut of the same module (JIT_NO_VIS / JIT_PLAIN), or null
    bool jit_failed[N_JIT_SLOTS] = {false, false, false};
    bool jit_palette_miss = false;   // a compiled frame met a PaletteIndex without a colour: this set runs interpreted from now on (VMF_JIT_PALETTE_MISS)
    // background mode (the default): the compilation of a level runs in a child process (rxr_jitc); the interpreter renders until it is done
    bool jit_async = false;
    std::string jit_wait_key[N_JIT_SLOTS];           // the background compilation (rxr_jit.hip registry) this context is attached to, per level
    std::string jit_source, jit_arch;
    // mid-sized scenes: bin lists by k_blockscan (rxr_device.h RXR_BLOCKSCAN_*).  blockscan_off: the current frame overflowed a block or a
    // bin and goes through the general pipeline (reset by the next upload); RXR_BLOCKSCAN=0 turns the mode off, RXR_BLOCKSCAN_CAP sets
    // the slots per bin (tests)
    bool blockscan_enabled = true, blockscan_off = false, last_used_blockscan = false;
    // the (primitives, bins) of the last frames that overflowed k_blockscan / k_blockscan2d (a ring of eight each): frames of such a shape
    // do not try again -- a caller that uploads every frame would pay the failed attempt and the second rendering every time
    struct BadShapes {
        size_t prims[8] = {}, bins[8] = {};
        uint32_t next = 0;
        bool has(size_t p, size_t b) const {
            for (int i = 0; i < 8; ++i)
                if (prims[i] == p && bins[i] == b && p) return true;
            return false;
        }
        void add(size_t p, size_t b) {
            if (has(p, b)) return;
            prims[next % 8u] = p;
            bins[next % 8u] = b;
            ++next;
        }
    } blockscan_bad, blockscan2d_bad;
    bool blockscan2d_off = false, last_used_blockscan2d = false;  // the same for the 2D bins (k_blockscan2d); RXR_BLOCKSCAN2D=0 turns it off
    uint32_t blockscan_cap = 0;           // RXR_BLOCKSCAN_CAP in effect
    bool relaxed_lights = true;           // rxr_set_light_math / RXR_LIGHT_MATH: the 3D light loop in relaxed arithmetic (RasterParams.relaxed_lights)
    bool frame_needs_chunk_paths = true;  // the uploaded frame uses the chunk paths (LevelFeatures.chunk: terrain / baked textures / staircase / editor paths)
    std::string jit_info;                // what happened to the last set ("compiled: ...", "not compiled: <why>", empty: not asked)
    bool programs_static = false;    // every program of the set has a stack depth that is a function of the pc (tag_static_depths)
    uint32_t small_mode = 2;         // RasterParams.fused_small for frames with <= RXR_STAGE_TRIS triangles;
                                     // RXR_SMALL_MODE=0|1|2 overrides it (tests / A-B runs)
    // Small host-projected frames (small_mode 2): rxr_upload_frame builds the TriSetup / TriShade records on the host, for the whole-frame
    // band, into two sections of the frame blob (rxr_tri_records, rxr_device.h); a render whose band lies on tile rows reads them there and
    // launches no k_setup3d.  The sections are immutable until the next upload.
    bool host_setup_on = true;       // RXR_HOST_SETUP=0 (read by rxr_create) keeps the launch (tests / A-B runs)
    bool host_records = false;       // the resident frame carries them ...
    size_t off_host_setup = 0, off_host_shade = 0;  // ... at these offsets of d_frame
    uint32_t last_setup_route = 0;   // what the last render did for the set-up records: 0 nothing (no 3D pass), 1 the blob's host-made
                                     // records, 2 a k_setup3d launch (rxr_debug_last_setup_route: tests)

    // device-side projection (rxr_set_meshes)
    std::vector<HostMesh> meshes;
    DevBuf d_obj, d_proj_out, d_proj_misc;
    ProjectParams PP{};
    size_t mesh_verts_out = 0, mesh_tris_out = 0;
    size_t pp_off_meshes = 0;  // byte offset of the per-frame DevMesh array inside d_proj_misc
    size_t obj_off_meshes = 0; // byte offset of the registration's static DevMesh array inside d_obj (PP.meshes moves to the per-frame one)
    DevBuf d_mesh_check;       // rxr_update_meshes: one MeshCheckRec per named mesh (rxr_resize_meshes: one MeshResizeRec)
    hipEvent_t ev_repack[2] = {nullptr, nullptr};   // rxr_resize_meshes: around the last k_mesh_repack launch (rxr_debug_resize_repack; made by the first resize)
    uint64_t repack_bytes = 0;                      // ... and the bytes it wrote (it reads as many)
    DevBuf d_obj_alt;          // rxr_resize_meshes: the object blob that is not in use; the new pools are built in it from d_obj, then the two swap
    DevBuf d_mirror_scratch;   // rxr_mirror_scratch (rxr_api.hip): a host layer's device scratch
    bool frame_uses_meshes = false;
    // ... and its 2D half (rxr_set_meshes2d / rxr_set_projection2d)
    struct HostMesh2D {
        uint32_t vin_base, n_verts, n_tris, n_prims, prim_base, mode, repeat_mode, receives_light;
        rxr_source source;
        int32_t shader, chunk;
    };
    std::vector<HostMesh2D> meshes2d;
    DevBuf d_obj2d, d_proj2d_misc;
    Project2DParams PP2{};
    size_t meshes2d_prims = 0, meshes2d_tris = 0;
    bool has_matrix2d = false;
    float matrix2d[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    bool frame_uses_meshes2d = false;

    // Rusteria programs (rxr_set_shaders)
    DevBuf d_vm_code, d_programs, d_patterns, d_pattern_data, d_palette;
    std::vector<DevProgram> programs;
    std::vector<uint32_t> program_field_reads;  // PF_* each program reads before writing (see rxr_set_shaders)
    std::vector<uint32_t> program_field_writes; // PF_* each program writes anywhere (rxr_bake_refusal)
    std::vector<uint32_t> program_flags;        // PG_* per program (see rxr_set_shaders)
    uint32_t n_patterns = 0, n_normal_patterns = 0, n_palette = 0;
    bool frame_uses_programs = false;

    QueryLane lane[Q_LANES];         // the device queries below: stream ordering and staging (rxr_query.h)

    // ray picking (rxr_intersect.hip): buffers of its own -- an intersect never touches the frame state (has_frame, the bins, the
    // counters).  d_isect_tris: (p0, edge1, edge2) per registered triangle; d_isect_misc: the segments and per-mesh profile ids
    // (isect_host: their host copy, kept alive for the asynchronous upload); d_isect_keys: per ray and segment the (t, triangle)
    // minimum.
    DevBuf d_isect_tris, d_isect_misc, d_isect_keys;
    std::vector<uint32_t> isect_host;
    bool meshes_valid = true;        // false while / after an rxr_set_meshes that did not complete
    bool isect_ready = false;        // d_isect_tris / d_isect_misc describe the current meshes but for those of refresh_named (rxr_set_meshes clears it)
    uint32_t isect_nseg = 0, isect_stride = 0;
    size_t isect_off_pid = 0;        // words into d_isect_misc

    // the opt-in box tree over the same triangles (rxr_ray_accel.hip; rxr_set_ray_accel).  d_accel_tris / d_accel_perm: the records in
    // sorted order and each position's global triangle; d_accel_nodes: the levels, leaves first; d_accel_stats: two 64-bit words, the
    // ray-triangle tests of the last counted call and the wild triangles; d_accel_scratch: the build's keys and the sort's scratch.
    DevBuf d_accel_tris, d_accel_perm, d_accel_nodes, d_accel_stats, d_accel_scratch;
    uint32_t accel_mode = 0;         // RXR_RAY_ACCEL_*
    bool accel_ready = false;        // the tree describes the records of isect_ready (isect_prepare clears it with them)
    bool accel_stats_zeroed = false;
    uint32_t accel_ntri = 0, accel_nodes = 0, accel_levels = 0;
    uint64_t accel_builds = 0, accel_batches = 0;
    // a wave per ray through that tree (rxr_set_ray_wave; k_accel_by_wave): the mode, and the batches and rays that went that way
    uint32_t wave_mode = 0;          // RXR_RAY_WAVE_*
    uint64_t wave_batches = 0, wave_rays = 0;

    // ranged refresh after rxr_update_meshes (rxr_set_ray_refresh).  refresh_named: one byte per registered mesh,
    // 1 while an update named it and no query has run since (refresh_pending of them; only ever set while isect_ready);
    // d_refresh_table: the dirty meshes' triangle ranges and the refit's node intervals (refresh_host: their host copy, kept alive for
    // the asynchronous upload); d_refresh_verify: rxr_ray_refresh_verify's recomputed arrays and its four counters.
    uint32_t refresh_mode = 0;       // RXR_RAY_REFRESH_*
    std::vector<uint8_t> refresh_named;
    uint32_t refresh_pending = 0;
    DevBuf d_refresh_table, d_refresh_verify;
    std::vector<uint32_t> refresh_host;
    uint64_t refresh_count = 0, refit_count = 0;
    uint32_t refresh_last_tris = 0, refresh_last_leaves = 0, refresh_last_nodes = 0, refresh_last_route = 0;

    // path tracing (rxr_trace.hip): buffers of its own, like the intersect's.  d_trace_scene: the blob of rxr_set_trace_scene -- the
    // segment table over the participating meshes, one record per mesh (texel source, repeat mode, material), the lights, the
    // sRGB table and one record per terrain-sourced mesh (trace_off: their byte offsets); d_trace_paths: per pixel origin, direction, throughput, radiance and the live flag;
    // d_trace_keys: per ray and segment the (t, triangle) minimum of a batch of rays.
    DevBuf d_trace_scene, d_trace_paths, d_trace_keys;
    bool trace_set = false;          // d_trace_scene describes the current meshes and textures (rxr_set_meshes / rxr_set_textures / rxr_set_chunk_textures clear it)
    size_t trace_off[5] = {};
    uint32_t trace_nseg = 0, trace_n_lights = 0, trace_sample_mode = 0, trace_hash_anim = 0;

    // shader-texture bakes (rxr_bake.hip): buffers of their own, like the intersect's -- a bake touches neither the frame state nor the
    // compiled programs.  d_bake_jobs: the program index per bake of the launches in flight (a ring of bake_jobs_cap words, filled
    // through its page-locked twin h_bake_jobs); d_bake_fault: BAKE_FAULT_WORDS words, sticky (the first faulting texel wins) until
    // the host has reported them; h_bake_fault: their pinned host copy, refreshed behind every bake.
    DevBuf d_bake_jobs, d_bake_fault;
    uint32_t *h_bake_fault = nullptr, *h_bake_jobs = nullptr;
    size_t bake_jobs_cap = 0;        // words
    size_t bake_jobs_used = 0;       // ... of which launches since the last rxr_quiesce may still read this many
    uint32_t last_bake_kernel = 0;   // the last bake launch's kernel: 0 none yet, 1 k_bake, 2 k_bake_s (rxr_debug_last_bake_kernel: tests)

    // terrain chunk textures (rxr_terrain.hip): the resident terrain of rxr_set_terrain and the bake's buffers, all its own.
    // d_terrain_cells: the dense grid (TerrainCell per cell of the bounding rectangle); d_terrain_tex / _texels: the source textures'
    // records and packed texels; d_terrain_weights: 256 table offsets by radius, then one tap-weight table per radius in use.
    // terrain_blend: the grid's blend words on the host (the work estimate that splits a call into launches reads them).
    DevBuf d_terrain_cells, d_terrain_tex, d_terrain_texels, d_terrain_weights;
    std::vector<uint32_t> terrain_blend;
    bool terrain_set = false;
    float terrain_scale[2] = {1.0f, 1.0f};
    int32_t terrain_chunk_size = 0, terrain_x0 = 0, terrain_y0 = 0;
    uint32_t terrain_gw = 0, terrain_gh = 0, terrain_max_steps = 0;
    uint32_t terrain_launches = 0;    // k_terrain_bake launches of the last bake call (rxr_debug_terrain_launches)

    // terrain picks (rxr_terrain_hit.hip): the resident heights of rxr_set_terrain_heights, independent of the resident terrain above.
    // d_heights: the dense f32 grid over the cells' bounding rectangle; d_heights_tk: the 1500 values t_k of the march;
    // d_heights_mask: one byte per cell of the same grid, 1 where the caller listed the cell (rxr_terrain_mesh.hip: a listed 0.0 is a
    // cell of the mesh, an unlisted one is not).
    DevBuf d_heights, d_heights_tk, d_heights_mask;
    bool heights_set = false;
    float heights_scale[2] = {1.0f, 1.0f};
    int32_t heights_x0 = 0, heights_y0 = 0;
    uint32_t heights_gw = 0, heights_gh = 0;
    uint32_t heights_launches = 0;    // march launches of the last hit call (rxr_debug_terrain_hit_kernel)
    const char *heights_kernel = "";  // ... and their kernel's symbol name; a static string
    // flattened heights (rxr_terrain_flatten.hip): d_pheights / d_pheights_mask, the PROCESSED grid and mask over the rectangle of
    // d_heights, a copy of it after every rxr_set_terrain_heights and rewritten chunk by chunk by rxr_flatten_terrain[_to];
    // height_source: which pair the picks and the mesh builds read (rxr_set_terrain_height_source); d_flatten: the resident op and
    // edge / segment records of rxr_set_terrain_flatten (flatten_off: their byte offsets)
    DevBuf d_pheights, d_pheights_mask, d_flatten;
    uint32_t height_source = 0;       // RXR_TERRAIN_HEIGHTS_REGISTERED
    size_t flatten_off[2] = {};
    uint32_t flatten_ops = 0;         // resident ops
    uint32_t flatten_seg_slots = 0;   // the sum of the linedef ops' range lengths: a workgroup's segment list in LDS
    uint32_t flatten_launches = 0;    // launches of the last flatten call (rxr_debug_terrain_flatten_launches)
    uint32_t mesh_launches = 0;       // k_terrain_mesh launches of the last mesh call (rxr_debug_terrain_mesh_launches)

    // generated terrain heights (rxr_terrain_gen.hip): the resident records of rxr_set_terrain_generator, independent of both terrains
    // above.  d_gen: one blob of control points, ridges, ridge edge offsets, ridge edges and linedefs, in the kernel's record layout
    // (gen_off: their byte offsets; gen_n: control points, ridges, ridge edges, linedefs).
    DevBuf d_gen;
    bool gen_set = false;
    size_t gen_off[5] = {};
    uint32_t gen_n[4] = {};
    float gen_box[4] = {};
    uint32_t gen_launches = 0;        // launches of the last evaluation call (rxr_debug_terrain_gen_launches)

    // excluded sectors of the generated terrain's chunk meshes (rxr_terrain_excl.hip): the resident records of rxr_set_terrain_exclusions,
    // independent of the generator's.  d_excl: one blob of sector boxes [S][4], vertex offsets [S + 1] and one edge record per polygon
    // vertex (excl_off: their byte offsets); excl_boxes: the boxes' host copy (which sectors are active for a chunk box decides its
    // layout, and with it what the call refuses); d_excl_scratch: a call's heights and inside-bits, reused launch after launch.
    DevBuf d_excl, d_excl_scratch;
    size_t excl_off[3] = {};
    uint32_t excl_S = 0, excl_V = 0;
    std::vector<float> excl_boxes;
    std::vector<uint32_t> excl_voff{0u};   // ... and of the vertex offsets (a round's work counts the vertices of a box's active sectors)
    uint32_t excl_launches = 0;       // classification launches of the last mesh call (rxr_debug_terrain_excl_launches)

    // tile overrides of the generated terrain's chunk meshes (rxr_terrain_excl.hip, partition_by_tiles): the resident map of
    // rxr_set_terrain_tiles, independent of the generator and the exclusions.  d_tiles: the cells' keys [n] (u64: x then z, each
    // with its sign bit flipped, ascending) and behind them their tile slots [n]; tile_keys / tile_slots: their host copies (how many
    // groups a chunk box can have is bounded on the host, and decides what the call refuses).
    DevBuf d_tiles;
    uint32_t tile_cells = 0, tile_count = 1;
    std::vector<uint64_t> tile_keys;
    std::vector<uint32_t> tile_slots;
    uint32_t tile_launches = 0;       // emission launches of the last tile-mesh call (rxr_debug_terrain_tile_launches)

    // vertex normals (rxr_normals.hip): d_nrm_scratch: the general route's face normals, corner keys and values (in and out) and the
    // sort's scratch, reused launch after launch; nothing is resident between calls.
    DevBuf d_nrm_scratch;
    uint32_t nrm_route = 0;           // the last call's route: 0 none yet, RXR_VERTEX_NORMALS_ROUTE_* (rxr_debug_vertex_normals)
    uint32_t nrm_launches = 0;        // ... and its launches: workgroup-per-mesh launches, or rounds of the general route

    FrameStream fstream;    // rxr_stream_begin .. rxr_upload_frame
    int last_upload_streamed = 0;  // 0 plain, 1 streamed (copied), 2 streamed out of page-locked arrays

    bool has_frame = false;
    // Rows [content_row0, content_row1) hold everything the resident frame can draw (rxr_upload_frame; content_known false: unknown, the
    // whole frame): outside them every pixel is the 3D miss colour, which render_impl writes with a fill instead of launching tiles there
    bool content_known = false;
    uint32_t content_row0 = 0, content_row1 = 0;
    // Tile rows [d3_trow0, d3_trow1) hold everything 3D of the resident frame (RasterParams.d3_trow0 / 1): from the edge functions of the
    // records build_setup_records has just made, so small host-projected frames only; 0, 0xFFFFFFFF otherwise (all rows).  Not part of
    // the content rows or the spans: it changes no route, only what a launched workgroup of k_raster[_rl] does
    uint32_t d3_trow0 = 0, d3_trow1 = 0xFFFFFFFFu;
    // ... and per frame tile row the tile columns [x, y) it can draw in (RasterParams.row_spans): built by rxr_upload_frame from the batch
    // boxes in page-locked memory, copied to the device and used when they leave out enough of the content rows (spans_active)
    uint2 *h_row_spans = nullptr;    // RXR_MAX_TILE_ROWS entries, page-locked
    DevBuf d_row_spans;
    bool spans_active = false;
    bool dev_spans = false;          // device-projected meshes: the table is completed on the device behind the projection (k_spans_from_meshes)
    uint64_t last_download_bytes = 0, last_host_fill_bytes = 0;  // the last banded rxr_render_download: over PCIe / written by the host (tests)
    RasterParams P{};       // template for the resident frame (pointers resolved)
    uint32_t n_tris2d = 0;

    // last render
    bool rendered = false;
    bool last_had_prepass = false, last_had_prepass2d = false;
    uint32_t launches_since_sync = 0;   // renders queued since rxr_synchronize last drained the streams
    uint32_t rerenders = 0;             // launches rendered again by rxr_synchronize after a list overflow
    const char *last_raster_kernel = "";  // symbol name of the last raster launch's kernel (rxr_debug_last_raster_kernel: tests); a static string
    RenderSpec last_spec{};
    void *last_out = nullptr;
    hipStream_t last_stream = nullptr;
    hipStream_t upload_ordered_on = nullptr;  // stream already ordered behind the last upload
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr, ev_upload = nullptr;
    hipEvent_t ev_render = nullptr;     // recorded on the previous stream when a render moves to ANOTHER stream (orders it behind the earlier ones)
    ProfSlot *last_prof = nullptr;  // the slot of the last render, if it was sampled (rxr_get_stats)
    std::vector<ProfSlot> prof;  // rxr_profile_begin ring
    size_t prof_next = 0;
    rxr_stats stats{};
};

// ---- helpers shared by the host translation units (defined in rxr_api.hip) ------------------------
int rxr_fail(rxr_ctx *ctx, int code, const std::string &msg);
int rxr_ensure(rxr_ctx *ctx, DevBuf &b, size_t bytes);
int rxr_ensure_stage(rxr_ctx *ctx, size_t bytes);  // the same for the pinned staging blob (ctx->h_stage)
// waits until nothing queued by this context -- on its own streams or on the caller's stream of the last render -- is
// still running: the precondition for rewriting the staging blob, the frame blob or any scratch buffer
int rxr_quiesce(rxr_ctx *ctx);
// one render launch sequence of a plain context (rxr_render.hip)
extern "C" int rxr_render_spec(rxr_ctx *ctx, const RenderSpec &spec, void *dev_pixels, hipStream_t s);

// ---- defined here: what several host files need (rxr_render.hip, rxr_upload.hip, ...) ----------------------------------
// sparse frames (rxr_ctx::content_row0 / 1, row spans): the empty tiles a clamp must save before its fill launches pay (RXR_CONTENT_MIN_TILES
// overrides it -- the tests use small frames)
static inline size_t content_min_tiles() {
    const char *e = getenv("RXR_CONTENT_MIN_TILES");
    return e ? (size_t)atol(e) : 8192u;
}

// Execution fields whose lanes the raster loops do not (all) assign before each call (rasterizer.rs:773-785, :1259-1298,
// :1637-1662): a read sees what an EARLIER fragment's program left there unless this invocation wrote the field first
enum : uint32_t { PF_UV = 1, PF_ROUGHNESS = 2, PF_METALLIC = 4, PF_OPACITY = 8, PF_BUMP = 16, PF_NORMAL = 32, PF_HITPOINT = 64, PF_EMISSIVE = 128 };
// DevProgram.flags
enum : uint32_t {
    PG_WRITES_OPACITY = 1,     // contains SetOpacity: an opaque-pass batch running it needs the program in the visibility loop
    PG_WRITES_EMISSIVE = 2,    // contains SetEmissive (anywhere, callees included)
    PG_ASSIGNS_EMISSIVE = 4,   // `shade` executes a SetEmissive on EVERY path to its end (definite assignment, see PurityCheck)
};

// The bake's acceptance rule (include/rxr.h, rxr_bake_shaders) on top of rxr_set_shaders': Rusteria::shade keeps one Execution per
// tile and resets only uv and color between texels (rusteria/src/lib.rs:177-195), so roughness, metallic, opacity, normal and bump
// carry over from texel to texel -- a program that writes one of them must not read it before the same invocation wrote it.  `reads`:
// PF_* read before written, `writes`: PF_* written anywhere, both from the definite-assignment walk of rxr_set_shaders (PurityCheck).
// (For the raster loops `normal` is assigned before every call and therefore not part of rxr_set_shaders' own rule.)
static inline const char *rxr_bake_refusal(uint32_t reads, uint32_t writes) {
    if (reads & writes & (PF_ROUGHNESS | PF_METALLIC | PF_OPACITY | PF_NORMAL | PF_BUMP))
        return "bake: the program reads roughness / metallic / opacity / normal / bump before writing it and writes that field (Rusteria::shade "
               "resets only uv and color between texels: the read would see the previous texel's value)";
    return nullptr;
}
// rxr_bake.hip: turns the pinned fault words of a bake into RXR_ERR_INVALID + message and clears them (streams idle)
// (the device's words: the VMF_* code, then the program, the bake of the call and the texel it happened in; _SCRATCH: the interpreter's own report)
enum : uint32_t { BAKE_FAULT_CODE = 0, BAKE_FAULT_PROGRAM, BAKE_FAULT_JOB, BAKE_FAULT_X, BAKE_FAULT_Y, BAKE_FAULT_SCRATCH, BAKE_FAULT_WORDS = 8 };
int rxr_bake_report_fault(rxr_ctx *ctx);

static inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

static inline uint32_t pack_px(const uint8_t p[4]) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }

// the cursor that lays a blob out: take(bytes) is where the next section starts; sections are 256-byte aligned, an empty one keeps 16 bytes
struct BlobCursor {
    size_t o = 0;
    size_t operator()(size_t bytes) {
        size_t at = o;
        o = align_up(o + (bytes ? bytes : 16), 256);
        return at;
    }
};

#define HIPCHK(ctx, call)                                                                                  \
    do {                                                                                                   \
        hipError_t e_ = (call);                                                                            \
        if (e_ != hipSuccess)                                                                              \
            return rxr_fail(ctx, RXR_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_));          \
    } while (0)

// ---- multi-device handles (rxr_multi.hip); every function expects ctx->group != nullptr -------------
void rxr_group_destroy(rxr_ctx *ctx);
int rxr_group_set_textures(rxr_ctx *ctx, const rxr_tile *static_tiles, uint32_t n_static, const rxr_tile *dynamic_tiles, uint32_t n_dynamic);
int rxr_group_set_meshes(rxr_ctx *ctx, const rxr_mesh3d *meshes, uint32_t n_meshes);
int rxr_group_update_meshes(rxr_ctx *ctx, const uint32_t *mesh_indices, uint32_t n, const uint32_t *counts, const float *vertices, const uint32_t *indices,
                            const float *normals, uint32_t vertex_stride, uint32_t triangle_stride);
int rxr_group_resize_meshes(rxr_ctx *ctx, const uint32_t *mesh_indices, uint32_t n, const uint32_t *counts, const float *vertices, const float *uvs,
                            const uint32_t *indices, const float *normals, uint32_t vertex_stride, uint32_t triangle_stride);
int rxr_group_each(rxr_ctx *ctx, const std::function<int(rxr_ctx *)> &fn);   // fn(member) for every member, on the members' worker threads
int rxr_group_set_meshes2d(rxr_ctx *ctx, const rxr_mesh2d *meshes, uint32_t n_meshes);
int rxr_group_set_projection2d(rxr_ctx *ctx, const float *mat3);
int rxr_group_set_shaders(rxr_ctx *ctx, const rxr_shader_set *set);
int rxr_group_upload_frame(rxr_ctx *ctx, const rxr_frame *frame);
int rxr_group_render(rxr_ctx *ctx);                          // every member renders its stripes (asynchronous)
int rxr_group_download(rxr_ctx *ctx, uint8_t *pixels);       // ... and ships them to host `pixels`; blocks
int rxr_group_render_download(rxr_ctx *ctx, uint8_t *pixels);
int rxr_group_synchronize(rxr_ctx *ctx);
int rxr_group_get_stats(rxr_ctx *ctx, rxr_stats *out);
int rxr_group_render_stripes_batch(rxr_ctx *ctx, uint32_t first, uint32_t stride, uint32_t n_frames, void *dev_pixels, size_t frame_stride_bytes,
                                   void *hip_stream);

// rxr_jit.hip: program sets compiled at run time
bool rxr_jit_generate(const std::vector<uint32_t> &code, const std::vector<DevProgram> &progs, std::string &src, std::string &why);
bool rxr_jit_compile(const std::string &gen, const std::string &arch, int level, std::vector<char> &obj, double &seconds, std::string &err);
int rxr_jit_build(rxr_ctx *ctx, const std::vector<uint32_t> &code, const std::vector<DevProgram> &progs);
void rxr_jit_drop(rxr_ctx *ctx);
bool rxr_jit_launch(rxr_ctx *ctx, const RasterParams *P, hipStream_t s);

// kernel durations of one sampled render from its slot: the sum over its set-up kernels and the raster kernel, microseconds
static inline bool rxr_prof_slot_us(const ProfSlot &p, float *setup_us, float *raster_us) {
    float a = 0.0f, b = 0.0f;
    for (uint32_t k = 0; k < p.n; ++k) {
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, p.ev[2u * k], p.ev[2u * k + 1u]) != hipSuccess) return false;
        (k < p.raster_first ? a : b) += ms * 1000.0f;
    }
    *setup_us = a;
    *raster_us = b;
    return true;
}
