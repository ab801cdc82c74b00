// rusterix_host.hpp -- C++ mirror of the reference's host-side API for the rasterizer path.
//
// In a real deployment this layer is Rusterix itself (Rust): Scene / Batch2D / Batch3D / Assets /
// Rasterizer with `Rasterizer::setup(..).rasterize(&mut scene, pixels, w, h, tile_size, &assets)`.
// No Rust toolchain exists in this image, so the same surface is mirrored in C++ with the same
// names, argument meaning and error behaviour.  What stays on the host is exactly what the
// north-star keeps there: scene set-up, Scene::project (batch projection + near clipping) and the
// Edges precompute.  Everything after `scene.project(..)` crosses the C ABI of include/rxr.h.
//
// Storage is flat (std::vector<float> / uint32_t / rxr_edges) so that a projected batch can be handed
// to rxr_batch3d / rxr_batch2d without repacking.
//
// All citations are file:line under /root/reference/.
#pragma once
#include <cstdint>
#include <map>
#include <set>
#include <string>
#include <functional>
#include <new>
#include <vector>

#include "../../../include/rusterix_vek.hpp"
#include "../../../include/rxr.h"

namespace rusterix {

// Allocator of the projected arrays: page-locked, device-readable memory from the device library (rxr_alloc_pinned) while that
// works, ordinary memory otherwise (no GPU: the CPU tests project with this mirror too).  Large blocks only -- a page-locked block
// costs a system call, and small scenes are not streamed anyway.  all_pinned() tells Rasterizer::upload whether the promise of
// rxr_stream_begin_pinned can be made: false as soon as ONE block of at least the threshold had to come from malloc.
struct PinnedPool {
    static constexpr size_t threshold = 8u << 10;
    static bool &any_unpinned() {
        static bool v = false;
        return v;
    }
    static void *take(size_t bytes, bool &pinned);
    static void give(void *p, bool pinned);
};
template <class T> struct PinnedAlloc {
    using value_type = T;
    PinnedAlloc() = default;
    template <class U> PinnedAlloc(const PinnedAlloc<U> &) {}
    T *allocate(size_t n) {
        // one header word in front of the block says where it came from
        const size_t bytes = n * sizeof(T) + 64;
        bool pinned = false;
        uint8_t *raw = (uint8_t *)PinnedPool::take(bytes, pinned);
        if (!raw) throw std::bad_alloc();
        *(uint64_t *)raw = pinned ? 1u : 0u;
        return (T *)(raw + 64);
    }
    void deallocate(T *p, size_t) {
        uint8_t *raw = (uint8_t *)p - 64;
        PinnedPool::give(raw, *(uint64_t *)raw != 0u);
    }
    template <class U> bool operator==(const PinnedAlloc<U> &) const { return true; }
    template <class U> bool operator!=(const PinnedAlloc<U> &) const { return false; }
};
template <class T> using PinnedVec = std::vector<T, PinnedAlloc<T>>;
// is the vector's CURRENT buffer page-locked?  (the allocator's header word in front of it)
// (a vector without a buffer -- a batch that was always rejected -- has nothing the device could read: fine)
template <class T> inline bool is_pinned(const PinnedVec<T> &v) { return v.capacity() == 0 || *(const uint64_t *)((const uint8_t *)v.data() - 64) == 1u; }


using rvek::Mat3;
using rvek::Mat4;
using rvek::Vec2;
using rvek::Vec3;
using rvek::Vec4;

using Pixel = uint8_t[4];

enum class CullMode { Off = 0, Front = 1, Back = 2 };  // src/batch/mod.rs:17-26

// src/map/pixelsource.rs:23-37
struct PixelSource {
    uint32_t kind = RXR_SOURCE_OTHER;  // RXR_SOURCE_*, or RXR_HOST_SOURCE_ENTITY_TILE / _ITEM_TILE (index = id, seq = sequence index)
    uint32_t index = 0;
    uint8_t pixel[4] = {0, 0, 0, 0};
    uint32_t seq = 0;
    static PixelSource EntityTile(uint32_t id, uint32_t index) { PixelSource s; s.kind = RXR_HOST_SOURCE_ENTITY_TILE; s.index = id; s.seq = index; return s; }
    static PixelSource ItemTile(uint32_t id, uint32_t index) { PixelSource s; s.kind = RXR_HOST_SOURCE_ITEM_TILE; s.index = id; s.seq = index; return s; }
    static PixelSource Off() { return {}; }
    static PixelSource StaticTileIndex(uint16_t i) { PixelSource s; s.kind = RXR_SOURCE_STATIC_TILE; s.index = i; return s; }
    static PixelSource DynamicTileIndex(uint16_t i) { PixelSource s; s.kind = RXR_SOURCE_DYNAMIC_TILE; s.index = i; return s; }
    static PixelSource Terrain() { PixelSource s; s.kind = RXR_SOURCE_TERRAIN; return s; }
    static PixelSource FromPixel(const uint8_t p[4]) { PixelSource s; s.kind = RXR_SOURCE_PIXEL; for (int i = 0; i < 4; ++i) s.pixel[i] = p[i]; return s; }
};

// src/texture.rs:46-54
struct Texture {
    std::vector<uint8_t> data;
    uint32_t width = 0, height = 0;
};
// src/map/tile.rs
struct Tile {
    std::vector<Texture> textures;
};
// src/server/assets.rs
uint64_t next_generation();  // process-wide unique stamps (never reused, unlike addresses)
// rusteria TexStorage (rusteria/src/textures/mod.rs:10-15): width * height RGB f32
struct Pattern {
    uint32_t width = 0, height = 0;
    std::vector<float> rgb;
};

struct Assets {
    std::vector<Tile> tile_list;
    // src/server/assets.rs:28, :34 (FxHashMap<u32, IndexMap<String, Tile>>): id -> sequence tiles in insertion order, which is all
    // the raster loops use (`.get(&id)`, `.get_index(i)`, rasterizer.rs:1140-1187).  Rasterizer::upload resolves
    // EntityTile / ItemTile sources against these and ships the tiles with the dynamic textures.
    std::map<uint32_t, std::vector<Tile>> entity_tiles, item_tiles;
    uint64_t generation = next_generation();  // re-stamped on every mutation; lets the rasterizer skip texture re-uploads
    Assets &textures(std::vector<Tile> tiles) { tile_list = std::move(tiles); generation = next_generation(); return *this; }
    // what a Rusteria program reads besides its own code: assets.palette (ThePalette.colors) and rusteria's
    // process-global pattern banks (rusteria/src/textures/patterns.rs), which the caller hands over as data
    std::vector<Pattern> patterns, patterns_normal;
    std::vector<float> palette_rgb;        // [n][3]
    std::vector<uint8_t> palette_present;  // [n]
    uint64_t shader_env_generation = next_generation();
};

// rusteria::Program (rusteria/src/node/program.rs:7-29): user functions as NodeOp trees in the word
// serialisation of include/rxr.h (there is no Rusteria parser / compiler on this side)
struct Program {
    uint32_t globals = 0;
    int32_t shade_index = -1;
    uint32_t shade_locals = 0;
    std::vector<std::vector<uint32_t>> user_functions;
};

// src/rect.rs
struct Rect {
    float x = 0, y = 0, width = 0, height = 0;
};

using CompiledLight = rxr_light;  // src/map/light.rs:456-477

// src/batch/batch3d.rs:15-78
class Batch3D {
public:
    std::vector<float> vertices;           // [n][4]
    std::vector<uint32_t> indices;         // [m][3]
    std::vector<float> uvs;                // [n][2]
    std::vector<float> normals;            // [n][3] or empty
    // what clip_and_project produces lives in page-locked memory when a device is there (PinnedAlloc below): the library's streaming
    // hand-over then lets the GPU read it in place (rxr_stream_begin_pinned) instead of copying it into a staging buffer first
    PinnedVec<float> projected_vertices;    // [n'][4]
    PinnedVec<uint32_t> clipped_indices;    // [m'][3]
    PinnedVec<float> clipped_uvs;           // [n'][2]
    PinnedVec<float> clipped_normals;       // [n'][3]
    PinnedVec<rxr_edges> edges;             // [m']
    PinnedVec<uint32_t> edge_visible;       // [m']: edges[t].visible as a word -- what travels instead of `edges` when the device builds the
                                            // records itself (device_edges(), rxr_batch3d.edges == NULL, ABI 5)
    bool has_bounding_box = false;
    Rect bounding_box;
    uint32_t repeat_mode_ = RXR_REPEAT_CLAMP_XY;
    CullMode cull_mode_ = CullMode::Off;
    PixelSource source_;
    Mat4 transform_3d = Mat4::identity();
    bool receives_light_ = true;
    Vec3 ambient_color_{0, 0, 0};
    int shader_ = -1;
    bool has_profile_id = false;
    uint32_t profile_id_ = 0;
    // Option<Material> (src/shapestack/material.rs:115-121; only the path tracer reads it): role and modifier as their to_u8 / from_u8 numbers
    bool has_material = false;
    uint32_t material_role = 0, material_modifier = 0;
    float material_value = 1.0f;
    // geometry stamp for the device-projection cache: re-stamped by every mutator below; code that edits the
    // public vectors directly calls touch().  Copies keep the stamp (same content).
    uint64_t geometry_stamp = next_generation();
    void touch() { geometry_stamp = next_generation(); }

    static Batch3D empty() { return Batch3D(); }
    static Batch3D make(const float *verts4, size_t nv, const uint32_t *idx3, size_t nt, const float *uvs2);  // Batch3D::new, :109-137
    static Batch3D from_box(float x, float y, float z, float w, float h, float d);                          // :140-229
    static Batch3D from_obj(const std::string &text);                                                      // :407-419 + src/wavefront.rs
    void add(const float *verts4, size_t nv, const uint32_t *idx3, size_t nt, const float *uvs2);          // :238-253
    void compute_vertex_normals();                                                                          // :771-809
    // :482-740.  Returns false where the reference panics (normals shorter than vertices, :605-607).
    bool clip_and_project(const Mat4 &view, const Mat4 &proj, float viewport_width, float viewport_height);

    size_t vertex_count() const { return vertices.size() / 4; }
    size_t triangle_count() const { return indices.size() / 3; }
};

// src/batch/batch2d.rs:10-52
class Batch2D {
public:
    uint32_t mode_ = RXR_MODE_TRIANGLES;
    std::vector<float> vertices;           // [n][2]
    std::vector<uint32_t> indices;         // [m][3]
    std::vector<float> uvs;                // [n][2]
    std::vector<float> projected_vertices; // [n][2]
    std::vector<rxr_edges> edges;          // [m]
    bool has_bounding_box = false;
    Rect bounding_box;
    uint32_t repeat_mode_ = RXR_REPEAT_CLAMP_XY;
    PixelSource source_;
    bool receives_light_ = true;
    int shader_ = -1;

    static Batch2D make(const float *verts2, size_t nv, const uint32_t *idx3, size_t nt, const float *uvs2);  // :83-106
    static Batch2D from_rectangle(float x, float y, float w, float h);                                       // :109-127
    void project(const Mat3 *matrix);                                                                         // :373-425
};

// src/map/mini.rs (fields the raster loops read)
struct MapMini {
    std::vector<rxr_occluder> occluded_sectors;
    std::vector<rxr_linedef> linedefs;
};

// src/chunk.rs (fields the raster loops read)
struct Chunk {
    std::vector<Batch3D> batches3d_opacity, batches3d;
    std::vector<Batch2D> batches2d;
    std::vector<CompiledLight> lights;
    std::vector<rxr_occluder> occluded_sectors;
    std::vector<Program> shaders;  // src/chunk.rs:51
    // Option<..> fields as 0- or 1-element vectors / presence flags
    std::vector<Batch2D> terrain_batch2d;           // src/chunk.rs:34
    std::vector<Batch3D> terrain_batch3d;           // :35
    bool has_terrain_texture = false;               // :36
    Texture terrain_texture;
    int32_t origin[2] = {0, 0};                     // :25
    int32_t size = 1;                               // :26
    std::vector<Texture> shader_textures;           // :53, Vec<Option<Texture>>
    std::vector<uint8_t> shader_texture_present;
    // Resident chunk textures (Scene::resident_chunk_textures): whether the context's registration still holds this chunk's textures is
    // decided by this stamp, not by their bytes.  Every mirror method that assigns terrain_texture or shader_textures re-stamps it; code
    // that writes the fields directly calls touch_textures().
    uint64_t textures_generation = next_generation();
    void touch_textures() { textures_generation = next_generation(); }
    // Terrain::rebuild_chunk_textures' fast path wrote the device's slot and left terrain_texture.data as it was: Scene::refresh_chunk_textures
    // (which the C API's reader calls) brings the bytes back
    bool terrain_texture_stale = false;
    int32_t terrain_slot = -1;                      // the texture's slot in the registration (Rasterizer::upload)
    uint64_t slot_registration = 0;                 // ... and which registration that was (chunk_texture_registrations() when it was made)
};

// src/scene.rs:8-50
class Scene {
public:
    uint32_t background = RXR_BG_NONE;  // Option<Box<dyn Shader>>: VGrayGradientShader and GridShader are evaluated on the device
    float background_grid[4] = {30.0f, 2.0f, 0.0f, 0.0f};  // GridShader: grid_size, subdivisions, offset (shader/grid.rs:12-16)
    std::vector<CompiledLight> lights, dynamic_lights;
    std::vector<Batch3D> d3_static, d3_dynamic, d3_overlay;
    std::vector<Batch2D> d2_static, d2_dynamic;
    std::vector<Tile> dynamic_textures;
    uint64_t dynamic_textures_generation = next_generation();
    size_t animation_frame = 1;
    std::vector<Chunk> chunks;
    std::vector<Program> shaders;  // src/scene.rs:43
    uint64_t shaders_generation = next_generation();
    // scene.add_shader (src/scene.rs:104-134) minus parse + compile; returns the shader index
    size_t add_program(Program p) { shaders.push_back(std::move(p)); shaders_generation = next_generation(); return shaders.size() - 1; }

    // src/scene.rs:154-200.  false where the reference panics.
    // on_projected3d (optional): called on the projecting thread right after clip_and_project of 3D batch `index` (index = the batch's
    // position in the submission order of Rasterizer::upload's frame) -- the hook of the streaming hand-over (rxr_stream_batch3d)
    bool project(const Mat3 *m2d, const Mat4 &view, const Mat4 &proj, float width, float height,
                 const std::function<void(size_t index, const Batch3D &)> *on_projected3d = nullptr);
    // the 3D batches in submission order (what project() walks and Rasterizer::upload flattens)
    std::vector<const Batch3D *> batches3d_in_order() const;
    // the 2D half only (src/scene.rs:163-187); used when the 3D half runs on the device
    void project_2d(const Mat3 *m2d);
    // src/scene.rs:216-276 for n rays at once, on the device (rxr_intersect, include/rxr.h): registers the 3D batches with
    // rxr_set_meshes unless the context already holds this geometry, whether or not device projection is on.  `mesh` indexes the
    // batches in the order of batches3d_in_order().  Returns RXR_OK or a negative rxr_status; there is no CPU path.
    int intersect(const float *origins, const float *dirs, uint32_t n, uint32_t flags, float *t, uint32_t *mesh, uint32_t *triangle,
                  float *hitpoint, float *uv, float *normal) const;
    // Rusteria::shade + RenderBuffer::as_rgba_bytes (rusteria/src/lib.rs:161-210, renderbuffer.rs:88-107) on the device (rxr_bake_shaders,
    // include/rxr.h): n bakes of width x height; programs[i] indexes scene.shaders followed by every chunk's shaders in chunk order (the
    // table Rasterizer::upload makes resident, which this call makes resident too when it is not).  Returns RXR_OK or a negative rxr_status.
    int bake_shaders(const Assets &assets, const uint32_t *programs, uint32_t n, uint32_t width, uint32_t height, float *pixels, uint8_t *rgba) const;
    // Chunk::add_shader (src/chunk.rs:84-131) behind the compiler: pushes the program onto chunks[chunk].shaders and the 64 x 64 texture
    // baked from it on the device onto shader_textures (None for a program without `shade`, which is not baked); the bytes are host memory.
    // Returns the shader's index in the chunk or a negative rxr_status (a program the device cannot bake is not added).
    int chunk_add_shader(size_t chunk, Program program, const Assets &assets);
    // A height stroke's way to the frame without crossing PCIe: the meshes of the terrain's chunks coords[i] = (cx, cy) are built on the
    // device (rxr_terrain_meshes_to, into device scratch) and written over the registered geometry of chunks[chunks_[i]]'s single
    // terrain_batch3d in place (rxr_update_meshes_to on the same stream, include/rxr.h).  Needs device projection (else
    // RXR_ERR_UNSUPPORTED).  Returns
    //   0  the fast path: the context's meshes are the new ones.  THE HOST Batch3D ARRAYS OF THOSE BATCHES ARE LEFT AS THEY WERE: their
    //      geometry_stamp, and with it the registration's fingerprints, are unchanged, so the next upload sends matrices only and does
    //      not overwrite the device's newer geometry with the stale host copy.  (Anything else that re-registers the scene -- another
    //      batch touched, a material changed -- does send the stale copy: refresh these batches from Terrain::build_meshes first.)
    //   1  the fallback: the update was refused (RXR_ERR_INVALID: a cell was added or removed, so the counts changed), or the context
    //      does not hold a device-projection registration of this scene's geometry yet (the next upload registers from the host arrays,
    //      which must then be the new ones), or the context is a multi-device one.  Terrain::build_meshes to the host, the batches'
    //      geometry replaced and touch()ed: the next upload registers again.
    //   a negative rxr_status otherwise.
    int rebuild_terrain_meshes(const class Terrain &terrain, const int32_t *coords, uint32_t n, const uint32_t *chunks_);
    // the same for the GENERATED terrain: chunk chunks_[i]'s batches3d -- all of them; terrain_batch3d is an Option and holds one --
    // are the tile groups of boxes[i] in ascending tile slot (TerrainGenerator::generate_tile_meshes), at most max_groups of them.  Held registration: rxr_generated_tile_meshes_to ->
    // rxr_vertex_normals_to -> rxr_update_meshes_to on the context's stream, returns 0.  Refused by the update (counts changed), or
    // no registration held: the batches' geometry is replaced on the host (the CPU partition, Batch3D::compute_vertex_normals),
    // returns 1, and the next upload registers the scene again.  A chunk whose number of groups changed is RXR_ERR_INVALID.
    int rebuild_generated_tile_meshes(const class TerrainGenerator &gen, const float *boxes, uint32_t n, const uint32_t *chunks_, uint32_t max_groups);
    // src/scene.rs:203-215: Batch3D::compute_vertex_normals for every batch of d3_static / d3_dynamic.  `route`:
    //   NORMALS_CPU     batch after batch on the calling thread (the reference's loop; where it panics -- an index out of range -- so does this)
    //   NORMALS_POOL    one batch a task over the host's worker pool, as the reference's par_iter_mut (what tools/vertex_normals_bench.py
    //                   measures the device against)
    //   NORMALS_DEVICE  the batches packed into ONE strided call of rxr_vertex_normals (include/rxr.h; strides = the largest counts)
    //                   and the normals written back into the batches: the same bits.  A batch with an index out of range is refused
    //                   (RXR_ERR_INVALID, nothing written).
    // Every batch is touch()ed.  Returns RXR_OK or a negative rxr_status.
    enum : int { NORMALS_CPU = 0, NORMALS_DEVICE = 1, NORMALS_POOL = 2 };
    int compute_static_normals(int route = NORMALS_CPU) { return compute_normals(d3_static, route); }
    int compute_dynamic_normals(int route = NORMALS_CPU) { return compute_normals(d3_dynamic, route); }
    static int compute_normals(std::vector<Batch3D> &batches, int route);
    // Opt-in, off by default: Rasterizer::upload registers the chunks' terrain and shader textures once (rxr_set_chunk_textures,
    // include/rxr.h) and sends frames without them, instead of handing every texel over with every frame.  The registration is made again
    // when a chunk's textures_generation differs from the one registered, when chunks were added or removed, or when another scene's
    // registration is held; a scene with the option off removes a registration it finds.
    bool resident_chunk_textures = false;
    // Opt-in, off by default: when rxr_update_meshes_to refuses rebuild_terrain_meshes / rebuild_generated_tile_meshes because counts
    // changed, the same device arrays go through rxr_resize_meshes_to on the same stream (include/rxr.h) and the call returns
    //   2  resized on the device: the context's registration is the new one, the named batches' host arrays take the new COUNTS
    //      (their contents are stale, as after a return of 0; every index is 0) and the registration's fingerprints follow, so the
    //      next upload sends matrices only.  The resident frame, the pick records and the trace scene are gone, as after a registration.
    // instead of 1.  A chunk whose number of groups changed is still RXR_ERR_INVALID.  Off: every call behaves as described above.
    bool resize_meshes = false;
    // Opt-in, off by default (RXR_RAY_ACCEL_OFF): intersect() and Tracer::trace hand the mode to the context (rxr_set_ray_accel,
    // include/rxr.h), which then culls its many-ray queries with a box tree built on the device over the registered triangles.  The
    // results are the same words; RXR_RAY_ACCEL_COUNT also counts the ray-triangle tests (ray_accel_info).
    uint32_t ray_accel = RXR_RAY_ACCEL_OFF;
    // rxr_ray_accel_info of the context: RXR_RAY_ACCEL_INFO_WORDS words.  RXR_OK or a negative rxr_status.
    int ray_accel_info(uint64_t *out) const;
    // Opt-in, RXR_RAY_WAVE_OFF by default, on top of ray_accel and handed over next to it (rxr_set_ray_wave, include/rxr.h): with the
    // tree on, RXR_RAY_WAVE_ON sends the batches rxr_ray_wave_takes() names through it a wave per ray, RXR_RAY_WAVE_FORCE every batch.
    // The results are the same words.
    uint32_t ray_wave = RXR_RAY_WAVE_OFF;
    // rxr_ray_wave_info of the context: RXR_RAY_WAVE_INFO_WORDS words.  RXR_OK or a negative rxr_status.
    int ray_wave_info(uint64_t *out) const;
    // Opt-in, RXR_RAY_REFRESH_FULL by default: what an rxr_update_meshes on the shared context leaves for the next intersect() or
    // Tracer::trace -- handed over next to ray_accel (rxr_set_ray_refresh, include/rxr.h).  RXR_RAY_REFRESH_RANGED rewrites only the
    // updated meshes' records and refits the tree; the results are the same words.
    uint32_t ray_refresh = RXR_RAY_REFRESH_FULL;
    // rxr_ray_refresh_info of the context: RXR_RAY_REFRESH_INFO_WORDS words.  RXR_OK or a negative rxr_status.
    int ray_refresh_info(uint64_t *out) const;
    // the host copies of the textures the device holds newer bytes of (Chunk::terrain_texture_stale), read back through
    // rxr_read_chunk_texture.  RXR_OK, or RXR_ERR_INVALID when the context no longer holds this scene's registration (another scene was
    // uploaded in between: the bytes are gone, build the chunk again).
    int refresh_chunk_textures();
};
// src/tracer/buffer.rs: linear RGBA f32, [height][width][4], and the number of frames averaged into it
class AccumBuffer {
public:
    size_t width = 0, height = 0, frame = 0;
    std::vector<float> pixels;
    AccumBuffer(size_t w, size_t h) : width(w), height(h), pixels(w * h * 4, 0.0f) {}
    void reset() { frame = 0; }
    std::vector<uint8_t> to_u8_vec() const;   // :78-91, on the host (std::pow)
};

// src/tracer/trace.rs: the path tracer over a Scene.  trace() runs n_frames samples a pixel on the device (rxr_set_trace_scene +
// rxr_trace, include/rxr.h): it registers the scene's textures and 3D batches as Rasterizer::upload and Scene::intersect do, hands
// over every batch's material, scene.lights chained with scene.dynamic_lights and the chunks' origin and size, and advances
// accum.frame.  `camera`: RXR_TRACE_CAMERA_* and the RXR_TRACE_CAMERA_FLOATS floats the camera's create_ray computes before it looks
// at the pixel.  cpu == true: the same loop on host threads (threads == 0: one per core, at most 16) with the library's generator
// (rxr_trace_rand) and sRGB table (rxr_trace_srgb_table), no device needed -- every float equals the device's until a path's first
// diffuse bounce, where cos and sin are the host's.  A terrain-sourced batch samples the chunk's host terrain_texture there; on the
// device it needs the registration of Scene::resident_chunk_textures (else RXR_ERR_UNSUPPORTED).  A miss adds nothing (no render
// graph); `background` is kept for API parity only, as in the reference, where nothing reads it.  Returns RXR_OK or a negative rxr_status.
class Tracer {
public:
    uint32_t sample_mode = RXR_SAMPLE_NEAREST;
    bool has_background = false;
    uint8_t background[4] = {0, 0, 0, 0};
    int trace(uint32_t camera_kind, const float *camera, const Scene &scene, AccumBuffer &accum, const Assets &assets, uint32_t n_frames,
              uint32_t seed, uint32_t bounces = RXR_TRACE_MAX_BOUNCES, bool cpu = false, unsigned threads = 0) const;
};

// how many times Rasterizer::upload has called rxr_set_chunk_textures with textures (tests: an unchanged scene registers nothing)
uint64_t chunk_texture_registrations();
// how many times a Terrain has called rxr_set_terrain_heights / rxr_set_terrain_flatten (tests: unchanged heights and ops register nothing)
uint64_t terrain_height_registrations();
uint64_t terrain_flatten_registrations();

// src/terrain/mod.rs, src/terrain/chunk.rs: what Terrain::bake_chunk reads -- `sources` and `blend_modes` per cell, behind the asset
// lookup: a cell's source is the texture sample_source would sample (tile.textures.first()), or a source without one (a PixelSource
// that is neither TileId nor MaterialId, or whose lookup fails: the checker, as for no source at all)
class Terrain {
public:
    struct Cell {
        bool has_source = false;
        int32_t texture = -1;                         // index into `textures`
        uint32_t blend = RXR_TERRAIN_BLEND_NONE;      // kind | radius << 8 (include/rxr.h)
        float offset[2] = {0.0f, 0.0f};
    };
    float scale[2] = {1.0f, 1.0f};                    // :22
    int32_t chunk_size = 16;                          // :24
    std::map<std::pair<int32_t, int32_t>, Cell> cells;            // keyed (x, y), world tile coordinates
    std::set<std::pair<int32_t, int32_t>> chunks;                 // Terrain.chunks' keys (get_or_create_chunk, :43-51)
    std::vector<Texture> textures;                                // de-duplicated by content
    uint64_t generation = next_generation();                      // re-stamped by every mutator; code that edits the fields calls touch()
    void touch() { generation = next_generation(); }

    void set_source(int32_t x, int32_t y, const Texture *texture);   // :133-137; nullptr: a source without a texture
    void set_blend_mode(int32_t x, int32_t y, uint32_t kind, uint32_t radius, float offset_x, float offset_y);   // :127-130
    // Terrain::bake_chunk (:318-369) on the CPU, rows over the host's worker pool as the reference's run over rayon: side * side * 4
    // bytes, side = chunk_size * pixels_per_tile.  RXR_OK, or RXR_ERR_INVALID for a scale that is not finite and > 0, chunk_size < 1 or
    // pixels_per_tile < 1.  No bound on the radius.
    int bake_chunk(int32_t cx, int32_t cy, int32_t pixels_per_tile, std::vector<uint8_t> &rgba) const;
    // the same for n chunks on the device (rxr_set_terrain when the terrain changed since it was registered, then rxr_bake_terrain,
    // include/rxr.h): n * side * side * 4 bytes.  RXR_OK or a negative rxr_status; there is no fall-back to the CPU.
    int bake_chunks(const int32_t *coords, uint32_t n, int32_t pixels_per_tile, uint8_t *rgba) const;
    // Terrain::build_chunk_at (:372-399) with modifiers == false: bakes on the device and sets chunk.terrain_texture -- unless the
    // terrain has no chunk at `coord`, as in the reference.  RXR_OK or a negative rxr_status.
    int build_chunk_at(int32_t cx, int32_t cy, int32_t pixels_per_tile, Chunk &chunk) const;
    // A texture stroke's way to the frame without crossing PCIe: the textures of the terrain's chunks coords[i] = (cx, cy) are baked on the
    // device (rxr_bake_terrain_to, into device scratch) and written over the slots of scene.chunks[chunks_[i]]'s terrain textures on the
    // same stream (rxr_update_chunk_textures_to, include/rxr.h).  Returns
    //   0  the fast path.  The chunks' host terrain_texture bytes are left as they were and marked stale (Chunk::terrain_texture_stale);
    //      the registration counts as current, so the next upload sends no texel.
    //   1  the fallback, build_chunk_at per chunk (the next upload registers again): scene.resident_chunk_textures is off, the context
    //      does not hold this scene's registration, it is a multi-device one, a chunk has no terrain texture yet, its side is not
    //      chunk_size * pixels_per_tile, the terrain has no chunk at a coordinate, or a chunk is named twice.
    //   a negative rxr_status otherwise.
    int rebuild_chunk_textures(Scene &scene, const int32_t *coords, uint32_t n, const uint32_t *chunks_, int32_t pixels_per_tile) const;
    // the cell list of rxr_set_terrain
    void flatten(std::vector<int32_t> &xy, std::vector<int32_t> &texture, std::vector<uint32_t> &blend, std::vector<float> &offset) const;

    // ---- heights and the editor's pick (:82-95, :148-173, :427-479) ----
    // TerrainHit (src/terrain/mod.rs:11-16); `t` is t_hit, which the reference computes and drops
    struct Hit {
        float t = 0.0f;
        float world_pos[3] = {0.0f, 0.0f, 0.0f};
        int32_t grid_pos[2] = {0, 0};
        float height = 0.0f;
    };
    std::map<std::pair<int32_t, int32_t>, float> heights;         // what get_height returns per cell, keyed (x, y)
    uint64_t heights_generation = next_generation();              // re-stamped by set_height alone: a height edit does not re-register the bake's terrain
    void set_height(int32_t x, int32_t y, float height);          // :92-95
    void remove_height(int32_t x, int32_t y);                     // :98-104 (an emptied chunk stays listed)
    float get_height(int32_t x, int32_t y) const;                 // :82-89: 0.0 for a cell that does not exist
    float sample_height(float x, float y) const;                  // :148-152
    float sample_height_bilinear(float x, float y) const;         // :155-173
    // Terrain::ray_terrain_hit (:427-479) on the CPU, a plain transcription: false for None
    bool ray_terrain_hit(const float origin[3], const float dir[3], float max_distance, Hit &hit) const;
    // the same for n rays on the device (rxr_set_terrain_heights when the heights changed since they were registered, then
    // rxr_terrain_hits, include/rxr.h); t, world_pos and grid_pos may be null.  RXR_OK or a negative rxr_status; there is no fall-back
    // to the CPU.
    int ray_terrain_hits(const float *origins, const float *dirs, uint32_t n, float max_distance, uint32_t *hit, float *t, float *world_pos,
                         int32_t *grid_pos) const;
    // the same on the CPU over the host's worker pool (what tools/terrain_hit_bench.py measures the device against)
    void ray_terrain_hits_cpu(const float *origins, const float *dirs, uint32_t n, float max_distance, uint32_t *hit, float *t, float *world_pos,
                              int32_t *grid_pos) const;
    // the cell list of rxr_set_terrain_heights
    void flatten_heights(std::vector<int32_t> &xy, std::vector<float> &height) const;

    // ---- the chunk mesh (src/terrain/chunk.rs:253-297) ----
    // TerrainChunk::build_mesh for chunk (cx, cy) on the CPU, the plain dictionary transcription with the cells visited in ascending
    // (ly, lx) (the reference's hash order is not an order: DESIGN.md section 13): a cell is present iff it is a key of `heights`;
    // source Terrain, uvs zero, normals from compute_vertex_normals.  An empty batch for a chunk without a present cell.
    Batch3D build_mesh(int32_t cx, int32_t cy) const;
    // the same for n chunks on the device (rxr_set_terrain_heights when the heights changed since they were registered, then
    // rxr_terrain_meshes, include/rxr.h): out[i] is the batch of coords[i].  RXR_OK or a negative rxr_status; there is no fall-back
    // to the CPU.
    int build_meshes(const int32_t *coords, uint32_t n, std::vector<Batch3D> &out) const;
    // build_mesh for n chunks over the host's worker pool (what tools/terrain_mesh_bench.py measures the device against)
    void build_meshes_cpu(const int32_t *coords, uint32_t n, std::vector<Batch3D> &out) const;

    // ---- processed_heights: the Height pass of TerrainChunk::process_batch_modifiers (src/terrain/chunk.rs:144-208) ----
    // One Flatten node applied to one sector or to one group of linedefs, as rxr_set_terrain_flatten takes it (include/rxr.h):
    // `records` holds RXR_TERRAIN_FLATTEN_RECORD_FLOATS floats an edge or segment.  The list's order is the caller's.
    struct FlattenOp {
        uint32_t kind = RXR_TERRAIN_FLATTEN_SECTOR;
        float bevel = 0.5f, floor_height = 0.0f;
        float box[4] = {0.0f, 0.0f, 0.0f, 0.0f};      // the sector's bounding_box: min x, min y, max x, max y
        std::vector<float> records;
    };
    std::vector<FlattenOp> flatten_ops;
    uint64_t flatten_generation = next_generation();              // code that edits flatten_ops calls touch_flatten()
    void touch_flatten() { flatten_generation = next_generation(); }
    // the list from the arrays of rxr_set_terrain_flatten; RXR_OK, or what rxr_check_terrain_flatten refuses (nothing changes then)
    int set_flatten_ops(const uint32_t *kinds, const float *params, const uint32_t *ranges, uint32_t n_ops, const float *records, uint32_t n_records);
    // ... and back: every op's records one after the other
    void flatten_op_arrays(std::vector<uint32_t> &kinds, std::vector<float> &params, std::vector<uint32_t> &ranges, std::vector<float> &records) const;
    // The Height pass for n chunks on the CPU over the host's worker pool, a chunk a task: the plain dictionary transcription -- the
    // reference's loops over each op's integer range, inserts into a map, nothing hoisted; a sector's range is clipped to the chunk's
    // cells +- 130 before it is walked, which drops no insert (every insert sits behind chunk_bbox.contains, and `x as f32` is within
    // 64 of x up to 2^30).  heights [n][chunk_size^2] (0.0 for an absent cell) and present, the chunk's own cells row by row, as
    // rxr_flatten_terrain returns them; either may be null.
    void process_heights_cpu(const int32_t *coords, uint32_t n, float *heights, uint8_t *present) const;
    // the same on the device (rxr_set_terrain_heights / rxr_set_terrain_flatten when heights / ops changed since they were
    // registered, then rxr_flatten_terrain).  RXR_OK or a negative rxr_status; there is no fall-back to the CPU.
    int process_heights(const int32_t *coords, uint32_t n, float *heights, uint8_t *present) const;
    // Opt-in, off by default: Scene::rebuild_terrain_meshes and build_meshes build from processed_heights -- the chunks are flattened
    // on the device first (every chunk of the terrain after a registration, which resets the processed grid; else the named ones:
    // rxr_flatten_terrain_to), and the mesh kernels read the processed grid (rxr_set_terrain_height_source for the length of the
    // call), all on the context's stream.
    bool device_modifiers = false;

private:
    friend class Scene;   // (rebuild_terrain_meshes registers the heights)
    int register_flatten(rxr_ctx *ctx) const;   // rxr_set_terrain_flatten unless the context holds this generation
    int flatten_resident(rxr_ctx *ctx, const int32_t *coords, uint32_t n) const;   // device_modifiers: the processed grid made current for these chunks
    void process_chunk_cpu(int32_t cx, int32_t cy, std::map<std::pair<int32_t, int32_t>, float> &processed) const;
    // get_height's answers as a dense grid over the cells' bounding rectangle, rebuilt when heights_generation moved (the CPU march
    // looks a cell up 1500 times a ray)
    struct HeightGrid {
        uint64_t generation = 0;
        int64_t x0 = 0, y0 = 0, w = 0, h = 0;
        std::vector<float> cells;
    };
    mutable HeightGrid height_grid_;
    const HeightGrid &height_grid() const;
    int register_heights(rxr_ctx *ctx) const;   // rxr_set_terrain_heights unless the context holds this generation
};

// src/chunkbuilder/terrain_generator.rs: the height field of the generated 3D terrain, over the lists TerrainGenerator::generate
// collects from the Map (:255-294), flattened as rxr_set_terrain_generator takes them (include/rxr.h).  The CPU functions are plain
// transcriptions (nothing hoisted); the device forms register the lists when they changed.  apply_exclusions is generate_meshes,
// partition_by_tiles generate_tile_meshes (mesh_fix_winding never swaps such a mesh); the blend batches are the caller's.
class TerrainGenerator {
public:
    uint32_t subdivisions = 1;                        // TerrainConfig.subdivisions (:24)
    // the map's sectors of terrain_mode == 1, flattened as rxr_set_terrain_exclusions takes them: a sector's bounding box as the
    // reference computes it and its linedefs' start vertices in linedef order (missing ones skipped, possibly none)
    std::vector<float> excluded_boxes;                // [S][4]: min.x, min.y, max.x, max.y
    std::vector<uint32_t> excluded_vertex_offsets{0u};   // [S + 1]
    std::vector<float> excluded_vertices;             // [V][2]
    std::vector<float> control_points;                // [C][4]: x, y, height, smoothness (config.smoothness's default applied)
    std::vector<float> ridges;                        // [R][4]: height, plateau_width, falloff_distance, falloff_steepness
    std::vector<uint32_t> ridge_edge_offsets{0u};     // [R + 1]
    std::vector<float> ridge_edges;                   // [E][4]: x0, y0, x1, y1
    std::vector<float> linedefs;                      // [L][9]: start, end, start_height, end_height, width, falloff_distance, falloff_steepness
    float map_box[4] = {-100.0f, -100.0f, 100.0f, 100.0f};   // (:273-284)
    uint64_t generation = next_generation();          // code that edits the fields calls touch()
    void touch() { generation = next_generation(); }

    float sample_height_at(float x, float y) const;                     // :57-163
    void sample_normal_at(float x, float y, float normal[3]) const;     // :166-181
    void tile_normal(int32_t tx, int32_t tz, float normal[3]) const;    // :184-189
    std::vector<float> tile_outline_world(int32_t tx, int32_t tz) const;   // :194-242: [4 * max(subdivisions, 1)][3]
    // generate_grid (:460-485): the points [steps_y][steps_x][2]; the steps as the reference's i32 (a negative one: no points)
    std::vector<float> generate_grid(const float box[4], int32_t &steps_x, int32_t &steps_y) const;
    void grid_steps(const float box[4], int32_t &steps_x, int32_t &steps_y) const;   // ... the steps alone: nothing is allocated
    // interpolate_heights (:488-509) for n points [n][2] over the host's worker pool; normals ([n][3]) may be null
    void interpolate_heights(const float *points, size_t n, float *heights, float *normals = nullptr) const;
    // triangulate (:829-879) without exclusions: the indices are a closed form of the counts -- per cell (ix, iy), row by row,
    // (i, i + steps_x, i + 1) and (i + 1, i + steps_x, i + steps_x + 1) with i = iy * steps_x + ix
    static std::vector<uint32_t> triangulate(int32_t steps_x, int32_t steps_y);
    // n boxes [n][4] on the CPU, in the layout of rxr_generated_grids
    void grid_heights_cpu(const float *boxes, uint32_t n, uint32_t stride, uint32_t *counts, float *heights) const;
    // the device forms (rxr_set_terrain_generator when the lists changed since they were registered, then rxr_generated_heights /
    // rxr_generated_grids, include/rxr.h).  RXR_OK or a negative rxr_status; there is no fall-back to the CPU.
    int sample_heights(const float *points, uint32_t n, float *heights, float *normals) const;
    int grid_heights(const float *boxes, uint32_t n, uint32_t stride, uint32_t *counts, float *heights) const;
    // collect_excluded_sectors' test (:438-457): does sector s's box intersect the chunk box as given?
    bool sector_active(uint32_t s, const float box[4]) const;
    bool point_in_sector(float x, float y, uint32_t s) const;   // :891-950
    // apply_exclusions (:747-825) over the grid points [P][2] and their heights, for the sectors `active` in list order: the
    // vertices [..][3] = (x, h, y); shared layout (grid order) when `active` is empty, else three per kept triangle.  The keep
    // flags are computed over the host's worker pool.
    std::vector<float> apply_exclusions(const float *grid, const float *heights, int32_t steps_x, int32_t steps_y, const std::vector<uint32_t> &active) const;
    // n boxes [n][4] on the CPU, in the layout of rxr_generated_meshes: counts [n][4], vertices [n][stride][4] (a box whose layout
    // does not fit the stride gets its counts and no vertices)
    void generate_meshes_cpu(const float *boxes, uint32_t n, uint32_t stride, uint32_t *counts, float *vertices) const;
    // ... and on the device (rxr_set_terrain_generator / rxr_set_terrain_exclusions when the lists changed, then
    // rxr_generated_meshes).  RXR_OK or a negative rxr_status; there is no fall-back to the CPU.
    int generate_meshes(const float *boxes, uint32_t n, uint32_t stride, uint32_t *counts, float *vertices) const;

    // the tile overrides (the reference's FxHashMap<(i32, i32), PixelSource>, every pixel source resolved to a tile SLOT by the
    // caller, slot 0 the default tile), flattened as rxr_set_terrain_tiles takes them.  RXR_OK, or what rxr_check_terrain_tiles
    // refuses (nothing changes then)
    std::vector<int32_t> tile_cells;                  // [N][2]: x, z
    std::vector<uint32_t> tile_slots;                 // [N]
    uint32_t n_tiles = 1;
    std::map<std::pair<int32_t, int32_t>, uint32_t> tile_overrides;   // the same as a map, built by set_tiles (partition_by_tiles looks cells up in it)
    int set_tiles(const int32_t *cells, const uint32_t *slots, uint32_t n, uint32_t n_tiles_);
    // partition_by_tiles (:954-1034) over vertices [V][3], indices [3 T] and uvs [V][2], line by line, the dictionary walk included.
    // The groups come in ascending tile slot (the reference's order is a hash map's)
    struct TileGroup {
        uint32_t slot;
        std::vector<float> vertices, uvs;             // [..][3], [..][2]
        std::vector<uint32_t> indices;
    };
    std::vector<TileGroup> partition_by_tiles(const float *vertices, const uint32_t *indices, size_t n_indices, const float *uvs) const;
    // n boxes [n][4] on the CPU, in the layout of rxr_generated_tile_meshes (a box whose layout does not fit the strides or
    // max_groups gets its box_counts with n_groups = 0 and nothing else): heights and keep flags over the worker pool box by box,
    // then the partition one box a task over the pool
    void generate_tile_meshes_cpu(const float *boxes, uint32_t n, uint32_t max_groups, uint32_t vertex_stride, uint32_t triangle_stride, uint32_t *box_counts,
                                  uint32_t *counts, uint32_t *group_tiles, float *vertices, float *uvs, uint32_t *indices) const;
    // ... and on the device (the three registrations when their lists changed, then rxr_generated_tile_meshes).  RXR_OK or a
    // negative rxr_status; there is no fall-back to the CPU.
    int generate_tile_meshes(const float *boxes, uint32_t n, uint32_t max_groups, uint32_t vertex_stride, uint32_t triangle_stride, uint32_t *box_counts,
                             uint32_t *counts, uint32_t *group_tiles, float *vertices, float *uvs, uint32_t *indices) const;

private:
    friend class Scene;   // (rebuild_generated_tile_meshes registers the lists)
    int register_records(rxr_ctx *ctx) const;
    int register_exclusions(rxr_ctx *ctx) const;
    int register_tiles(rxr_ctx *ctx) const;
};

// src/rasterizer.rs:35-193
class Rasterizer {
public:
    bool d2_active = true, d3_active = true, ignore_background_shader = false;  // RenderMode
    bool has_m2d = false;
    Mat3 projection_matrix_2d = Mat3::identity();
    Mat4 view_matrix = Mat4::identity(), projection_matrix = Mat4::identity();
    Mat4 inverse_view_matrix = Mat4::identity(), inverse_projection_matrix = Mat4::identity();
    float width = 0, height = 0;
    Vec3 camera_pos;
    MapMini mapmini;
    uint32_t sample_mode_ = RXR_SAMPLE_NEAREST;
    uint32_t hash_anim = 0;
    bool has_background_color = false;
    uint8_t background_color[4] = {0, 0, 0, 0};
    // brush_preview: Option<BrushPreview> (src/rasterizer.rs:13-17, :65)
    bool has_brush_preview = false;
    float brush_position[3] = {0, 0, 0};
    float brush_radius = 0.0f, brush_falloff = 0.0f;
    bool has_ambient = false;
    Vec4 ambient_color;
    Vec2 translationd2{0, 0};
    float scaled2 = 1.0f;
    bool preserve_transparency = false;
    float time_ = 0.0f;
    bool has_sun = false;
    Vec3 sun_dir;
    float day_factor = 0.0f;

    static Rasterizer setup(const Mat3 *projection_matrix_2d, const Mat4 &view, const Mat4 &proj);  // :92-152

    // :185-580.  Projects the scene on the host, flattens it and renders it on the GPU through the
    // C ABI.  Returns RXR_OK or a negative rxr_status (the reference panics / has no error path).
    int rasterize(Scene &scene, uint8_t *pixels, size_t width, size_t height, size_t tile_size, const Assets &assets);
    // the same up to and including the host->device hand-over (project + flatten + rxr_upload_frame);
    // callers then drive rxr_render_rows / rxr_render_rows_to themselves (bench, multi-GPU host)
    int upload(Scene &scene, size_t width, size_t height, size_t tile_size, const Assets &assets);
    // :1843-1870 (width / height: those of the last rasterize / upload, 0 before, as in the reference)
    void screen_ray(float x, float y, float origin[3], float dir[3]) const;
};

// the process-wide device context.  Every function that uses it holds one process-wide lock for its whole duration, so
// Rasterizers on several threads are serialised (the reference's are independent values; this layer shares one context).  Device index from RXR_DEVICE, else
// LOCAL_RANK, else 0.
rxr_ctx *context(std::string *error = nullptr);
// device-side projection: when on, Rasterizer::upload registers the object-space
// batches once (rxr_set_meshes) and each frame sends matrices only; Scene::project's 3D half
// (clip_and_project, Edges::new, bounding boxes) then runs on the GPU.  Off by default.
void set_device_projection(bool on);
bool device_projection();
// host-projected 3D batches cross the ABI WITHOUT their Edges records (40 of 124 bytes per triangle over PCIe): a word per triangle says
// `visible`, the device rebuilds a / b / c from the projected vertices it receives anyway (rxr.h, ABI 5).  Default on; RXR_HOST_EDGES=1 or
// set_device_edges(false) sends the records as rounds 1-3 did.
void set_device_edges(bool on);
bool device_edges();
// arithmetic of the 3D light loop (rxr_set_light_math, include/rxr.h): relaxed by default -- point lights within the 1-per-channel
// tolerance of lit 3D fragments; exact = the reference's correctly rounded operations throughout.  Applies from the next frame on.
void set_light_math(bool exact);
bool light_math_exact();
void set_device(int device);
// more than one entry: the context becomes a multi-device one (rxr_create_multi): rasterize() then shards every frame over
// these GPUs inside the library.  A device may be listed more than once (logical members on one GPU).
void set_devices(const int *devices, int n);
const std::string &last_error();

// cameras: src/camera/d3orbit.rs:23-56,186-195 and src/camera/d3firstp.rs:17-42
void orbit_camera(Vec3 center, float distance, float azimuth, float elevation, float fov, float near, float far, float w,
                  float h, Mat4 &view, Mat4 &proj);
void firstp_camera(Vec3 position, Vec3 center, float fov, float near, float far, float w, float h, Mat4 &view, Mat4 &proj);

uint32_t hash_u32(uint32_t seed);  // src/rasterizer.rs:199-207

}  // namespace rusterix
