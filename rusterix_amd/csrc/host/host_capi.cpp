// host_capi.cpp -- extern "C" handle API over the C++ host mirror (rusterix_host.hpp), bound from
// Python by rusterix_amd/binding.py (prefix `rxh_`).  Product code: rasterize() goes through the
// C ABI of include/rxr.h to the HIP kernels; there is no CPU path here.
#include <cstring>
#include <string>
#include <vector>

#include "rusterix_host.hpp"

using namespace rusterix;

namespace {
Mat4 mat4_from(const float *m) {
    Mat4 o{};
    memcpy(o.m, m, sizeof(o.m));
    return o;
}
Tile make_tile(const uint8_t *const *frames, const uint32_t *ws, const uint32_t *hs, uint32_t n) {
    Tile t;
    for (uint32_t i = 0; i < n; ++i) {
        Texture x;
        x.width = ws[i];
        x.height = hs[i];
        x.data.assign(frames[i], frames[i] + (size_t)ws[i] * hs[i] * 4);
        t.textures.push_back(std::move(x));
    }
    return t;
}
std::vector<Batch3D> *list3d(Scene *s, int list, int chunk) {
    const bool chunk_ok = chunk >= 0 && (size_t)chunk < s->chunks.size();
    switch (list) {
        case RXR_LIST_CHUNK_OPACITY: return chunk_ok ? &s->chunks[chunk].batches3d_opacity : nullptr;
        case RXR_LIST_CHUNK: return chunk_ok ? &s->chunks[chunk].batches3d : nullptr;
        case RXR_LIST_CHUNK_TERRAIN: return chunk_ok ? &s->chunks[chunk].terrain_batch3d : nullptr;
        case RXR_LIST_STATIC: return &s->d3_static;
        case RXR_LIST_DYNAMIC: return &s->d3_dynamic;
        case RXR_LIST_OVERLAY: return &s->d3_overlay;
    }
    return nullptr;
}
void set_source(PixelSource &s, uint32_t kind, uint32_t index, const uint8_t *pixel) {
    s.kind = kind;
    s.index = index;
    if (pixel) memcpy(s.pixel, pixel, 4);
}
}  // namespace

extern "C" {

const char *rxh_last_error() { return last_error().c_str(); }
void rxh_set_device(int device) { set_device(device); }
// more than one device: the context becomes a multi-device one (rxr_create_multi); a device may repeat (logical members)
void rxh_set_devices(const int *devices, int n) { set_devices(devices, n); }
// the process-wide rxr_ctx (NULL + rxh_last_error() when no GPU): lets callers drive the split-phase
// ABI (rxr_render_rows_to / rxr_get_stats) after rxh_rasterizer_upload
void *rxh_context() { return context(); }
// device-side projection on/off (rusterix::set_device_projection)
void rxh_set_device_projection(int on) { set_device_projection(on != 0); }
// host-projected batches with (0) or without (1, the default) their Edges records across the ABI (rusterix::set_device_edges)
void rxh_set_device_edges(int on) { set_device_edges(on != 0); }
int rxh_get_device_edges() { return device_edges() ? 1 : 0; }
int rxh_get_device_projection() { return device_projection() ? 1 : 0; }
// light-loop arithmetic (rusterix::set_light_math): 1 = exact, 0 = relaxed (the default)
void rxh_set_light_math_exact(int exact) { set_light_math(exact != 0); }
int rxh_get_light_math_exact() { return light_math_exact() ? 1 : 0; }

// ---- scene ----------------------------------------------------------------------------------------
void *rxh_scene_new() { return new Scene(); }
// Scene::intersect for n rays (rxr_intersect's arrays and flags, include/rxr.h); RXR_OK or a negative rxr_status
int rxh_scene_intersect(void *s, const float *origins, const float *dirs, uint32_t n, uint32_t flags, float *t, uint32_t *mesh,
                        uint32_t *triangle, float *hitpoint, float *uv, float *normal) {
    return ((Scene *)s)->intersect(origins, dirs, n, flags, t, mesh, triangle, hitpoint, uv, normal);
}
// Tracer::trace into an AccumBuffer handle (rusterix_host.hpp): camera_kind + the 14 floats of include/rxr.h; cpu != 0: the host loop
int rxh_scene_trace(void *s, void *assets, void *accum, uint32_t camera_kind, const float *camera, uint32_t sample_mode, uint32_t n_frames,
                    uint32_t seed, uint32_t bounces, int cpu, uint32_t threads) {
    Tracer t;
    t.sample_mode = sample_mode;
    return t.trace(camera_kind, camera, *(Scene *)s, *(AccumBuffer *)accum, *(Assets *)assets, n_frames, seed, bounces, cpu != 0, threads);
}
void *rxh_accum_new(uint32_t width, uint32_t height) { return new AccumBuffer(width, height); }
void rxh_accum_free(void *a) { delete (AccumBuffer *)a; }
float *rxh_accum_pixels(void *a) { return ((AccumBuffer *)a)->pixels.data(); }
uint64_t rxh_accum_frame(void *a) { return ((AccumBuffer *)a)->frame; }
void rxh_accum_set_frame(void *a, uint64_t frame) { ((AccumBuffer *)a)->frame = (size_t)frame; }
void rxh_accum_to_u8(void *a, uint8_t *out) {
    const std::vector<uint8_t> v = ((AccumBuffer *)a)->to_u8_vec();
    memcpy(out, v.data(), v.size());
}
void rxh_scene_free(void *s) { delete (Scene *)s; }
void rxh_scene_set_animation_frame(void *s, uint64_t f) { ((Scene *)s)->animation_frame = (size_t)f; }
void rxh_scene_set_background(void *s, int kind) { ((Scene *)s)->background = (uint32_t)kind; }
// GridShader::set_parameter_f32 / set_parameter_vec2 (shader/grid.rs:19-34)
void rxh_scene_set_background_grid(void *s, float grid_size, float subdivisions, float offset_x, float offset_y) {
    float *g = ((Scene *)s)->background_grid;
    g[0] = grid_size;
    g[1] = subdivisions;
    g[2] = offset_x;
    g[3] = offset_y;
}
void rxh_scene_add_light(void *s, const rxr_light *l, int dynamic) {
    (dynamic ? ((Scene *)s)->dynamic_lights : ((Scene *)s)->lights).push_back(*l);
}
void rxh_scene_add_dynamic_tile(void *s, const uint8_t *const *frames, const uint32_t *ws, const uint32_t *hs, uint32_t n) {
    Scene *sc = (Scene *)s;
    sc->dynamic_textures.push_back(make_tile(frames, ws, hs, n));
    sc->dynamic_textures_generation = next_generation();
}
int rxh_scene_add_chunk(void *s) {
    ((Scene *)s)->chunks.emplace_back();
    return (int)((Scene *)s)->chunks.size() - 1;
}
void rxh_chunk_add_occluder(void *s, int chunk, float minx, float miny, float maxx, float maxy, float occ) {
    ((Scene *)s)->chunks[chunk].occluded_sectors.push_back(rxr_occluder{{minx, miny}, {maxx, maxy}, occ});
}
// chunk.terrain_texture / origin / size (src/chunk.rs:25-36); rgba == NULL: no texture
void rxh_chunk_set_terrain(void *s, int chunk, const uint8_t *rgba, uint32_t w, uint32_t h, int ox, int oy, int size) {
    Chunk &c = ((Scene *)s)->chunks[chunk];
    c.origin[0] = ox;
    c.origin[1] = oy;
    c.size = size;
    c.has_terrain_texture = rgba != nullptr;
    c.terrain_texture_stale = false;
    c.touch_textures();
    if (rgba) {
        c.terrain_texture.width = w;
        c.terrain_texture.height = h;
        c.terrain_texture.data.assign(rgba, rgba + (size_t)w * h * 4);
    }
}
void rxh_chunk_set_terrain_batch2d(void *s, int chunk, void *b) {
    Chunk &c = ((Scene *)s)->chunks[chunk];
    c.terrain_batch2d.clear();
    c.terrain_batch2d.push_back(*(Batch2D *)b);
}
// chunk.shader_textures.push(texture) (src/chunk.rs:129); rgba == NULL pushes None
void rxh_chunk_add_shader_texture(void *s, int chunk, const uint8_t *rgba, uint32_t w, uint32_t h) {
    Chunk &c = ((Scene *)s)->chunks[chunk];
    Texture t;
    if (rgba) {
        t.width = w;
        t.height = h;
        t.data.assign(rgba, rgba + (size_t)w * h * 4);
    }
    c.shader_textures.push_back(std::move(t));
    c.shader_texture_present.push_back(rgba ? 1 : 0);
    c.touch_textures();
}
// ---- resident chunk textures (Scene::resident_chunk_textures) ----------------------------------------
void rxh_scene_set_resident_chunk_textures(void *s, int on) { ((Scene *)s)->resident_chunk_textures = on != 0; }
int rxh_scene_resident_chunk_textures(void *s) { return ((Scene *)s)->resident_chunk_textures ? 1 : 0; }
// ---- the ray box tree (Scene::ray_accel): RXR_RAY_ACCEL_* ---------------------------------------------
void rxh_scene_set_ray_accel(void *s, uint32_t mode) { ((Scene *)s)->ray_accel = mode; }
uint32_t rxh_scene_ray_accel(void *s) { return ((Scene *)s)->ray_accel; }
int rxh_scene_ray_accel_info(void *s, uint64_t *out) { return ((Scene *)s)->ray_accel_info(out); }
// ---- a wave per ray through that tree (Scene::ray_wave): RXR_RAY_WAVE_* --------------------------------
void rxh_scene_set_ray_wave(void *s, uint32_t mode) { ((Scene *)s)->ray_wave = mode; }
uint32_t rxh_scene_ray_wave(void *s) { return ((Scene *)s)->ray_wave; }
int rxh_scene_ray_wave_info(void *s, uint64_t *out) { return ((Scene *)s)->ray_wave_info(out); }
// ---- counts that change are resized on the device (Scene::resize_meshes) ---------------------------------
void rxh_scene_set_resize_meshes(void *s, int on) { ((Scene *)s)->resize_meshes = on != 0; }
int rxh_scene_resize_meshes(void *s) { return ((Scene *)s)->resize_meshes ? 1 : 0; }

// ---- the ranged refresh after mesh updates (Scene::ray_refresh): RXR_RAY_REFRESH_* ----------------------
void rxh_scene_set_ray_refresh(void *s, uint32_t mode) { ((Scene *)s)->ray_refresh = mode; }
uint32_t rxh_scene_ray_refresh(void *s) { return ((Scene *)s)->ray_refresh; }
int rxh_scene_ray_refresh_info(void *s, uint64_t *out) { return ((Scene *)s)->ray_refresh_info(out); }
// Chunk::textures_generation (0 for a bad index) and Chunk::touch_textures
uint64_t rxh_chunk_textures_generation(void *s, int chunk) {
    Scene *sc = (Scene *)s;
    return chunk >= 0 && (size_t)chunk < sc->chunks.size() ? sc->chunks[chunk].textures_generation : 0;
}
void rxh_chunk_touch_textures(void *s, int chunk) {
    Scene *sc = (Scene *)s;
    if (chunk >= 0 && (size_t)chunk < sc->chunks.size()) sc->chunks[chunk].touch_textures();
}
// 1: the device holds newer bytes of chunks[chunk].terrain_texture than the host copy (rxh_chunk_terrain_texture reads them back)
int rxh_chunk_terrain_texture_stale(void *s, int chunk) {
    Scene *sc = (Scene *)s;
    return chunk >= 0 && (size_t)chunk < sc->chunks.size() && sc->chunks[chunk].terrain_texture_stale ? 1 : 0;
}
// how many registrations Rasterizer::upload has made (tests: an unchanged scene registers nothing)
uint64_t rxh_chunk_texture_registrations(void) { return chunk_texture_registrations(); }
// Terrain::rebuild_chunk_textures: 0 (baked and updated in place on the device), 1 (fallback: build_chunk_at per chunk) or a negative rxr_status
int rxh_terrain_rebuild_chunk_textures(void *t, void *s, const int32_t *coords, uint32_t n, const uint32_t *chunks, int32_t ppt) {
    return ((Terrain *)t)->rebuild_chunk_textures(*(Scene *)s, coords, n, chunks, ppt);
}
// Chunk::add_shader with the bake (Scene::chunk_add_shader): the shader index in the chunk, or a negative rxr_status
int rxh_chunk_add_shader_baked(void *s, int chunk, void *assets, uint32_t n_globals, int32_t shade_index, uint32_t shade_locals,
                               const uint32_t *const *fn_words, const uint32_t *fn_lens, uint32_t n_functions) {
    Program p;
    p.globals = n_globals;
    p.shade_index = shade_index;
    p.shade_locals = shade_locals;
    for (uint32_t i = 0; i < n_functions; ++i) p.user_functions.emplace_back(fn_words[i], fn_words[i] + fn_lens[i]);
    if (chunk < 0) return RXR_ERR_INVALID;
    return ((Scene *)s)->chunk_add_shader((size_t)chunk, std::move(p), *(const Assets *)assets);
}
// chunks[chunk].shader_textures[index]: 1 and its size if present, 0 for None, -1 for a bad index; rgba (may be NULL) receives w * h * 4 bytes
int rxh_chunk_shader_texture(void *s, int chunk, uint32_t index, uint32_t *w, uint32_t *h, uint8_t *rgba) {
    Scene *sc = (Scene *)s;
    if (chunk < 0 || (size_t)chunk >= sc->chunks.size() || index >= sc->chunks[chunk].shader_textures.size()) return -1;
    const Chunk &c = sc->chunks[chunk];
    if (!c.shader_texture_present[index]) return 0;
    *w = c.shader_textures[index].width;
    *h = c.shader_textures[index].height;
    if (rgba) memcpy(rgba, c.shader_textures[index].data.data(), c.shader_textures[index].data.size());
    return 1;
}
// Scene::bake_shaders (rxr_bake_shaders' arrays, include/rxr.h); RXR_OK or a negative rxr_status
int rxh_scene_bake_shaders(void *s, void *assets, const uint32_t *programs, uint32_t n, uint32_t width, uint32_t height, float *pixels, uint8_t *rgba) {
    return ((Scene *)s)->bake_shaders(*(const Assets *)assets, programs, n, width, height, pixels, rgba);
}
// ---- terrain (rusterix::Terrain) --------------------------------------------------------------------
void *rxh_terrain_new(float scale_x, float scale_y, int32_t chunk_size) {
    Terrain *t = new Terrain();
    t->scale[0] = scale_x;
    t->scale[1] = scale_y;
    t->chunk_size = chunk_size;
    return t;
}
void rxh_terrain_free(void *t) { delete (Terrain *)t; }
// Terrain::set_source behind the asset lookup: the texture the source resolves to; rgba == NULL: a source without one
void rxh_terrain_set_source(void *t, int32_t x, int32_t y, const uint8_t *rgba, uint32_t w, uint32_t h) {
    if (!rgba) return ((Terrain *)t)->set_source(x, y, nullptr);
    Texture tex;
    tex.width = w;
    tex.height = h;
    tex.data.assign(rgba, rgba + (size_t)w * h * 4);
    ((Terrain *)t)->set_source(x, y, &tex);
}
// Terrain::set_blend_mode; kind: RXR_TERRAIN_BLEND_* (include/rxr.h)
void rxh_terrain_set_blend_mode(void *t, int32_t x, int32_t y, uint32_t kind, uint32_t radius, float offset_x, float offset_y) {
    ((Terrain *)t)->set_blend_mode(x, y, kind, radius, offset_x, offset_y);
}
// Terrain::set_height / get_height
void rxh_terrain_set_height(void *t, int32_t x, int32_t y, float height) { ((Terrain *)t)->set_height(x, y, height); }
void rxh_terrain_remove_height(void *t, int32_t x, int32_t y) { ((Terrain *)t)->remove_height(x, y); }
float rxh_terrain_get_height(void *t, int32_t x, int32_t y) { return ((Terrain *)t)->get_height(x, y); }
float rxh_terrain_sample_height(void *t, float x, float y) { return ((Terrain *)t)->sample_height(x, y); }
float rxh_terrain_sample_height_bilinear(void *t, float x, float y) { return ((Terrain *)t)->sample_height_bilinear(x, y); }
// Terrain::ray_terrain_hit on the CPU: 1 and t_hit, world_pos[3], grid_pos[2] for Some, 0 for None
int rxh_terrain_ray_hit(void *t, const float *origin, const float *dir, float max_distance, float *t_hit, float *world_pos, int32_t *grid_pos) {
    Terrain::Hit h;
    if (!((Terrain *)t)->ray_terrain_hit(origin, dir, max_distance, h)) return 0;
    *t_hit = h.t;
    memcpy(world_pos, h.world_pos, sizeof h.world_pos);
    memcpy(grid_pos, h.grid_pos, sizeof h.grid_pos);
    return 1;
}
// the same for n rays over the host's worker pool, in the layout of rxr_terrain_hits
void rxh_terrain_ray_hits_cpu(void *t, const float *origins, const float *dirs, uint32_t n, float max_distance, uint32_t *hit, float *t_hit, float *world_pos,
                              int32_t *grid_pos) {
    ((Terrain *)t)->ray_terrain_hits_cpu(origins, dirs, n, max_distance, hit, t_hit, world_pos, grid_pos);
}
// ... and on the device (rxr_terrain_hits); RXR_OK or a negative rxr_status
int rxh_terrain_ray_hits(void *t, const float *origins, const float *dirs, uint32_t n, float max_distance, uint32_t *hit, float *t_hit, float *world_pos,
                         int32_t *grid_pos) {
    return ((Terrain *)t)->ray_terrain_hits(origins, dirs, n, max_distance, hit, t_hit, world_pos, grid_pos);
}
// TerrainChunk::build_mesh on the CPU: a new Batch3D (rxh_batch3d_free)
void *rxh_terrain_build_mesh(void *t, int32_t cx, int32_t cy) { return new Batch3D(((Terrain *)t)->build_mesh(cx, cy)); }
// the same for n chunks on the device (rxr_terrain_meshes) or, device == 0, on the CPU over the host's worker pool: out[i] is a new
// Batch3D; RXR_OK or a negative rxr_status (nothing is allocated then)
int rxh_terrain_build_meshes(void *t, const int32_t *coords, uint32_t n, int device, void **out) {
    std::vector<Batch3D> meshes;
    if (device) {
        const int rc = ((Terrain *)t)->build_meshes(coords, n, meshes);
        if (rc != RXR_OK) return rc;
    } else {
        ((Terrain *)t)->build_meshes_cpu(coords, n, meshes);
    }
    for (uint32_t i = 0; i < n; ++i) out[i] = new Batch3D(std::move(meshes[i]));
    return RXR_OK;
}
// Terrain::flatten_ops from the arrays of rxr_set_terrain_flatten (include/rxr.h); 0, or what rxr_check_terrain_flatten refuses (nothing changes then)
int rxh_terrain_set_flatten_ops(void *t, const uint32_t *kinds, const float *params, const uint32_t *ranges, uint32_t n_ops, const float *records, uint32_t n_records) {
    return ((Terrain *)t)->set_flatten_ops(kinds, params, ranges, n_ops, records, n_records);
}
// processed_heights of n chunks in the layout of rxr_flatten_terrain: on the device, or, device == 0, the dictionary transcription over
// the host's worker pool; RXR_OK or a negative rxr_status
int rxh_terrain_process_heights(void *t, const int32_t *coords, uint32_t n, int device, float *heights, uint8_t *present) {
    if (device) return ((Terrain *)t)->process_heights(coords, n, heights, present);
    ((Terrain *)t)->process_heights_cpu(coords, n, heights, present);
    return RXR_OK;
}
void rxh_terrain_set_device_modifiers(void *t, int on) { ((Terrain *)t)->device_modifiers = on != 0; }
// out[0], out[1]: how often a Terrain has called rxr_set_terrain_heights / rxr_set_terrain_flatten
void rxh_terrain_registrations(uint64_t *out) {
    out[0] = terrain_height_registrations();
    out[1] = terrain_flatten_registrations();
}
// ---- the generated terrain's height field (rusterix::TerrainGenerator) ----------------------------
void *rxh_terrain_generator_new(uint32_t subdivisions) {
    TerrainGenerator *g = new TerrainGenerator();
    g->subdivisions = subdivisions;
    return g;
}
void rxh_terrain_generator_free(void *g) { delete (TerrainGenerator *)g; }
// the lists of rxr_set_terrain_generator (include/rxr.h); 0, or RXR_ERR_INVALID for offsets the lists do not fit (nothing changes then)
int rxh_terrain_generator_set(void *g_, const float *cps, uint32_t C, const float *ridges, uint32_t R, const uint32_t *off, const float *edges, uint32_t E,
                              const float *lines, uint32_t L, const float *map_box) {
    TerrainGenerator *g = (TerrainGenerator *)g_;
    if (rxr_check_terrain_generator(cps, C, ridges, R, off, edges, E, lines, L, map_box, nullptr, 0) == RXR_ERR_INVALID) return RXR_ERR_INVALID;
    g->control_points.assign(cps, cps + 4 * (size_t)C);
    g->ridges.assign(ridges, ridges + 4 * (size_t)R);
    g->ridge_edge_offsets.assign(1, 0u);
    if (R) g->ridge_edge_offsets.assign(off, off + R + 1);
    g->ridge_edges.assign(edges, edges + 4 * (size_t)E);
    g->linedefs.assign(lines, lines + 9 * (size_t)L);
    memcpy(g->map_box, map_box, sizeof g->map_box);
    g->touch();
    return RXR_OK;
}
// interpolate_heights / sample_normal_at for n points on the CPU over the host's worker pool (normals may be NULL)
void rxh_terrain_generator_sample_cpu(void *g, const float *points, uint32_t n, float *heights, float *normals) {
    ((TerrainGenerator *)g)->interpolate_heights(points, n, heights, normals);
}
// ... and on the device (rxr_generated_heights); RXR_OK or a negative rxr_status
int rxh_terrain_generator_sample(void *g, const float *points, uint32_t n, float *heights, float *normals) {
    return ((TerrainGenerator *)g)->sample_heights(points, n, heights, normals);
}
void rxh_terrain_generator_tile_normal(void *g, int32_t tx, int32_t tz, float *normal) { ((TerrainGenerator *)g)->tile_normal(tx, tz, normal); }
// tile_outline_world: out receives [4 * max(subdivisions, 1)][3]
void rxh_terrain_generator_tile_outline(void *g, int32_t tx, int32_t tz, float *out) {
    const std::vector<float> o = ((TerrainGenerator *)g)->tile_outline_world(tx, tz);
    memcpy(out, o.data(), o.size() * sizeof(float));
}
// generate_grid's steps; points (may be NULL) receives [steps_y][steps_x][2] when both are positive and their product is at most capacity
void rxh_terrain_generator_grid(void *g, const float *box, int32_t *steps, float *points, uint32_t capacity) {
    ((TerrainGenerator *)g)->grid_steps(box, steps[0], steps[1]);
    if (!points || steps[0] <= 0 || steps[1] <= 0 || (uint64_t)steps[0] * (uint64_t)steps[1] > capacity) return;   // (no points are made then)
    const std::vector<float> grid = ((TerrainGenerator *)g)->generate_grid(box, steps[0], steps[1]);
    memcpy(points, grid.data(), grid.size() * sizeof(float));
}
// triangulate: 6 * (steps_x - 1) * (steps_y - 1) indices
void rxh_terrain_generator_triangulate(int32_t steps_x, int32_t steps_y, uint32_t *indices) {
    const std::vector<uint32_t> t = TerrainGenerator::triangulate(steps_x, steps_y);
    memcpy(indices, t.data(), t.size() * sizeof(uint32_t));
}
// n boxes in the layout of rxr_generated_grids: on the device, or (device == 0) on the CPU
int rxh_terrain_generator_grids(void *g, const float *boxes, uint32_t n, uint32_t stride, int device, uint32_t *counts, float *heights) {
    if (device) return ((TerrainGenerator *)g)->grid_heights(boxes, n, stride, counts, heights);
    ((TerrainGenerator *)g)->grid_heights_cpu(boxes, n, stride, counts, heights);
    return RXR_OK;
}
// the lists of rxr_set_terrain_exclusions (include/rxr.h); 0, or RXR_ERR_INVALID for offsets the lists do not fit (nothing changes then)
int rxh_terrain_generator_set_exclusions(void *g_, const float *boxes, const uint32_t *off, const float *verts, uint32_t S, uint32_t V) {
    TerrainGenerator *g = (TerrainGenerator *)g_;
    if (rxr_check_terrain_exclusions(boxes, off, verts, S, V, nullptr, 0) == RXR_ERR_INVALID) return RXR_ERR_INVALID;
    g->excluded_boxes.assign(boxes, boxes + 4 * (size_t)S);
    g->excluded_vertex_offsets.assign(1, 0u);
    if (S) g->excluded_vertex_offsets.assign(off, off + S + 1);
    g->excluded_vertices.assign(verts, verts + 2 * (size_t)V);
    g->touch();
    return RXR_OK;
}
// n boxes in the layout of rxr_generated_meshes: on the device, or (device == 0) the CPU apply_exclusions
int rxh_terrain_generator_meshes(void *g, const float *boxes, uint32_t n, uint32_t stride, int device, uint32_t *counts, float *vertices) {
    if (device) return ((TerrainGenerator *)g)->generate_meshes(boxes, n, stride, counts, vertices);
    ((TerrainGenerator *)g)->generate_meshes_cpu(boxes, n, stride, counts, vertices);
    return RXR_OK;
}
// the tile overrides of rxr_set_terrain_tiles (include/rxr.h); 0, or what rxr_check_terrain_tiles refuses (nothing changes then)
int rxh_terrain_generator_set_tiles(void *g, const int32_t *cells, const uint32_t *slots, uint32_t n, uint32_t n_tiles) {
    return ((TerrainGenerator *)g)->set_tiles(cells, slots, n, n_tiles);
}
// n boxes in the layout of rxr_generated_tile_meshes: on the device, or (device == 0) the CPU partition_by_tiles
int rxh_terrain_generator_tile_meshes(void *g, const float *boxes, uint32_t n, uint32_t max_groups, uint32_t vertex_stride, uint32_t triangle_stride, int device,
                                      uint32_t *box_counts, uint32_t *counts, uint32_t *group_tiles, float *vertices, float *uvs, uint32_t *indices) {
    TerrainGenerator *t = (TerrainGenerator *)g;
    if (device) return t->generate_tile_meshes(boxes, n, max_groups, vertex_stride, triangle_stride, box_counts, counts, group_tiles, vertices, uvs, indices);
    t->generate_tile_meshes_cpu(boxes, n, max_groups, vertex_stride, triangle_stride, box_counts, counts, group_tiles, vertices, uvs, indices);
    return RXR_OK;
}
// point_in_sector for n points [n][2] against sector s on the CPU: inside [n] (1 / 0)
void rxh_terrain_generator_points_in_sector(void *g, const float *points, uint32_t n, uint32_t s, uint8_t *inside) {
    for (uint32_t i = 0; i < n; ++i) inside[i] = ((TerrainGenerator *)g)->point_in_sector(points[2 * (size_t)i], points[2 * (size_t)i + 1], s) ? 1 : 0;
}
// Scene::rebuild_terrain_meshes: 0 (updated in place on the device), 1 (fallback: the batches were replaced on the host) or a negative rxr_status
int rxh_scene_rebuild_terrain_meshes(void *s, void *t, const int32_t *coords, uint32_t n, const uint32_t *chunks) {
    return ((Scene *)s)->rebuild_terrain_meshes(*(const Terrain *)t, coords, n, chunks);
}
// Scene::rebuild_generated_tile_meshes: 0 (updated in place on the device), 1 (the batches were replaced on the host) or a negative rxr_status
int rxh_scene_rebuild_generated_tile_meshes(void *s, void *g, const float *boxes, uint32_t n, const uint32_t *chunks, uint32_t max_groups) {
    return ((Scene *)s)->rebuild_generated_tile_meshes(*(const TerrainGenerator *)g, boxes, n, chunks, max_groups);
}
// Terrain::bake_chunk on the CPU: side * side * 4 bytes; RXR_OK or a negative rxr_status
int rxh_terrain_bake_chunk(void *t, int32_t cx, int32_t cy, int32_t ppt, uint8_t *rgba) {
    std::vector<uint8_t> out;
    const int rc = ((Terrain *)t)->bake_chunk(cx, cy, ppt, out);
    if (rc == RXR_OK) memcpy(rgba, out.data(), out.size());
    return rc;
}
// the same for n chunks on the device (rxr_bake_terrain)
int rxh_terrain_bake_chunks(void *t, const int32_t *coords, uint32_t n, int32_t ppt, uint8_t *rgba) {
    return ((Terrain *)t)->bake_chunks(coords, n, ppt, rgba);
}
// Terrain::build_chunk_at without modifiers: chunks[chunk].terrain_texture from the device's bake
int rxh_terrain_build_chunk_at(void *t, int32_t cx, int32_t cy, int32_t ppt, void *s, int chunk) {
    Scene *sc = (Scene *)s;
    if (chunk < 0 || (size_t)chunk >= sc->chunks.size()) return RXR_ERR_INVALID;
    return ((Terrain *)t)->build_chunk_at(cx, cy, ppt, sc->chunks[chunk]);
}
// chunks[chunk].terrain_texture: 1 and its size if present, 0 for None; rgba (may be NULL) receives w * h * 4 bytes
int rxh_chunk_terrain_texture(void *s, int chunk, uint32_t *w, uint32_t *h, uint8_t *rgba) {
    Scene *sc = (Scene *)s;
    if (chunk < 0 || (size_t)chunk >= sc->chunks.size()) return -1;
    const Chunk &c = sc->chunks[chunk];
    if (!c.has_terrain_texture) return 0;
    if (rgba && c.terrain_texture_stale) {   // the device's slot holds the bytes (Terrain::rebuild_chunk_textures): read them back
        const int rc = sc->refresh_chunk_textures();
        if (rc != RXR_OK) return rc;
    }
    *w = c.terrain_texture.width;
    *h = c.terrain_texture.height;
    if (rgba) memcpy(rgba, c.terrain_texture.data.data(), c.terrain_texture.data.size());
    return 1;
}
void rxh_chunk_add_light(void *s, int chunk, const rxr_light *l) { ((Scene *)s)->chunks[chunk].lights.push_back(*l); }
// scene.add_shader (src/scene.rs:104-134) minus the parser / compiler; chunk >= 0: that chunk's shaders
int rxh_scene_add_program(void *s, int chunk, uint32_t n_globals, int32_t shade_index, uint32_t shade_locals,
                          const uint32_t *const *fn_words, const uint32_t *fn_lens, uint32_t n_functions) {
    Scene *sc = (Scene *)s;
    Program p;
    p.globals = n_globals;
    p.shade_index = shade_index;
    p.shade_locals = shade_locals;
    for (uint32_t i = 0; i < n_functions; ++i) p.user_functions.emplace_back(fn_words[i], fn_words[i] + fn_lens[i]);
    if (chunk >= 0) {
        if ((size_t)chunk >= sc->chunks.size()) return RXR_ERR_INVALID;
        sc->chunks[chunk].shaders.push_back(std::move(p));
        sc->shaders_generation = next_generation();
        return (int)sc->chunks[chunk].shaders.size() - 1;
    }
    return (int)sc->add_program(std::move(p));
}
uint32_t rxh_scene_num_dynamic_lights(void *s) { return (uint32_t)((Scene *)s)->dynamic_lights.size(); }

// ---- Batch3D --------------------------------------------------------------------------------------
void *rxh_batch3d_new(const float *v4, uint32_t nv, const uint32_t *idx, uint32_t nt, const float *uv2) {
    return new Batch3D(Batch3D::make(v4, nv, idx, nt, uv2));
}
void *rxh_batch3d_from_box(float x, float y, float z, float w, float h, float d) { return new Batch3D(Batch3D::from_box(x, y, z, w, h, d)); }
void *rxh_batch3d_from_obj(const char *text) { return new Batch3D(Batch3D::from_obj(text)); }
void rxh_batch3d_free(void *b) { delete (Batch3D *)b; }
void rxh_batch3d_add(void *b, const float *v4, uint32_t nv, const uint32_t *idx, uint32_t nt, const float *uv2) {
    ((Batch3D *)b)->add(v4, nv, idx, nt, uv2);
}
void rxh_batch3d_set_normals(void *b, const float *n3, uint32_t n) {
    ((Batch3D *)b)->normals.assign(n3, n3 + (size_t)n * 3);
    ((Batch3D *)b)->touch();
}
void rxh_batch3d_compute_vertex_normals(void *b) { ((Batch3D *)b)->compute_vertex_normals(); }
void rxh_batch3d_set_source(void *b, uint32_t kind, uint32_t index, const uint8_t *pixel) { set_source(((Batch3D *)b)->source_, kind, index, pixel); }
// PixelSource::EntityTile(id, seq) / ItemTile(id, seq)
void rxh_batch3d_set_source_seq(void *b, int is_item, uint32_t id, uint32_t seq) {
    ((Batch3D *)b)->source_ = is_item ? PixelSource::ItemTile(id, seq) : PixelSource::EntityTile(id, seq);
}
void rxh_batch3d_set_repeat_mode(void *b, int m) { ((Batch3D *)b)->repeat_mode_ = (uint32_t)m; }
// batch.material (src/shapestack/material.rs): role and modifier as their to_u8 / from_u8 numbers; has == 0: None
void rxh_batch3d_set_material(void *b, int has, uint32_t role, uint32_t modifier, float value) {
    Batch3D *B = (Batch3D *)b;
    B->has_material = has != 0;
    B->material_role = role;
    B->material_modifier = modifier;
    B->material_value = value;
}
void rxh_batch3d_set_cull_mode(void *b, int m) { ((Batch3D *)b)->cull_mode_ = (CullMode)m; }
void rxh_batch3d_set_ambient_color(void *b, float r, float g, float bl) { ((Batch3D *)b)->ambient_color_ = Vec3{r, g, bl}; }
void rxh_batch3d_set_transform(void *b, const float *m16) { ((Batch3D *)b)->transform_3d = mat4_from(m16); }
void rxh_batch3d_set_profile_id(void *b, int has, uint32_t id) {
    ((Batch3D *)b)->has_profile_id = has != 0;
    ((Batch3D *)b)->profile_id_ = id;
}
void rxh_batch3d_set_shader(void *b, int shader) { ((Batch3D *)b)->shader_ = shader; }
void rxh_batch3d_counts(void *b, uint32_t *nv, uint32_t *nt) {
    *nv = (uint32_t)((Batch3D *)b)->vertex_count();
    *nt = (uint32_t)((Batch3D *)b)->triangle_count();
}
uint32_t rxh_batch3d_num_normals(void *b) { return (uint32_t)(((Batch3D *)b)->normals.size() / 3); }
void rxh_batch3d_get_geometry(void *b, float *v4, uint32_t *idx, float *uv2, float *n3) {
    Batch3D *p = (Batch3D *)b;
    memcpy(v4, p->vertices.data(), p->vertices.size() * 4);
    memcpy(idx, p->indices.data(), p->indices.size() * 4);
    memcpy(uv2, p->uvs.data(), p->uvs.size() * 4);
    if (n3) memcpy(n3, p->normals.data(), p->normals.size() * 4);
}
int rxh_scene_push_batch3d(void *s, void *b, int list, int chunk) {
    auto *l = list3d((Scene *)s, list, chunk);
    if (!l) return RXR_ERR_INVALID;
    if (list == RXR_LIST_CHUNK_TERRAIN) l->clear();  // Option<Batch3D>: the latest one wins
    l->push_back(*(Batch3D *)b);
    return 0;
}

// ---- Batch2D --------------------------------------------------------------------------------------
void *rxh_batch2d_new(const float *v2, uint32_t nv, const uint32_t *idx, uint32_t nt, const float *uv2) {
    return new Batch2D(Batch2D::make(v2, nv, idx, nt, uv2));
}
void *rxh_batch2d_from_rectangle(float x, float y, float w, float h) { return new Batch2D(Batch2D::from_rectangle(x, y, w, h)); }
void rxh_batch2d_free(void *b) { delete (Batch2D *)b; }
void rxh_batch2d_set_mode(void *b, int m) { ((Batch2D *)b)->mode_ = (uint32_t)m; }
void rxh_batch2d_set_repeat_mode(void *b, int m) { ((Batch2D *)b)->repeat_mode_ = (uint32_t)m; }
void rxh_batch2d_set_source(void *b, uint32_t kind, uint32_t index, const uint8_t *pixel) { set_source(((Batch2D *)b)->source_, kind, index, pixel); }
void rxh_batch2d_set_source_seq(void *b, int is_item, uint32_t id, uint32_t seq) {
    ((Batch2D *)b)->source_ = is_item ? PixelSource::ItemTile(id, seq) : PixelSource::EntityTile(id, seq);
}
void rxh_batch2d_set_receives_light(void *b, int v) { ((Batch2D *)b)->receives_light_ = v != 0; }
void rxh_batch2d_set_shader(void *b, int shader) { ((Batch2D *)b)->shader_ = shader; }
int rxh_scene_push_batch2d(void *s, void *b, int dynamic, int chunk) {
    Scene *sc = (Scene *)s;
    if (chunk >= 0) {
        if ((size_t)chunk >= sc->chunks.size()) return RXR_ERR_INVALID;
        sc->chunks[chunk].batches2d.push_back(*(Batch2D *)b);
    } else {
        (dynamic ? sc->d2_dynamic : sc->d2_static).push_back(*(Batch2D *)b);
    }
    return 0;
}

// ---- Assets ---------------------------------------------------------------------------------------
void *rxh_assets_new() { return new Assets(); }
void rxh_assets_free(void *a) { delete (Assets *)a; }
void rxh_assets_add_tile(void *a, const uint8_t *const *frames, const uint32_t *ws, const uint32_t *hs, uint32_t n) {
    Assets *as = (Assets *)a;
    as->tile_list.push_back(make_tile(frames, ws, hs, n));
    as->generation = next_generation();
}

// assets.entity_tiles / item_tiles: makes `id` known (an entry without sequences) ...
void rxh_assets_add_sequence_id(void *a, int is_item, uint32_t id) {
    Assets *as = (Assets *)a;
    (is_item ? as->item_tiles : as->entity_tiles)[id];
    as->generation = next_generation();
}
// ... and appends one sequence tile to it (IndexMap insertion order = get_index order)
void rxh_assets_add_sequence_tile(void *a, int is_item, uint32_t id, const uint8_t *const *frames, const uint32_t *ws, const uint32_t *hs, uint32_t n) {
    Assets *as = (Assets *)a;
    (is_item ? as->item_tiles : as->entity_tiles)[id].push_back(make_tile(frames, ws, hs, n));
    as->generation = next_generation();
}

void rxh_assets_set_patterns(void *a, int normal, const float *const *rgb, const uint32_t *ws, const uint32_t *hs, uint32_t n) {
    Assets *as = (Assets *)a;
    std::vector<Pattern> &dst = normal ? as->patterns_normal : as->patterns;
    dst.clear();
    for (uint32_t i = 0; i < n; ++i) {
        Pattern t;
        t.width = ws[i];
        t.height = hs[i];
        t.rgb.assign(rgb[i], rgb[i] + (size_t)3 * ws[i] * hs[i]);
        dst.push_back(std::move(t));
    }
    as->shader_env_generation = next_generation();
}
void rxh_assets_set_palette(void *a, const float *rgb3, const uint8_t *present, uint32_t n) {
    Assets *as = (Assets *)a;
    as->palette_rgb.assign(rgb3, rgb3 + (size_t)3 * n);
    as->palette_present.assign(n, 1);
    if (present) as->palette_present.assign(present, present + n);
    as->shader_env_generation = next_generation();
}

// ---- Rasterizer -----------------------------------------------------------------------------------
void *rxh_rasterizer_setup(const float *m2d9, const float *view16, const float *proj16) {
    Mat3 m2d{};
    if (m2d9) memcpy(m2d.m, m2d9, sizeof(m2d.m));
    return new Rasterizer(Rasterizer::setup(m2d9 ? &m2d : nullptr, mat4_from(view16), mat4_from(proj16)));
}
void rxh_rasterizer_free(void *r) { delete (Rasterizer *)r; }
void rxh_rasterizer_render_mode(void *r, int d2, int d3, int ignore_bg) {
    Rasterizer *x = (Rasterizer *)r;
    x->d2_active = d2 != 0;
    x->d3_active = d3 != 0;
    x->ignore_background_shader = ignore_bg != 0;
}
void rxh_rasterizer_sample_mode(void *r, int m) { ((Rasterizer *)r)->sample_mode_ = (uint32_t)m; }
void rxh_rasterizer_brush_preview(void *r, int on, float px, float py, float pz, float radius, float falloff) {
    Rasterizer *x = (Rasterizer *)r;
    x->has_brush_preview = on != 0;
    x->brush_position[0] = px;
    x->brush_position[1] = py;
    x->brush_position[2] = pz;
    x->brush_radius = radius;
    x->brush_falloff = falloff;
}
void rxh_rasterizer_background(void *r, const uint8_t *px) {
    Rasterizer *x = (Rasterizer *)r;
    x->has_background_color = px != nullptr;
    if (px) memcpy(x->background_color, px, 4);
}
void rxh_rasterizer_ambient(void *r, const float *a4) {
    Rasterizer *x = (Rasterizer *)r;
    x->has_ambient = a4 != nullptr;
    if (a4) x->ambient_color = Vec4{a4[0], a4[1], a4[2], a4[3]};
}
void rxh_rasterizer_time(void *r, float t) { ((Rasterizer *)r)->time_ = t; }
void rxh_rasterizer_preserve_transparency(void *r, int v) { ((Rasterizer *)r)->preserve_transparency = v != 0; }
void rxh_rasterizer_sun(void *r, const float *dir3, float day_factor) {
    Rasterizer *x = (Rasterizer *)r;
    x->has_sun = dir3 != nullptr;
    if (dir3) x->sun_dir = Vec3{dir3[0], dir3[1], dir3[2]};
    x->day_factor = day_factor;
}
void rxh_rasterizer_mapmini_add_occluder(void *r, float minx, float miny, float maxx, float maxy, float occ) {
    ((Rasterizer *)r)->mapmini.occluded_sectors.push_back(rxr_occluder{{minx, miny}, {maxx, maxy}, occ});
}
void rxh_rasterizer_mapmini_add_linedef(void *r, float x0, float y0, float x1, float y1) {
    ((Rasterizer *)r)->mapmini.linedefs.push_back(rxr_linedef{{x0, y0}, {x1, y1}});
}
void rxh_rasterizer_get_derived(void *r, float *inv_view16, float *inv_proj16, float *camera_pos3) {
    Rasterizer *x = (Rasterizer *)r;
    memcpy(inv_view16, x->inverse_view_matrix.m, 64);
    memcpy(inv_proj16, x->inverse_projection_matrix.m, 64);
    camera_pos3[0] = x->camera_pos.x; camera_pos3[1] = x->camera_pos.y; camera_pos3[2] = x->camera_pos.z;
}
// Rasterizer::screen_ray (src/rasterizer.rs:1843-1870): origin3 / dir3 receive the ray
void rxh_rasterizer_screen_ray(void *r, float x, float y, float *origin3, float *dir3) { ((Rasterizer *)r)->screen_ray(x, y, origin3, dir3); }
int rxh_rasterizer_rasterize(void *r, void *scene, uint8_t *pixels, uint32_t w, uint32_t h, uint32_t tile_size, void *assets) {
    return ((Rasterizer *)r)->rasterize(*(Scene *)scene, pixels, w, h, tile_size, *(Assets *)assets);
}
// project + flatten + host->device hand-over only (no render)
int rxh_rasterizer_upload(void *r, void *scene, uint32_t w, uint32_t h, uint32_t tile_size, void *assets) {
    return ((Rasterizer *)r)->upload(*(Scene *)scene, w, h, tile_size, *(Assets *)assets);
}
// host-side projection only (what stays on the host); used by the CPU tests
int rxh_scene_project(void *r, void *scene, uint32_t w, uint32_t h) {
    Rasterizer *x = (Rasterizer *)r;
    return ((Scene *)scene)->project(x->has_m2d ? &x->projection_matrix_2d : nullptr, x->view_matrix, x->projection_matrix, (float)w, (float)h)
               ? 0
               : RXR_ERR_INVALID;
}

// ---- introspection of projected batches -------------------------------------------------------------
int rxh_scene_batch3d_counts(void *s, int list, int chunk, uint32_t i, uint32_t *nv, uint32_t *nt, uint32_t *has_normals) {
    auto *l = list3d((Scene *)s, list, chunk);
    if (!l || i >= l->size()) return RXR_ERR_INVALID;
    const Batch3D &b = (*l)[i];
    *nv = (uint32_t)(b.projected_vertices.size() / 4);
    *nt = (uint32_t)b.edges.size();
    *has_normals = b.normals.empty() ? 0 : 1;
    return 0;
}
int rxh_scene_batch3d_copy(void *s, int list, int chunk, uint32_t i, float *pv4, float *uv2, float *n3, uint32_t *idx3,
                           float *edges10, float *bbox5) {
    auto *l = list3d((Scene *)s, list, chunk);
    if (!l || i >= l->size()) return RXR_ERR_INVALID;
    const Batch3D &b = (*l)[i];
    const size_t nv = b.projected_vertices.size() / 4;
    memcpy(pv4, b.projected_vertices.data(), b.projected_vertices.size() * 4);
    memcpy(uv2, b.clipped_uvs.data(), std::min(b.clipped_uvs.size(), nv * 2) * 4);
    memcpy(n3, b.clipped_normals.data(), std::min(b.clipped_normals.size(), nv * 3) * 4);
    for (size_t k = 0; k < b.edges.size(); ++k) {
        for (int j = 0; j < 3; ++j) idx3[k * 3 + j] = b.clipped_indices[k * 3 + j];
        for (int j = 0; j < 3; ++j) {
            edges10[k * 10 + j] = b.edges[k].a[j];
            edges10[k * 10 + 3 + j] = b.edges[k].b[j];
            edges10[k * 10 + 6 + j] = b.edges[k].c[j];
        }
        edges10[k * 10 + 9] = b.edges[k].visible ? 1.0f : 0.0f;
    }
    bbox5[0] = b.has_bounding_box ? 1.0f : 0.0f;
    bbox5[1] = b.bounding_box.x; bbox5[2] = b.bounding_box.y; bbox5[3] = b.bounding_box.width; bbox5[4] = b.bounding_box.height;
    return 0;
}

// Scene::compute_static_normals (dynamic == 0) / compute_dynamic_normals; route: Scene::NORMALS_CPU, _DEVICE, _POOL
int rxh_scene_compute_normals(void *s, int dynamic, int route) {
    return dynamic ? ((Scene *)s)->compute_dynamic_normals(route) : ((Scene *)s)->compute_static_normals(route);
}
// the object-space normals of one batch: its vertex count, and (n3 given, room for `capacity` vertices) their values
int rxh_scene_batch3d_normals(void *s, int list, int chunk, uint32_t i, float *n3, uint32_t capacity) {
    auto *l = list3d((Scene *)s, list, chunk);
    if (!l || i >= l->size()) return RXR_ERR_INVALID;
    const Batch3D &b = (*l)[i];
    const size_t nv = b.normals.size() / 3;
    if (n3) memcpy(n3, b.normals.data(), std::min<size_t>(nv, capacity) * 12);
    return (int)nv;
}

// ---- cameras ----------------------------------------------------------------------------------------
void rxh_camera_orbit(const float *center3, float distance, float azimuth, float elevation, float fov, float near, float far,
                      float w, float h, float *view16, float *proj16) {
    Mat4 v, p;
    orbit_camera(Vec3{center3[0], center3[1], center3[2]}, distance, azimuth, elevation, fov, near, far, w, h, v, p);
    memcpy(view16, v.m, 64);
    memcpy(proj16, p.m, 64);
}
void rxh_camera_firstp(const float *pos3, const float *center3, float fov, float near, float far, float w, float h,
                       float *view16, float *proj16) {
    Mat4 v, p;
    firstp_camera(Vec3{pos3[0], pos3[1], pos3[2]}, Vec3{center3[0], center3[1], center3[2]}, fov, near, far, w, h, v, p);
    memcpy(view16, v.m, 64);
    memcpy(proj16, p.m, 64);
}

}  // extern "C"
