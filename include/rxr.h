/*
 * rxr.h -- C ABI of the MI355X (gfx950) rasterizer back end for Rusterix' tile rasterizer.
 *
 * This is the drop-in boundary.  The reference has no FFI of its own; the boundary it exposes is the
 * Rust call
 *
 *     Rasterizer::setup(m2d, view, proj) .. .rasterize(&mut scene, pixels, w, h, tile_size, &assets)
 *                                                   (reference src/rasterizer.rs:92-152, 185-193)
 *
 * The host side (Rust in a real deployment, the C++ mirror under rusterix_amd/csrc/host here) keeps
 * scene set-up, Scene::project (src/scene.rs:154-200) and the Edges precompute (src/edge.rs:12-24),
 * flattens what the per-tile loops read into the POD structs below and hands them to the entry
 * points declared at the bottom of this file.  Everything that `rasterize` does after
 * `scene.project(..)` (src/rasterizer.rs:256-579) happens behind this ABI on the GPU.
 *
 * Conventions
 *   - plain C, no torch / C++ types; all pointers are HOST pointers unless the name says `dev`.
 *   - every function returns RXR_OK (0) or a negative rxr_status; nothing throws or aborts.
 *   - matrices are column-major exactly as vek stores them: m[c*4 + r] == cols[c][r].
 *   - `usize` indices of the reference are u32 here (the shim asserts < 2^32).
 *   - structs carry no implicit ownership: the caller keeps every buffer alive until the call
 *     returns; the library copies what it needs.
 *   - threads: a context (and a multi-device handle with its members) is used by one thread at a time -- the one exception is
 *     rxr_stream_batch3d, which any number of threads may call on the same context between rxr_stream_begin and
 *     rxr_upload_frame.  Different contexts are independent: threads that each own their contexts need no lock between them, on
 *     one GPU or several (what the library shares process-wide, the run-time compiler's cache and job table, it guards itself;
 *     tests/abi_threads.c).
 */
#ifndef RXR_H
#define RXR_H

#if !defined(__HIPCC_RTC__) /* (hiprtc, the run-time compiler of rxr_jit.hip, has size_t built in and no <stddef.h>) */
#include <stddef.h>
#endif
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RXR_ABI_VERSION 5u

typedef enum rxr_status {
    RXR_OK = 0,
    RXR_ERR_INVALID = -1,     /* bad argument / index out of range (the reference would panic)   */
    RXR_ERR_NO_DEVICE = -2,   /* no HIP device, or device id out of range                         */
    RXR_ERR_HIP = -3,         /* a HIP runtime call failed; see rxr_last_error                    */
    RXR_ERR_UNSUPPORTED = -4, /* scene uses a feature the device path does not implement (yet)    */
    RXR_ERR_OOM = -5,
    RXR_ERR_OVERFLOW = -6     /* rxr_synchronize: a bin list overflowed in a launch that was queued BEFORE the last one (an
                                 asynchronous caller that does not synchronize per frame): that frame was shipped incomplete.
                                 The lists have been grown and the last launch rendered again; render the lost frames again. */
} rxr_status;

/* ---- enums mirrored from the reference ------------------------------------------------------ */

/* SampleMode, src/texture.rs:5-12 */
enum { RXR_SAMPLE_NEAREST = 0, RXR_SAMPLE_LINEAR = 1 };
/* RepeatMode, src/texture.rs:14-25 */
enum { RXR_REPEAT_CLAMP_XY = 0, RXR_REPEAT_REPEAT_XY = 1, RXR_REPEAT_REPEAT_X = 2, RXR_REPEAT_REPEAT_Y = 3 };
/* PrimitiveMode, src/batch/mod.rs:4-15 */
enum { RXR_MODE_TRIANGLES = 0, RXR_MODE_LINES = 1, RXR_MODE_LINE_STRIP = 2, RXR_MODE_LINE_LOOP = 3 };
/* LightType, src/map/light.rs:6-14 */
enum { RXR_LIGHT_POINT = 0, RXR_LIGHT_AMBIENT = 1, RXR_LIGHT_AMBIENT_DAYLIGHT = 2, RXR_LIGHT_SPOT = 3,
       RXR_LIGHT_AREA = 4, RXR_LIGHT_DAYLIGHT = 5 };
/* PixelSource, src/map/pixelsource.rs:23-37.  Only the variants the raster loops distinguish
 * (src/rasterizer.rs:672-758, 1101-1222); every other variant is RXR_SOURCE_OTHER. */
enum { RXR_SOURCE_OTHER = 0,         /* Off / TileId / MaterialId / Sequence / Color / ShapeFXGraphId:
                                        3D texel [0,0,0,255], 2D texel [0,0,0,0]                   */
       RXR_SOURCE_STATIC_TILE = 1,   /* StaticTileIndex(u16) -> assets.tile_list[index]            */
       RXR_SOURCE_DYNAMIC_TILE = 2,  /* DynamicTileIndex(u16) -> scene.dynamic_textures[index]     */
       RXR_SOURCE_PIXEL = 3,         /* Pixel([u8;4])                                              */
       RXR_SOURCE_TERRAIN = 4,       /* Terrain (chunk terrain texture)                            */
       RXR_SOURCE_MISSING = 5 };     /* EntityTile/ItemTile whose lookup failed on the host: [0,0,0,0];
                                        a successful lookup is passed as RXR_SOURCE_DYNAMIC_TILE     */
/* Host-side only -- these two never cross the ABI (rxr_upload_frame answers them with RXR_ERR_INVALID): EntityTile(id, index) /
 * ItemTile(id, index), src/map/pixelsource.rs:29-30.  The raster loops look (id, index) up per fragment in
 * assets.entity_tiles / assets.item_tiles (FxHashMap<u32, IndexMap<String, Tile>>; src/rasterizer.rs:1140-1187, :705-748,
 * :1548-1595); the lookup is frame-constant, so the HOST does it once per batch and hands the device
 * RXR_SOURCE_DYNAMIC_TILE (hit: the tile travels with the dynamic tiles of rxr_set_textures) or RXR_SOURCE_MISSING (unknown
 * id, or no `index`-th sequence: [0,0,0,0] in all three loops).  The host mirror and the oracle use these values for the
 * unresolved variants. */
enum { RXR_HOST_SOURCE_ENTITY_TILE = 64, RXR_HOST_SOURCE_ITEM_TILE = 65 };
/* which Scene list a 3D batch came from; order of the array is submission order
 * (src/rasterizer.rs:314-405) */
enum { RXR_LIST_CHUNK_OPACITY = 0, RXR_LIST_CHUNK = 1, RXR_LIST_CHUNK_TERRAIN = 2, RXR_LIST_STATIC = 3,
       RXR_LIST_DYNAMIC = 4, RXR_LIST_OVERLAY = 5 };
/* background shader kinds (trait Shader, src/shader/mod.rs:9-33) that the device evaluates itself */
enum { RXR_BG_NONE = 0, RXR_BG_VGRADIENT = 1 /* src/shader/vgradient.rs:11-15 */,
       RXR_BG_HOST_PIXELS = 2 /* any other `dyn Shader`, evaluated by the host into background_pixels */,
       RXR_BG_GRID = 3 /* GridShader, src/shader/grid.rs:10-109; parameters in rxr_frame.background_grid */ };

/* rxr_frame.flags */
#define RXR_FLAG_D2_ACTIVE             (1u << 0) /* RenderMode.d2_active, src/rendermode.rs:4-11   */
#define RXR_FLAG_D3_ACTIVE             (1u << 1) /* RenderMode.d3_active                            */
#define RXR_FLAG_IGNORE_BG_SHADER      (1u << 2) /* RenderMode.ignore_background_shader             */
#define RXR_FLAG_PRESERVE_TRANSPARENCY (1u << 3) /* Rasterizer.preserve_transparency, :72           */
#define RXR_FLAG_HAS_BACKGROUND_COLOR  (1u << 4) /* Rasterizer.background_color.is_some(), :59      */
#define RXR_FLAG_HAS_AMBIENT           (1u << 5) /* Rasterizer.ambient_color.is_some(), :62         */
#define RXR_FLAG_HAS_SUN               (1u << 6) /* Rasterizer.sun_dir.is_some(), :86               */

/* ---- PODs ------------------------------------------------------------------------------------ */

/* one Texture (src/texture.rs:46-54): RGBA8 row-major, data[(y*width + x)*4] */
typedef struct rxr_texture {
    const uint8_t *rgba;
    uint32_t width, height;
} rxr_texture;

/* one Tile (src/map/tile.rs `textures: Vec<Texture>`): the animation frames of a tile; the raster
 * loops pick textures[animation_frame % len] (src/rasterizer.rs:1104-1105) */
typedef struct rxr_tile {
    const rxr_texture *textures;
    uint32_t n_textures;
} rxr_tile;

/* CompiledLight, src/map/light.rs:456-477, field for field */
typedef struct rxr_light {
    uint32_t light_type;
    float position[3];
    float color[3];
    float intensity;
    uint32_t emitting;
    float start_distance, end_distance, flicker;
    float direction[3];
    float cone_angle;
    float normal[3];
    float width, height;
    uint32_t from_linedef;
} rxr_light;

/* Edges, src/edge.rs:2-8.  `Edges` is repr(Rust) with private a/b/c; the shim needs the accessor
 * shown in INTEGRATION.md to fill this. */
typedef struct rxr_edges {
    float a[3], b[3], c[3];
    uint32_t visible;
} rxr_edges;

typedef struct rxr_source {
    uint32_t kind;    /* RXR_SOURCE_*            */
    uint32_t index;   /* tile index for *_TILE   */
    uint8_t pixel[4]; /* colour for RXR_SOURCE_PIXEL */
} rxr_source;

/* Batch3D after clip_and_project (src/batch/batch3d.rs:15-78, outputs of :482-740) */
typedef struct rxr_batch3d {
    const float *projected_vertices;  /* [n_vertices][4] = (screen x, screen y, ndc z, clip w), :694-699 */
    const float *clipped_uvs;         /* [n_vertices][2]                                           */
    const float *clipped_normals;     /* [n_vertices][3]; NULL iff batch.normals.is_empty() (:1083) */
    const uint32_t *clipped_indices;  /* [n_triangles][3]                                          */
    const rxr_edges *edges;           /* [n_triangles]                                             */
    uint32_t n_vertices, n_triangles;
    uint32_t has_bounding_box;        /* bounding_box.is_some(); None => batch skipped (:978)      */
    float bounding_box[4];            /* Rect x, y, width, height (src/rect.rs:5-10)               */
    uint32_t repeat_mode;
    rxr_source source;
    float ambient_color[3];
    int32_t shader;                   /* Option<usize>: -1 = None                                  */
    uint32_t has_profile_id, profile_id;
    uint32_t list;                    /* RXR_LIST_*                                                */
    int32_t chunk;                    /* index into rxr_frame.chunks, -1 for the scene-level lists */
    /* ABI 5, optional: edges == NULL.  The Edges records are the largest array of the hand-over (40 of the 124 bytes per triangle that a
     * frame of boxes sends over PCIe) and a function of arrays that travel anyway: the device then builds them itself from the projected
     * vertices -- Edges::new([v0,v1,v2],[v1,v2,v0]) behind the winding swap of `cull_mode` (src/edge.rs:12-24,
     * src/batch/batch3d.rs:706-746; the same operations in the same order: the same floats) -- and the host sends one word per
     * triangle: edge_visible[t] != 0 iff the record's `visible` (what the host would have passed to Edges::new).  Every 3D batch of a
     * frame takes the same form (all with `edges` or all without); rxr_stream_batch3d likewise. */
    const uint32_t *edge_visible;     /* [n_triangles]; read only when edges == NULL               */
    uint32_t cull_mode;               /* RXR_CULL_* of the batch; read only when edges == NULL     */
} rxr_batch3d;

/* CullMode, src/batch/mod.rs:17-26 */
enum { RXR_CULL_OFF = 0, RXR_CULL_FRONT = 1, RXR_CULL_BACK = 2 };

/* Batch3D BEFORE projection: the inputs of Batch3D::clip_and_project (src/batch/batch3d.rs:482-740).
 * Used by the device-side projection path (rxr_set_meshes + rxr_frame.use_meshes): the geometry is
 * uploaded once and every frame sends only matrices; the device then performs the view transform,
 * the near-plane clip (z < -0.1) with its appended fan triangles, the screen mapping (:689-700),
 * Edges::new with the cull-mode rule (:706-739, src/edge.rs:12-24) and the bounding box (:749-768). */
typedef struct rxr_mesh3d {
    const float *vertices;            /* [n_vertices][4]                                            */
    const uint32_t *indices;          /* [n_triangles][3]                                           */
    const float *uvs;                 /* [n_vertices][2]                                            */
    const float *normals;             /* [n_vertices][3]; required when n_triangles > 0 (the
                                         reference indexes self.normals unconditionally, :605-607)   */
    uint32_t n_vertices, n_triangles;
    float transform_3d[16];           /* Batch3D.transform_3d, column-major                         */
    uint32_t cull_mode;               /* RXR_CULL_*                                                 */
    uint32_t repeat_mode;
    rxr_source source;
    float ambient_color[3];
    int32_t shader;
    uint32_t has_profile_id, profile_id;
    uint32_t list;                    /* RXR_LIST_*                                                 */
    int32_t chunk;
} rxr_mesh3d;

/* Batch2D after project (src/batch/batch2d.rs:10-52, outputs of :373-425) */
typedef struct rxr_batch2d {
    const float *projected_vertices;  /* [n_vertices][2] */
    const float *uvs;                 /* [n_vertices][2] */
    const uint32_t *indices;          /* [n_triangles][3]; for Lines only .0/.1 are used (:902)     */
    const rxr_edges *edges;           /* [n_triangles], or NULL (ABI 5): Edges::new([v0,v1,v2],[v1,v2,v0], true) of the projected
                                         vertices, as Batch2D::project builds them (src/batch/batch2d.rs:413-424), is then built by
                                         the library                                                */
    uint32_t n_vertices, n_triangles;
    uint32_t has_bounding_box;
    float bounding_box[4];
    uint32_t mode;                    /* RXR_MODE_* */
    uint32_t repeat_mode;
    rxr_source source;
    uint32_t receives_light;
    int32_t shader;
    int32_t chunk;
} rxr_batch2d;

/* Batch2D BEFORE projection: the inputs of Batch2D::project (src/batch/batch2d.rs:373-425) -- the 2D half of the device-side
 * projection path (rxr_set_meshes2d + rxr_frame.use_meshes bit 1): the geometry is uploaded once, every frame sends the optional
 * Mat3 (rxr_set_projection2d), and the device applies it, accumulates the bounding box (f32::min / f32::max: NaN dropped),
 * builds the Edges (src/edge.rs:12-24) and the clamped pixel boxes (src/rasterizer.rs:615-634, :1777-1821). */
typedef struct rxr_mesh2d {
    const float *vertices;            /* [n_vertices][2]                                            */
    const uint32_t *indices;          /* [n_triangles][3]; Lines read .0/.1 only (:902)             */
    const float *uvs;                 /* [n_vertices][2]                                            */
    uint32_t n_vertices, n_triangles;
    uint32_t mode;                    /* RXR_MODE_* */
    uint32_t repeat_mode;
    rxr_source source;
    uint32_t receives_light;
    int32_t shader;
    int32_t chunk;
} rxr_mesh2d;

/* (BBox, occlusion) entry of MapMini.occluded_sectors / Chunk.occluded_sectors
 * (src/map/mini.rs:58-66, src/chunk.rs:154-161, src/map/bbox.rs:35-40) */
typedef struct rxr_occluder {
    float min[2], max[2];
    float occlusion;
} rxr_occluder;

/* CompiledLinedef start/end as used by MapMini::is_visible (src/map/mini.rs:68-95) */
typedef struct rxr_linedef {
    float start[2], end[2];
} rxr_linedef;

/* the per-chunk data the raster loops read (src/chunk.rs); chunks in the host's iteration order */
typedef struct rxr_chunk {
    const rxr_occluder *occluders;    /* chunk.occluded_sectors (src/chunk.rs:42)                  */
    uint32_t n_occluders;
    /* chunk.shaders (src/chunk.rs:51): programs[program_base .. program_base + n_programs) of the set given to
     * rxr_set_shaders; a chunk batch's `shader` indexes this range (src/rasterizer.rs:763, :1285, :1645) */
    uint32_t program_base, n_programs;
    /* chunk.shader_textures (src/chunk.rs:53): the baked texture of shader i replaces the texel of a 3D
     * opaque-pass batch whose shader == i, and the program does not run (src/rasterizer.rs:1226-1267);
     * rgba == NULL for None */
    const rxr_texture *shader_textures;
    uint32_t n_shader_textures;
    /* chunk.terrain_texture (NULL = None), chunk.origin, chunk.size: what PixelSource::Terrain batches of
     * this chunk sample by world position (src/chunk.rs:133-151) */
    const rxr_texture *terrain_texture;
    int32_t origin[2];
    int32_t size;
} rxr_chunk;

/* everything `rasterize` reads from `self` and `scene` after projection */
typedef struct rxr_frame {
    uint32_t abi_version;             /* RXR_ABI_VERSION                                           */
    uint32_t width, height;           /* framebuffer size in pixels                                */
    uint32_t tile_size;               /* the caller's tile_size; accepted for API parity only: the
                                         result does not depend on it   */
    float inverse_view[16];           /* Rasterizer.inverse_view_matrix, :43, :97                  */
    float inverse_projection[16];     /* Rasterizer.inverse_projection_matrix, :44, :116           */
    float camera_pos[3];              /* :98-102                                                   */
    float translationd2[2];           /* :104-110                                                  */
    float scaled2;
    uint32_t hash_anim;               /* hash_u32(animation_frame), :199-208                       */
    uint64_t animation_frame;         /* scene.animation_frame (usize)                             */
    uint32_t flags;                   /* RXR_FLAG_*                                                */
    uint8_t background_color[4];
    float ambient[4];
    float sun_dir[3];
    float day_factor;
    uint32_t sample_mode;             /* RXR_SAMPLE_*; rasterizer-wide (:1119)                     */
    float time;
    uint32_t background_kind;         /* RXR_BG_*; only read when D3 is off or pixel is... see :292 */
    const uint8_t *background_pixels; /* RXR_BG_HOST_PIXELS: width*height*4                        */

    const rxr_batch3d *batches3d;     /* submission order, src/rasterizer.rs:314-405               */
    uint32_t n_batches3d;
    const rxr_batch2d *batches2d;     /* submission order, :503-552                                */
    uint32_t n_batches2d;
    const rxr_light *lights;          /* scene.lights followed by scene.dynamic_lights (:1373)     */
    uint32_t n_lights;
    const rxr_occluder *occluders;    /* Rasterizer.mapmini.occluded_sectors                       */
    uint32_t n_occluders;
    const rxr_linedef *linedefs;      /* Rasterizer.mapmini.linedefs                               */
    uint32_t n_linedefs;
    const rxr_chunk *chunks;
    uint32_t n_chunks;
    uint32_t n_shader_programs;       /* scene.shaders.len(); a batch whose shader index resolves
                                         to a program makes the call return RXR_ERR_UNSUPPORTED     */
    /* device-side projection: when use_meshes != 0 the 3D batches are the meshes
     * registered with rxr_set_meshes (batches3d must then be empty) and are projected on the device
     * with these matrices, replacing Scene::project's 3D half (src/scene.rs:189-199).
     * Bit 1 (value 2, alone or with bit 0): the 2D batches are the meshes registered with rxr_set_meshes2d (batches2d must then be
     * empty), projected on the device with the matrix of rxr_set_projection2d: Scene::project's 2D half (:163-187) */
    uint32_t use_meshes;
    float view[16];                   /* Rasterizer.view_matrix, :40                               */
    float projection[16];             /* Rasterizer.projection_matrix, :41                         */
    const float *mesh_transforms;     /* optional [n_meshes][16]: this frame's Batch3D.transform_3d of
                                         every registered mesh (moving objects need no re-registration);
                                         NULL = the transforms given to rxr_set_meshes                */
    /* ABI 3 */
    float background_grid[4];         /* RXR_BG_GRID: GridShader.grid_size, .subdivisions, .offset.x, .offset.y
                                         (src/shader/grid.rs:4-8; defaults 30, 2, (0, 0), :12-16)      */
    uint32_t has_brush_preview;       /* Rasterizer.brush_preview.is_some() (src/rasterizer.rs:13-17, :65): the editor's terrain
                                         brush, blended over the pixels no 3D fragment reached (:435-458) and into the terrain
                                         texels of chunk batches (:1192-1213, :1601-1622)               */
    float brush_position[3];
    float brush_radius, brush_falloff;
} rxr_frame;

/* ---- Rusteria shader programs -------------------------------------
 * A program is handed over as the reference's NodeOp tree (rusteria/src/node/nodeop.rs:12-103),
 * serialised depth-first into 32-bit words; opcodes are the NodeOp variants in declaration order:
 *   node := opcode [payload]
 *   LoadGlobal / StoreGlobal / LoadLocal / StoreLocal : index
 *   GetComponents / SetComponents                     : n, then n component indices (one per word)
 *   If                                                : then_len, has_else, else_len, then-block, else-block
 *   For                                               : init_len, cond_len, incr_len, body_len, the four blocks
 *   Push                                              : the f32 bits of x, y, z
 *   FunctionCall                                      : arity, total_locals, function index
 *   every other variant                               : no payload
 * (block lengths in words).  The library flattens the tree into jump code for the device. */
enum {
    RXR_NODE_LOAD_GLOBAL = 0, RXR_NODE_STORE_GLOBAL, RXR_NODE_LOAD_LOCAL, RXR_NODE_STORE_LOCAL, RXR_NODE_SWAP,
    RXR_NODE_GET_COMPONENTS, RXR_NODE_SET_COMPONENTS, RXR_NODE_IF, RXR_NODE_FOR, RXR_NODE_PUSH, RXR_NODE_FUNCTION_CALL,
    RXR_NODE_RETURN, RXR_NODE_DUP, RXR_NODE_CLEAR, RXR_NODE_PACK2, RXR_NODE_PACK3, RXR_NODE_ADD, RXR_NODE_SUB, RXR_NODE_MUL,
    RXR_NODE_DIV, RXR_NODE_LENGTH, RXR_NODE_LENGTH2, RXR_NODE_LENGTH3, RXR_NODE_ABS, RXR_NODE_SIN, RXR_NODE_SIN1,
    RXR_NODE_SIN2, RXR_NODE_COS, RXR_NODE_COS1, RXR_NODE_COS2, RXR_NODE_TAN, RXR_NODE_ATAN, RXR_NODE_ATAN2,
    RXR_NODE_ROTATE2D, RXR_NODE_DOT, RXR_NODE_DOT2, RXR_NODE_DOT3, RXR_NODE_CROSS, RXR_NODE_NORMALIZE, RXR_NODE_FLOOR,
    RXR_NODE_CEIL, RXR_NODE_ROUND, RXR_NODE_FRACT, RXR_NODE_MOD, RXR_NODE_DEGREES, RXR_NODE_RADIANS, RXR_NODE_MIN,
    RXR_NODE_MAX, RXR_NODE_MIX, RXR_NODE_SMOOTHSTEP, RXR_NODE_STEP, RXR_NODE_CLAMP, RXR_NODE_SQRT, RXR_NODE_POW,
    RXR_NODE_LOG, RXR_NODE_PRINT, RXR_NODE_EQ, RXR_NODE_NE, RXR_NODE_LT, RXR_NODE_LE, RXR_NODE_GT, RXR_NODE_GE,
    RXR_NODE_AND, RXR_NODE_OR, RXR_NODE_NOT, RXR_NODE_NEG, RXR_NODE_UV, RXR_NODE_SET_UV, RXR_NODE_NORMAL,
    RXR_NODE_SET_NORMAL, RXR_NODE_HITPOINT, RXR_NODE_TIME, RXR_NODE_SAMPLE, RXR_NODE_SAMPLE_NORMAL, RXR_NODE_COLOR,
    RXR_NODE_SET_COLOR, RXR_NODE_ROUGHNESS, RXR_NODE_SET_ROUGHNESS, RXR_NODE_METALLIC, RXR_NODE_SET_METALLIC,
    RXR_NODE_EMISSIVE, RXR_NODE_SET_EMISSIVE, RXR_NODE_OPACITY, RXR_NODE_SET_OPACITY, RXR_NODE_BUMP, RXR_NODE_SET_BUMP,
    RXR_NODE_ALLOC, RXR_NODE_ITERATE, RXR_NODE_SAVE, RXR_NODE_PALETTE_INDEX, RXR_NODE_COUNT
};

/* one user function: Arc<[NodeOp]> (rusteria/src/node/program.rs:15) */
typedef struct rxr_function {
    const uint32_t *words;
    uint32_t n_words;
} rxr_function;

/* rusteria::Program (rusteria/src/node/program.rs:7-29); `body` and `strings` are not read by the raster path */
typedef struct rxr_program {
    uint32_t n_globals;               /* Program.globals                                            */
    int32_t shade_index;              /* Program.shade_index; -1 = None (the batch then shades as if it had no shader) */
    uint32_t shade_locals;            /* Program.shade_locals                                       */
    const rxr_function *functions;    /* Program.user_functions                                     */
    uint32_t n_functions;
} rxr_program;

/* TexStorage of the global pattern bank (rusteria/src/textures/mod.rs:10-15): width*height RGB f32 */
typedef struct rxr_pattern {
    const float *rgb;
    uint32_t width, height;
} rxr_pattern;

typedef struct rxr_shader_set {
    const rxr_program *programs;      /* scene.shaders (src/scene.rs:43), indexed by rxr_batch*.shader */
    uint32_t n_programs;
    const rxr_pattern *patterns;      /* rusteria::textures::patterns::patterns(), read by NodeOp::Sample */
    uint32_t n_patterns;
    const rxr_pattern *normal_patterns; /* patterns_normal(), read by NodeOp::SampleNormal          */
    uint32_t n_normal_patterns;
    const float *palette_rgb;         /* assets.palette.colors as [n][3] (TheColor::to_vec3)        */
    const uint8_t *palette_present;   /* [n]: 0 where the palette slot is None                      */
    uint32_t n_palette;
} rxr_shader_set;

/* the last rendered frame.  The *_us fields (microseconds) are only measured while profiling is on (rxr_profile_begin with n > 0)
 * and are 0 otherwise: the sum of the set-up kernels' durations and the raster kernel's, each taken from a start / stop HIP event pair
 * bound to the dispatch itself (see rxr_profile_begin). */
typedef struct rxr_stats {
    float setup_us;      /* triangle set-up + binning kernels */
    float raster_us;     /* the tile raster / shade kernel    */
    float total_us;      /* first kernel start .. last kernel end */
    uint32_t n_triangles3d, n_triangles2d, n_bin_entries;
    uint32_t tiles_x, tiles_y;
} rxr_stats;

typedef struct rxr_ctx rxr_ctx;

/* ---- entry points ----------------------------------------------------------------------------
 * Each replaces a slice of Rasterizer::rasterize (src/rasterizer.rs:185-580):                     */

/* creates a context on HIP device `device_id` (no reference counterpart -- the reference uses rayon's global pool,
 * src/rasterizer.rs:273-275) */
int rxr_create(rxr_ctx **out, int device_id);
void rxr_destroy(rxr_ctx *ctx);

/* ABI 4.  A multi-device context: one member context per entry of device_ids (a device may be listed more than once: N
 * logical members on one GPU, which is how the single-GPU tests check byte identity), driven from this one process.  The
 * reference renders tiles independently and concatenates them at the end (src/rasterizer.rs:273-275, :559-579); this does
 * the same across GPUs.  On such a handle
 *   - rxr_set_textures / rxr_set_meshes / rxr_set_shaders / rxr_upload_frame replicate to every member (in parallel, one
 *     host thread and one PCIe link per device);
 *   - rxr_rasterize / rxr_render_download shard the frame by interleaved RXR_STRIPE_ROWS-row stripes (member i of N renders
 *     stripes i, i+N, ...) and EVERY device copies its own stripes straight into the caller's `pixels`;
 *   - rxr_render_gather assembles the frame in the memory of one member's device instead (peer copies over xGMI);
 *   - rxr_synchronize / rxr_get_stats / rxr_last_error cover all members; rxr_profile_* and rxr_selftest_math refer to
 *     member 0; the single-device calls that take device pointers, streams or row ranges (rxr_render_rows*,
 *     rxr_render_stripes_to, rxr_download_rows) return RXR_ERR_UNSUPPORTED -- use them on rxr_member(ctx, i).
 * The result is byte-identical to the single-device frame (tests/test_gpu_multi.py). */
int rxr_create_multi(rxr_ctx **out, const int *device_ids, int n_devices);
/* 1 for a plain context, the number of members for a multi-device one */
int rxr_member_count(const rxr_ctx *ctx);
/* member `index` of a multi-device context (owned by it; never destroy it), or `ctx` itself for index 0 of a plain one */
rxr_ctx *rxr_member(rxr_ctx *ctx, int index);

/* optional: page-locks the caller's pixel buffer (hipHostRegister, visible to every device) so that the downloads of
 * rxr_rasterize / rxr_render_download are direct DMA.  Unpinned buffers work too (the runtime locks them on the fly per copy).
 * Lock WHOLE PAGES of a mapping the buffer has to itself (an allocation of its own from mmap / posix_memalign(4096, ..) / a Vec with
 * page alignment; or take the memory from rxr_alloc_pinned and lock nothing): pages in the middle of the malloc heap are shared with
 * other allocations and reused by them after the buffer is freed, and a copy into such a page shortly after the unlock has been seen to
 * end in a GPU memory access fault on this runtime.  Unlock before the memory is freed. */
int rxr_pin_host_buffer(rxr_ctx *ctx, void *ptr, size_t bytes);
int rxr_unpin_host_buffer(rxr_ctx *ctx, void *ptr);
/* last error text for this context (or for rxr_create when ctx == NULL) */
const char *rxr_last_error(const rxr_ctx *ctx);
/* number of visible HIP devices, 0 if none (never fails) */
int rxr_device_count(void);

/* uploads assets.tile_list (static) and scene.dynamic_textures (dynamic); replaces the texture
 * reads at src/rasterizer.rs:1103-1137 / :674-704.  Call again only when the textures change. */
int rxr_set_textures(rxr_ctx *ctx, const rxr_tile *static_tiles, uint32_t n_static,
                     const rxr_tile *dynamic_tiles, uint32_t n_dynamic);

/* registers the object-space 3D batches of a scene for device-side projection (submission order).
 * Replaces nothing per frame: it is the one-time hand-over of what Batch3D::clip_and_project reads
 * from `self` (src/batch/batch3d.rs:482-740).  Call again only when geometry or materials change. */
int rxr_set_meshes(rxr_ctx *ctx, const rxr_mesh3d *meshes, uint32_t n_meshes);

/* Replaces the geometry of n ALREADY REGISTERED meshes in place, from host memory, when their counts are unchanged (a height stroke on a
 * terrain chunk moves vertices and normals, not which cells exist).  The layout is exactly what rxr_terrain_meshes[_to] writes, so its
 * output feeds this call with no repacking: counts [n][2] = vertices, triangles of mesh_indices[i]; vertices [n][vertex_stride][4];
 * indices [n][triangle_stride][3], mesh-local; normals [n][vertex_stride][3].  Slots past a mesh's counts are never read.
 * mesh_indices indexes the meshes in rxr_set_meshes order.  uvs, transform, cull mode, source, shader, list and chunk stay as
 * registered; so do every other mesh and every prefix array.
 * Accepted only if, for every i, counts[i] equals the registered (n_vertices, n_triangles) of mesh_indices[i] and every index is below
 * that vertex count; anything else is RXR_ERR_INVALID, the message names the first offending mesh and why, and NOTHING HAS BEEN
 * CHANGED -- not the pools, not the boxes, not a previously uploaded frame: the caller then falls back to rxr_set_meshes.  Also
 * RXR_ERR_INVALID: no valid registration, a mesh index out of range or named twice, a NULL pointer with n > 0 (an array of 0 bytes
 * -- a stride of 0 -- is not looked at), a stride below a named mesh's registered count, byte sizes that overflow.  n == 0 does nothing.
 * After success the object-space pools and the static originals of clipped_indices / clipped_normals hold the new values, the
 * context's object-space box of each named mesh is the new one (f32::min / f32::max over the vertices, a NaN coordinate ignored;
 * equal to the host loop's under ==, the sign of a zero bound is not specified), the pick records are rebuilt by the next
 * rxr_intersect, and THE RESIDENT FRAME IS DROPPED: upload it again, as after rxr_set_meshes.
 * Blocking: the call first waits for everything the context has queued (renders and picks read the pools) and returns once the pools
 * are updated, so work queued later on any stream sees the new geometry.  All arrays are read before it returns.  The checks run on
 * the device (k_mesh_check: counts, indices, box; one 32-byte record per mesh comes back), then k_mesh_commit writes.
 * Multi-device handles: every member.
 * Replaces, for the named meshes: the object-space box of batch3d.rs:494-507 (rxr_set_meshes' host loop) and the static copies of
 * batch3d.rs:566-574 (k_proj_static). */
int rxr_update_meshes(rxr_ctx *ctx, const uint32_t *mesh_indices, uint32_t n, const uint32_t *counts, const float *vertices,
                      const uint32_t *indices, const float *normals, uint32_t vertex_stride, uint32_t triangle_stride);
/* the same from DEVICE arrays (each one's first and last byte are checked to be memory of the context's device; 4-byte aligned: else
 * RXR_ERR_INVALID); mesh_indices is host memory and is read before the call returns.  The kernels are queued on hip_stream (NULL = the
 * context's stream), so the call is ordered behind the rxr_terrain_meshes_to on that stream that produced its inputs, and no geometry
 * crosses PCIe.  BLOCKING like the host form: it waits for the context's queued work, synchronises hip_stream for the read-back of
 * the n 32-byte check records, and again behind the writes.  Multi-device handles: RXR_ERR_UNSUPPORTED (use rxr_member).
 * Replaces: as rxr_update_meshes (batch3d.rs:494-507, :566-574). */
int rxr_update_meshes_to(rxr_ctx *ctx, const uint32_t *mesh_indices, uint32_t n, const uint32_t *dev_counts, const float *dev_vertices,
                         const uint32_t *dev_indices, const float *dev_normals, uint32_t vertex_stride, uint32_t triangle_stride,
                         void *hip_stream);
/* Replaces the geometry of n ALREADY REGISTERED meshes when their COUNTS CHANGE (an excluded sector added or removed, a tile override
 * painted, a terrain cell added or removed): what rxr_update_meshes refuses.  The layout is that of rxr_update_meshes with one more
 * array: counts [n][2] = the NEW vertices, triangles of mesh_indices[i] (they may grow, shrink, become 0 or stop being 0); vertices
 * [n][vertex_stride][4]; uvs [n][vertex_stride][2], or NULL: every uv of the named meshes is [0, 0] (TerrainChunk::build_mesh;
 * rxr_terrain_meshes[_to] writes no uv array); indices [n][triangle_stride][3], mesh-local; normals [n][vertex_stride][3].  Slots past a
 * mesh's own counts are never read, so rxr_generated_tile_meshes[_to]'s output feeds the call with no repacking.  Transform, cull mode,
 * repeat mode, source, ambient, shader, profile id, list and chunk stay as registered, and so do the number and the order of the meshes.
 * After success the context is in the state rxr_set_meshes of the whole scene with the new geometry would have left: the object-space
 * pools, the prefix arrays and the mesh table with every later mesh's bases moved, output pools and scratch of the new sizes with the
 * static originals written (k_proj_static), every box (the named ones as rxr_update_meshes computes them: equal to the host loop's
 * under ==), and -- exactly as after rxr_set_meshes -- NO RESIDENT FRAME, no pick records, no box tree, no pending ranged refresh and
 * no trace scene: upload the frame again, call rxr_set_trace_scene again before tracing; the next query rebuilds its records.
 * RXR_ERR_INVALID, with the message naming the first offending mesh and why, and NOTHING CHANGED (pools, boxes, the resident frame, the
 * pick records and a pending refresh all stay): no valid registration, a mesh index out of range or named twice, a NULL pointer other
 * than uvs with n > 0 (an array of 0 bytes -- a stride of 0 -- is not looked at), byte sizes that overflow, a count above its stride,
 * an index that is not below the new vertex count, new totals that reach rxr_set_meshes' limit of 2^31 output slots.  n == 0 does nothing.
 * Once the checks have passed, a failure to allocate the new object pools leaves the old registration in use; any later failure (the
 * output pools, a HIP error) leaves the context WITHOUT a valid registration, as a failed rxr_set_meshes does: register again.
 * Blocking like rxr_update_meshes: it waits for everything the context has queued, reads one 40-byte check record per named mesh back
 * (k_mesh_resize_check: counts against strides, indices, box; the host reads the counts nowhere else) and returns behind the writes.
 * The object pools are double-buffered: k_mesh_repack copies unnamed meshes from the old pools and named ones from the caller's arrays
 * into a second blob, which replaces the first at the end.  Multi-device handles: every member.
 * Replaces, for the whole registration: rxr_set_meshes (its host loop over batch3d.rs:494-507 and its copy of the scene over PCIe). */
int rxr_resize_meshes(rxr_ctx *ctx, const uint32_t *mesh_indices, uint32_t n, const uint32_t *counts, const float *vertices, const float *uvs,
                      const uint32_t *indices, const float *normals, uint32_t vertex_stride, uint32_t triangle_stride);
/* the same from DEVICE arrays (dev_counts too: each one's first and last byte are checked to be memory of the context's device, 4-byte
 * aligned, else RXR_ERR_INVALID; dev_uvs may be NULL); mesh_indices is host memory and is read before the call returns.  Everything is
 * queued on hip_stream (NULL = the context's stream), so the call is ordered behind the work on that stream that produced its inputs
 * (rxr_generated_tile_meshes_to -> rxr_vertex_normals_to -> rxr_resize_meshes_to), and no geometry crosses PCIe.  BLOCKING like the
 * host form.  Multi-device handles: RXR_ERR_UNSUPPORTED (use rxr_member). */
int rxr_resize_meshes_to(rxr_ctx *ctx, const uint32_t *mesh_indices, uint32_t n, const uint32_t *dev_counts, const float *dev_vertices,
                         const float *dev_uvs, const uint32_t *dev_indices, const float *dev_normals, uint32_t vertex_stride,
                         uint32_t triangle_stride, void *hip_stream);
/* debugging / tests: the object-space box the context currently holds for mesh `mesh_index` (batch3d.rs:494-507), whether it came from
 * rxr_set_meshes or from an update; (+inf, -inf) for a mesh without vertices.  Multi-device handles: member 0. */
int rxr_mesh_bounds(rxr_ctx *ctx, uint32_t mesh_index, float lo[3], float hi[3]);

/* The 2D half of the same: registers the object-space 2D batches of a scene (submission order, src/rasterizer.rs:503-552) for
 * device-side projection; what Batch2D::project reads from `self` (src/batch/batch2d.rs:373-425).  Call again only when geometry
 * or materials change.  A batch whose texture tile does not exist is refused HERE (the reference panics only when the batch is on
 * screen: the device does not know that before it has projected it). */
int rxr_set_meshes2d(rxr_ctx *ctx, const rxr_mesh2d *meshes, uint32_t n_meshes);
/* the `matrix: Option<Mat3<f32>>` of Batch2D::project for the uploads that follow: nine floats in vek's column-major order
 * (m[c * 3 + r]), or NULL for None (vertices are used as they are) */
int rxr_set_projection2d(rxr_ctx *ctx, const float *mat3);

/* debugging / tests: copies the device-projected arrays of mesh `index` (as produced for the last
 * rendered frame) back to the host in the layout of rxr_batch3d.  Any pointer may be NULL.
 * counts[0] = vertices (originals + appended), counts[1] = triangles (originals + appended). */
int rxr_read_projected_mesh(rxr_ctx *ctx, uint32_t index, uint32_t counts[2], float *projected_vertices, float *clipped_uvs,
                            float *clipped_normals, uint32_t *clipped_indices, rxr_edges *edges, float bounding_box[5],
                            uint32_t capacity_vertices, uint32_t capacity_triangles);
/* debugging / tests: the 16-pixel tile rows [out[0], out[1]) of the resident frame that any 3D triangle can reach, as rxr_upload_frame
 * found them from the triangles' edge functions (small host-projected frames whose set-up records it builds; the raster kernel of such
 * a frame skips the 3D passes outside them); 0, 0xFFFFFFFF when the range is "all rows" (every other frame, RXR_D3_ROWS=0, a brush
 * preview); 0, 0 when no triangle reaches any row.  -1: no context, a multi-device handle or no frame. */
int rxr_debug_d3_rows(rxr_ctx *ctx, uint32_t out[2]);

/* replaces the context's shader programs, pattern bank and palette (stay resident until the next call;
 * NULL or an empty set removes them).  Programs are restricted to what a per-fragment evaluation can
 * reproduce: RXR_ERR_UNSUPPORTED for Alloc / Iterate / Save, for SetEmissive (the
 * reference leaks it into every later fragment of the tile), for a local of `shade` or a global that is
 * read before the same invocation wrote it (the reference resizes, never clears them) and for Return inside
 * For (the reference unwinds that incorrectly).
 * Replaces: Execution::shade per fragment, src/rasterizer.rs:760-800, :1283-1304, :1642-1667. */
int rxr_set_shaders(rxr_ctx *ctx, const rxr_shader_set *set);
/* the validation half of rxr_set_shaders without a device (no context needed): same status codes; on failure `message`
 * receives the reason; code_words (optional) the length of the flattened jump code.  Lets a host decide up front whether
 * a scene's programs can run on the device or must take the CPU path. */
int rxr_check_shaders(const rxr_shader_set *set, uint32_t *code_words, char *message, uint32_t message_capacity);

/* Arithmetic of the 3D direct-light loop (src/rasterizer.rs:1373-1391 with CompiledLight::radiance_at, src/map/light.rs:491-552,
 * and shade_fast_brdf, :1875-1951), applied from the next rxr_upload_frame on:
 *   RXR_LIGHT_MATH_RELAXED (the default)  in frames with a 3D light loop, point lights are one fused term (fused multiply-adds,
 *       v_rsq_f32 normalisations, the smoothstep divided by a reciprocal), view direction, normal and -- without occluders -- the
 *       world position go through reciprocals, the encode through v_sqrt_f32: every operand within a few ulp of the reference's
 *       correctly rounded value.  Every quantity
 *       of that path is continuous in the fragment's position (range test, smoothstep, Lambert and specular cut-offs all meet
 *       zero), so a channel moves by at most one 8-bit step -- the tolerance BASELINE.json states for lit 3D fragments; measured:
 *       112 of 8 294 400 pixels of the bench frame differ from the oracle, each by 1.  Spot / area / daylight lights (hard
 *       cut-offs), unlit frames, 2D frames and frames that run Rusteria programs are computed exactly in both modes.
 *   RXR_LIGHT_MATH_EXACT  the reference's operations, correctly rounded, throughout (bit-identical to the CPU oracle up to the
 *       libm-dependent pow; 35 % slower on the bench frame).
 * The environment variable RXR_LIGHT_MATH=exact|relaxed, when set, overrides the context's mode (read at every upload).
 * RXR_ERR_INVALID for another mode.  On a multi-device context: every member.  Nothing in the reference corresponds to it. */
#define RXR_LIGHT_MATH_EXACT 0
#define RXR_LIGHT_MATH_RELAXED 1
int rxr_set_light_math(rxr_ctx *ctx, int mode);

/* Streaming hand-over for large scenes (an addition to ABI 4; optional -- rxr_upload_frame alone does the same, later).
 * The reference projects a scene's batches in parallel (Scene::project: rayon par_iter_mut, src/scene.rs:154-200) and only then
 * walks the tiles; with the tiles on the GPU, projecting a million triangles and THEN copying 124 MB to the device takes the host
 * longer than the GPU needs for ten frames.  A host that projects batch by batch hands each 3D batch over as soon as its
 * clip_and_project is done, from whatever thread did it:
 *     rxr_stream_begin(ctx, n, vertex_capacity, triangle_capacity)   n = the frame's number of 3D batches (rxr_frame.batches3d, same
 *                             order); capacity[i] = an upper bound of what projecting batch i can produce (vertices: n + 4 m,
 *                             triangles: 3 m for a batch of n vertices and m triangles covers the near-plane clip, batch3d.rs:627-686).
 *                             Waits for the previous frame's renders.
 *     rxr_stream_batch3d(ctx, i, &projected)      thread-safe, any order; only the five arrays and the two counts are read.  The arrays
 *                             must stay unchanged until rxr_upload_frame has returned.  Batches are retired in index order (a batch's
 *                             place in the pools -- hence the submission order of its triangles, which breaks depth ties -- is the sum
 *                             of its predecessors' sizes), copied into pinned memory and sent to the device in groups, while the
 *                             host projects the batches behind them.
 *     rxr_upload_frame(ctx, &frame)               as always, with frame.batches3d[i] naming the SAME arrays and counts: it then only
 *                             adds what surrounds them.  If anything differs (a batch missing, other pointers, a capacity exceeded)
 *                             the frame is handed over from scratch as if nothing had been streamed: correct either way.
 * Measured (1 M triangles, 7680x4320, 64 host threads, profiles/r03/c5_e2e_breakdown.jsonl): the call Rasterizer::rasterize 14.1 ms
 * (one copy and one transfer after the projection) -> 10.6 (rxr_upload_frame's own pipelined copy) -> 8.7 (streamed, ordinary
 * arrays) -> 6.4 ms (streamed, page-locked arrays: rxr_stream_begin_pinned below).
 * Multi-device handles: RXR_ERR_UNSUPPORTED (use rxr_upload_frame). */
int rxr_stream_begin(rxr_ctx *ctx, uint32_t n_batches3d, const uint32_t *vertex_capacity, const uint32_t *triangle_capacity);
/* The same with a promise: EVERY array handed to rxr_stream_batch3d lies in page-locked host memory that the device can read
 * (rxr_alloc_pinned below, hipHostMalloc, or memory registered with rxr_pin_host_buffer / hipHostRegister -- each array inside ONE
 * registration; the device reads through the device address the runtime reports for it, which for registered memory need not be
 * the host address).  The library then
 * copies nothing on the host: a kernel on the device pulls each group of batches straight out of the caller's arrays over PCIe
 * into the pools.  A pointer that breaks the promise is a device page fault -- only promise what an allocator guarantees. */
int rxr_stream_begin_pinned(rxr_ctx *ctx, uint32_t n_batches3d, const uint32_t *vertex_capacity, const uint32_t *triangle_capacity);
/* page-locked, device-readable host memory for a host's projected arrays (NULL when there is no device or no memory: fall back to
 * ordinary memory and rxr_stream_begin).  No context needed; free with rxr_free_pinned. */
void *rxr_alloc_pinned(size_t bytes);
void rxr_free_pinned(void *ptr);
int rxr_stream_batch3d(rxr_ctx *ctx, uint32_t index, const rxr_batch3d *projected);

/* validates + flattens a projected frame and copies it to HBM (replaces nothing in the reference:
 * it is the host->device hand-over).  The frame stays resident until the next upload. */
int rxr_upload_frame(rxr_ctx *ctx, const rxr_frame *frame);

/* renders rows [row0,row1) of the resident frame into the context's device framebuffer.
 * Replaces the tile list + rayon tile loop, src/rasterizer.rs:256-557.  Asynchronous. */
int rxr_render_rows(rxr_ctx *ctx, uint32_t row0, uint32_t row1);
/* same, but writes the band into caller-owned DEVICE memory (`dev_pixels` points at row `row0`,
 * rows are `width*4` bytes apart) on HIP stream `hip_stream` (hipStream_t; NULL means the context's own
 * non-blocking stream, NOT the legacy default stream -- pass an explicit stream to order with other work).
 * Used by the multi-GPU host, which then gathers the bands with RCCL.
 * Streams: a context has ONE set of scratch buffers, so a render on another stream than the context's previous render is ordered
 * behind that stream -- behind the earlier render AND whatever the caller queued on that stream after it (the event is recorded at the
 * switch, not after every render).  A caller that alternates streams must therefore not make later work of the OLD stream wait for
 * something the NEW stream produces: that wait would be circular.  Callers that stay on one stream, and lanes (one member context per
 * stream, rxr_create_multi), never meet the rule. */
int rxr_render_rows_to(rxr_ctx *ctx, uint32_t row0, uint32_t row1, void *dev_pixels, void *hip_stream);

/* multi-GPU sharding primitive: renders every `stride`-th stripe of RXR_STRIPE_ROWS pixel rows,
 * starting at stripe `first`, into a COMPACT caller-owned DEVICE buffer: local stripe j (frame rows
 * (first + j*stride)*RXR_STRIPE_ROWS ...) lands at dev_pixels + j*RXR_STRIPE_ROWS*width*4.  The
 * buffer must hold ceil((n_stripes - first) / stride) stripes.  Rank r of N renders (first=r,
 * stride=N); the compact buffers are then all-gathered (RCCL) and de-interleaved. */
#define RXR_STRIPE_ROWS 16u
int rxr_render_stripes_to(rxr_ctx *ctx, uint32_t first, uint32_t stride, void *dev_pixels, void *hip_stream);

/* K frames with one host call: renders the resident frame's stripes (first, stride: as rxr_render_stripes_to) `n_frames` times;
 * frame k's compact stripe buffer lands at dev_pixels + k * frame_stride_bytes (frame_stride_bytes >= one compact buffer), and the
 * batch is complete on `hip_stream` (NULL: the context's own stream).  A rank's share of a small frame is tens of microseconds of
 * GPU work -- less than the host spends on a call per frame plus a collective per frame -- so a multi-GPU host renders a bucket of
 * frames per call and exchanges the bucket with one collective (bench.py --bucket).
 * On a multi-device handle whose members ALL sit on one device (rxr_create_multi with the same id L times: "lanes", L frames in
 * flight on that GPU) frame k is rendered by member k mod L on that member's own stream: every member has its own resident frame
 * and scratch, so consecutive frames overlap on the GPU -- the tail of one launch sequence, when most of the chip is already idle,
 * runs under the head of the next (a 1/8 share of the 4K bench frame: 31 us per frame on one stream, 17.5 us with two lanes,
 * profiles/r03/).  The lanes' streams are forked from and joined to `hip_stream` with events.  Members on different devices:
 * RXR_ERR_UNSUPPORTED.  Every frame of the batch is byte-identical to rxr_render_stripes_to's.  Asynchronous; rxr_synchronize
 * waits for it.  The reference has no counterpart: it renders one frame per call (src/rasterizer.rs:185-193). */
int rxr_render_stripes_batch(rxr_ctx *ctx, uint32_t first, uint32_t stride, uint32_t n_frames, void *dev_pixels, size_t frame_stride_bytes,
                             void *hip_stream);

/* per-launch kernel timing for the benchmark: after rxr_profile_begin(ctx, n) every kernel of a render is launched with a start /
 * stop HIP event pair of its own (hipExtLaunchKernel, on the stream the render launches on) into a ring of n slots: the runtime
 * fills the pair with the dispatch's begin / end timestamps, the figures a profiler's kernel trace shows.  rxr_profile_read
 * synchronizes and returns, per sampled render, the SUM of its set-up kernels' durations and its raster kernel's, in microseconds
 * (time between kernels is in neither).  Nothing is recorded on the stream between the launches (rounds 1-3 did: each record is a
 * barrier packet that idles the GPU for microseconds and counts launch latency as kernel time).
 * rxr_profile_begin(ctx, 0) switches the timing off again (the default). */
int rxr_profile_begin(rxr_ctx *ctx, uint32_t max_frames);
/* sample every `stride`-th render only (default 1) */
int rxr_profile_stride(rxr_ctx *ctx, uint32_t stride);
int rxr_profile_read(rxr_ctx *ctx, float *setup_us, float *raster_us, uint32_t capacity, uint32_t *n_out);

/* copies rows [row0,row1) of the context's framebuffer into host `pixels` (full-frame layout:
 * row r goes to pixels + r*width*4).  Replaces the serial tile->framebuffer copy, :559-579.
 * Blocks until the bytes have landed. */
int rxr_download_rows(rxr_ctx *ctx, uint8_t *pixels, uint32_t row0, uint32_t row1);

/* the whole drop-in call: upload + render all rows + download.  `pixels` is width*height*4 bytes
 * of host memory, fully overwritten, as in the reference (src/rasterizer.rs:185-193). */
int rxr_rasterize(rxr_ctx *ctx, const rxr_frame *frame, uint8_t *pixels);
/* the second half of rxr_rasterize for callers that upload separately: renders every row of the uploaded frame and
 * writes width*height*4 bytes to `pixels` (host memory).  Frames that need no per-tile lists (at most 128 3D triangles,
 * few 2D primitives) are rendered in bands whose downloads overlap the rendering of the following bands; the result is
 * byte-identical to rxr_render_rows + rxr_download_rows.  Replaces src/rasterizer.rs:256-579 + the final copy. */
int rxr_render_download(rxr_ctx *ctx, uint8_t *pixels);

/* device-resident consumers: renders the whole uploaded frame and leaves it, in frame layout, in DEVICE memory of member
 * `root` (`dev_pixels` on that device, or that member's own framebuffer when NULL), complete on `hip_stream` (a stream of
 * the root's device; NULL = the root member's own stream).  On a multi-device context every other member renders its
 * stripes and pushes them to the root with peer copies over xGMI (one link per source GPU, all concurrent, each stripe
 * landing at its final place), the root renders its own stripes in place.  On a plain context (root 0) it is
 * rxr_render_rows_to over all rows.  Asynchronous; rxr_synchronize waits for it.
 * Replaces the tile loop + the final tile concatenation, src/rasterizer.rs:256-579. */
int rxr_render_gather(rxr_ctx *ctx, int root, void *dev_pixels, void *hip_stream);

/* Waits for everything the context has queued -- on its own streams AND on the caller's stream of the last
 * rxr_render_rows_to / rxr_render_stripes_to -- and reports what the launches since the previous call left behind:
 *   RXR_OK            every frame since the last call is complete (a bin-list overflow of the LAST launch is repaired here:
 *                     the lists are grown and that launch is rendered again);
 *   RXR_ERR_OVERFLOW  see above: an EARLIER launch overflowed; its frame was incomplete;
 *   RXR_ERR_INVALID   a fragment's Rusteria program did what makes the reference panic;
 *   RXR_ERR_UNSUPPORTED a pixel's opacity staircase overflowed (four nested GROUPS of opacity batches -- runs of opacity batches
 *                       without a profiled opaque batch between them --).
 * Stream contract: every render of a context uses the context's one set of scratch buffers.  A render on a different
 * stream than the previous one is ordered behind it by the library; rxr_upload_frame / rxr_set_* wait (on the host) for
 * all renders, including those on caller streams, before they overwrite anything.  A caller that queues frame after
 * frame without synchronizing must call rxr_synchronize before it declares those frames done. */
int rxr_synchronize(rxr_ctx *ctx);
int rxr_get_stats(rxr_ctx *ctx, rxr_stats *out);
/* device pointer of the context framebuffer (width*height*4 bytes of the last uploaded frame) */
void *rxr_device_framebuffer(rxr_ctx *ctx);

/* diagnostics: the raster kernel replaces hipcc's expansions of f32 division, sqrtf and exp2f(k*log2f(x))
 * by shorter instruction sequences that are bit-identical (rusterix_amd/csrc/rxr_exact_math.h).  This
 * runs both over `n_tuples` seeded operand tuples per operation kind on the device (rounded up to whole
 * workgroups) and returns the number of tuples whose results differ in mismatches[0..RXR_MATH_KINDS-1]:
 * 0 div2, 1 div3, 2 div3_self, 3 normalize3, 4 sqrt, 5 pow, 6 div1, 7 pixel-centre/size and byte/255,
 * 8 normalize3 with exactly-zero components (surface normals), 9 sqrt over a strided sweep of its whole
 * operand window (stride and phase from the seed; the sweep covers n_tuples operands), 10 the saturating float -> u32 conversion
 * (Rust's `as` casts, one v_cvt_u32_f32) against its compare-and-select form over a strided sweep of all bit patterns,
 * 11 the wave maximum of non-negative floats and 12 the wave's inclusive prefix sum through DPP operands against the shuffle forms
 * (at most 64 tuples per lane each).
 * Blocking.  Nothing in the reference corresponds to it. */
#define RXR_MATH_KINDS 13
int rxr_selftest_math(rxr_ctx *ctx, uint64_t n_tuples, uint64_t seed, uint64_t mismatches[RXR_MATH_KINDS]);

/* ---- ray picking over the meshes of the last rxr_set_meshes (rusterix_amd/csrc/rxr_intersect.hip) ---------------------------
 * Scene::intersect (src/scene.rs:216-276) with Batch3D::intersect per mesh (src/batch/batch3d.rs:844-948), exact to the bit:
 * Moeller-Trumbore on the OBJECT-SPACE vertices (transform_3d is ignored, as in the reference) against the normalised direction;
 * the closest hit per mesh (the earliest triangle on equal t); the meshes folded in array order -- RXR_LIST_CHUNK_OPACITY /
 * _CHUNK_TERRAIN / _STATIC / _DYNAMIC replace the best hit when closer, RXR_LIST_CHUNK the same unless the hit's profile id equals
 * the best's, RXR_LIST_OVERLAY replaces it whenever it hits.  Per ray: t (FLT_MAX on a miss), mesh (the index into the
 * rxr_set_meshes array -- which recovers profile_id and geometry_source -- or UINT32_MAX on a miss), triangle (mesh-local; 0 on a
 * miss), hitpoint = origin + dir * t with the caller's un-normalised dir ((0,0,0) on a miss).  RXR_INTERSECT_FULL adds what
 * Batch3D::intersect(ray, false) computes: the interpolated uv and the interpolated, normalised normal facing against dir (zeros
 * on a miss); the choice of hit is the same.  NULL required pointers: RXR_ERR_INVALID; n_rays == 0 does nothing; no meshes
 * registered: every ray misses.  An intersect changes no frame state: a frame uploaded before it renders as it would have.  Nothing
 * of this is part of Rasterizer::rasterize. */
#define RXR_INTERSECT_FULL (1u << 0)   /* Batch3D::intersect(ray, false): uv + normal as well */
/* host arrays, blocking: origins / dirs [n][3]; hitpoint [n][3], uv [n][2], normal [n][3] may be NULL.  Multi-device handles: member 0. */
int rxr_intersect(rxr_ctx *ctx, const float *origins, const float *dirs, uint32_t n_rays, uint32_t flags, float *t, uint32_t *mesh,
                  uint32_t *triangle, float *hitpoint, float *uv, float *normal);
/* the same on DEVICE arrays, queued on hip_stream (NULL = the context's stream; asynchronous).  Multi-device handles:
 * RXR_ERR_UNSUPPORTED (use rxr_member). */
int rxr_intersect_to(rxr_ctx *ctx, const float *dev_origins, const float *dev_dirs, uint32_t n_rays, uint32_t flags, float *dev_t,
                     uint32_t *dev_mesh, uint32_t *dev_triangle, float *dev_hitpoint, float *dev_uv, float *dev_normal, void *hip_stream);
/* Rasterizer::screen_ray (src/rasterizer.rs:1843-1870) for every pixel (x, y) of [x0, x0+w) x [y0, y0+h), row-major, into device
 * arrays [w*h][3]: inverse_view / inverse_projection are column-major 4x4 matrices, width / height the viewport.  Queued on
 * hip_stream (NULL = the context's stream).  Multi-device handles: RXR_ERR_UNSUPPORTED. */
int rxr_screen_rays_to(rxr_ctx *ctx, const float *inverse_view, const float *inverse_projection, float width, float height,
                       uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, float *dev_origins, float *dev_dirs, void *hip_stream);
/* Opt-in: cull the many-ray queries (rxr_intersect / _to with more than 64 rays, every round of rxr_trace / _to) with a tree of boxes
 * that the context builds on the device over the resident triangles (rusterix_amd/csrc/rxr_ray_accel.hip), lazily before the next such
 * query and again after every rxr_set_meshes / rxr_update_meshes (rxr_set_ray_refresh below: refitted instead).  Every output word stays what the brute-force kernels write: the
 * tree only skips triangles whose test would reject the ray, by a padded box test whose margin is measured, not proven (DESIGN.md
 * section 19).  RXR_RAY_ACCEL_OFF is the default; _COUNT is _ON plus a count of the ray-triangle tests a call runs (a second kernel
 * instantiation: _ON does not pay for it).  Any other mode: RXR_ERR_INVALID.  Multi-device handles: member 0. */
#define RXR_RAY_ACCEL_OFF 0u
#define RXR_RAY_ACCEL_ON 1u
#define RXR_RAY_ACCEL_COUNT 2u
int rxr_set_ray_accel(rxr_ctx *ctx, uint32_t mode);
/* blocking; out[..]: */
#define RXR_RAY_ACCEL_INFO_MODE 0u        /* RXR_RAY_ACCEL_*                                                              */
#define RXR_RAY_ACCEL_INFO_VALID 1u       /* 1: the tree describes the current meshes (the four words below: 0 otherwise) */
#define RXR_RAY_ACCEL_INFO_TRIANGLES 2u
#define RXR_RAY_ACCEL_INFO_NODES 3u
#define RXR_RAY_ACCEL_INFO_LEVELS 4u
#define RXR_RAY_ACCEL_INFO_WILD 5u        /* triangles that are always tested (not finite, or too thin for a box)         */
#define RXR_RAY_ACCEL_INFO_BUILDS 6u      /* builds since rxr_create                                                      */
#define RXR_RAY_ACCEL_INFO_BATCHES 7u     /* batches of rays that went through the tree since rxr_create                  */
#define RXR_RAY_ACCEL_INFO_TESTS 8u       /* ray-triangle tests of the last call under RXR_RAY_ACCEL_COUNT                */
#define RXR_RAY_ACCEL_INFO_WORDS 9u
int rxr_ray_accel_info(rxr_ctx *ctx, uint64_t out[RXR_RAY_ACCEL_INFO_WORDS]);
/* Opt-in, on top of rxr_set_ray_accel: batches of rays too small to fill the device with a thread per ray walk the same tree a WAVE
 * per ray, 64 boxes or 64 triangles at a step (k_accel_by_wave, rusterix_amd/csrc/rxr_ray_accel.hip).  It applies
 * only when the tree takes -- the accel mode is _ON or _COUNT and a tree stands; with the accel mode off the switch does nothing -- and
 * then ahead of both existing routes, in rxr_intersect / _to and every round of rxr_trace / _to.  Every output word stays what the
 * brute-force kernels write, under the margin of section 19 and no new one; _COUNT's tests cover this route too.  RXR_RAY_WAVE_OFF is
 * the default: batches route exactly as without the call (64 rays or fewer never open a tree batch).  Any other mode: RXR_ERR_INVALID,
 * nothing changed.  Multi-device handles: member 0. */
#define RXR_RAY_WAVE_OFF 0u    /* default: routes exactly as today                                                     */
#define RXR_RAY_WAVE_ON 1u     /* batches that rxr_ray_wave_takes() names go a wave per ray, when the tree takes       */
#define RXR_RAY_WAVE_FORCE 2u  /* every batch of >= 1 ray goes that way when the tree takes (tests, sweeps)            */
int rxr_set_ray_wave(rxr_ctx *ctx, uint32_t mode);
/* the rule of RXR_RAY_WAVE_ON for a batch of n_rays against a scene of n_triangles: 1 or 0.  No context, no device: a closed form over
 * the constants of rusterix_amd/csrc/rxr_isect.h, which profiles/ray_wave/README.md derives from its table. */
int rxr_ray_wave_takes(uint32_t n_rays, uint32_t n_triangles);
/* not blocking; out[..]: */
#define RXR_RAY_WAVE_INFO_MODE 0u     /* RXR_RAY_WAVE_*                                                                */
#define RXR_RAY_WAVE_INFO_BATCHES 1u  /* batches of rays that went a wave per ray since rxr_create                     */
#define RXR_RAY_WAVE_INFO_RAYS 2u     /* ... and their rays (RXR_RAY_ACCEL_INFO_BATCHES counts neither)                */
#define RXR_RAY_WAVE_INFO_WORDS 3u
int rxr_ray_wave_info(rxr_ctx *ctx, uint64_t out[RXR_RAY_WAVE_INFO_WORDS]);
/* Opt-in: what rxr_update_meshes / _to leaves for the next rxr_intersect / rxr_trace.  RXR_RAY_REFRESH_FULL, the
 * default: the pick records and the tree are invalid, the next query builds all of them again.  RXR_RAY_REFRESH_RANGED: a successful
 * update adds the meshes it named to a set on the context (a union; a refused update adds nothing, rxr_set_meshes empties it), and the
 * next query rewrites only those meshes' pick records and, when a tree stands and rxr_set_ray_accel's mode is on, their sorted records,
 * the leaves over them and the leaves' ancestors, each node by the build's own arithmetic -- the tree keeps the order of its last
 * build, RXR_RAY_ACCEL_INFO_BUILDS does not move and RXR_RAY_ACCEL_INFO_VALID is 1 only when nothing is pending.  With the accel mode
 * off a standing tree is dropped instead.  Every output word of a query is the same under both modes.  Switching to _FULL while meshes
 * are pending invalidates as _FULL would have.  Any other mode: RXR_ERR_INVALID.  Multi-device handles: member 0. */
#define RXR_RAY_REFRESH_FULL 0u
#define RXR_RAY_REFRESH_RANGED 1u
int rxr_set_ray_refresh(rxr_ctx *ctx, uint32_t mode);
/* a refit that rewrites up to this many leaves runs all levels in one launch of one workgroup, more take one launch per level
 * (profiles/ray_refresh/README.md has the sweep) */
#define RXR_RAY_REFIT_SMALL_MAX 256u
#define RXR_RAY_REFIT_NONE 0u
#define RXR_RAY_REFIT_SMALL 1u
#define RXR_RAY_REFIT_GENERAL 2u
/* not blocking; out[..]: */
#define RXR_RAY_REFRESH_INFO_MODE 0u       /* RXR_RAY_REFRESH_*                                                          */
#define RXR_RAY_REFRESH_INFO_PENDING 1u    /* meshes named by updates since the last query                               */
#define RXR_RAY_REFRESH_INFO_REFRESHES 2u  /* ranged refreshes of the pick records since rxr_create                      */
#define RXR_RAY_REFRESH_INFO_REFITS 3u     /* ... of which refitted a tree                                               */
#define RXR_RAY_REFRESH_INFO_TRIANGLES 4u  /* triangles whose records the last refresh rewrote                           */
#define RXR_RAY_REFRESH_INFO_LEAVES 5u     /* leaves its refit rewrote (0: no refit)                                     */
#define RXR_RAY_REFRESH_INFO_NODES 6u      /* nodes of all levels its refit rewrote, the leaves included                 */
#define RXR_RAY_REFRESH_INFO_ROUTE 7u      /* RXR_RAY_REFIT_* of the last refresh                                        */
#define RXR_RAY_REFRESH_INFO_WORDS 8u
int rxr_ray_refresh_info(rxr_ctx *ctx, uint64_t out[RXR_RAY_REFRESH_INFO_WORDS]);
/* For tests and tools, blocking: recomputes into scratch every pick record from the pools (the kernel of the full pass) and, where a
 * tree stands, every sorted record, leaf and level from the resident order (the build's kernels), and counts what differs from the
 * resident arrays bit for bit.  Pending meshes are not refreshed first: the call reports the arrays as they stand.  out[..]: */
#define RXR_RAY_REFRESH_VERIFY_PICK_WORDS 0u    /* words of the pick records that differ                                 */
#define RXR_RAY_REFRESH_VERIFY_SORTED_WORDS 1u  /* words of the tree's sorted records that differ                        */
#define RXR_RAY_REFRESH_VERIFY_NODES 2u         /* nodes that differ in any bit                                          */
#define RXR_RAY_REFRESH_VERIFY_WILD 3u          /* the recomputed count of RXR_RAY_ACCEL_INFO_WILD                       */
#define RXR_RAY_REFRESH_VERIFY_CHECKED 4u       /* bit 0: pick records stood and were compared, bit 1: a tree did        */
#define RXR_RAY_REFRESH_VERIFY_WORDS 5u
int rxr_ray_refresh_verify(rxr_ctx *ctx, uint64_t out[RXR_RAY_REFRESH_VERIFY_WORDS]);
/* drops the tree: the next many-ray query with the accel mode on builds it from scratch (a refit keeps the order of the last build;
 * after many updates a fresh order may cull better).  Pick records and pending meshes are left alone.  Multi-device handles: member 0. */
int rxr_ray_accel_invalidate(rxr_ctx *ctx);

/* ---- running a program over an image: the shader-texture bake (rusterix_amd/csrc/rxr_bake.hip) -------------------------------
 * Rusteria::shade (rusteria/src/lib.rs:161-210) over a width x height RenderBuffer, as Chunk::add_shader runs it at 64 x 64 for
 * chunk.shader_textures[i] (src/chunk.rs:104-122) and the rsia tool at any size.  Texel (x, y), row-major, top row first:
 * uv = (x / width, 1 - y / height, 0), color = 0, every other Execution field at its Execution::new value (roughness 0.5, the
 * rest 0: the bake sets neither time nor hitpoint), Execution::shade, pixel = (color.x, color.y, color.z, 1) with -0.0 stored as
 * +0.0 (RenderBuffer::accum_from at accum == 1, rusteria/src/renderbuffer.rs:64-85).  The bytes are RenderBuffer::as_rgba_bytes
 * (:88-107, :152-155): (c.powf(0.4545) * 255.0) as u8 per colour channel -- the cast saturates, truncates and maps NaN to 0 --
 * and 255 for alpha; powf comes from the device math library, so a channel whose exact value lies within a few ulp of an integer
 * may differ from a host's libm by one step.  Texture::generate_normals (chunk.rs:119) only fills Texture.data_ext, which the
 * rasterizer never reads: not computed.
 * Which programs: those rxr_set_shaders accepts that, in addition, never read roughness, metallic, opacity, normal or bump
 * before the same invocation has written it when the program writes that field anywhere (the reference keeps one Execution per
 * 80 x 80 tile and resets only uv and color between texels, so such a read would see the previous texel's value; a field that is
 * only read holds its constant).  Anything else: RXR_ERR_UNSUPPORTED.  A program without `shade` (shade_index -1; add_shader
 * pushes None and bakes nothing, chunk.rs:107-109) or an index outside the set: RXR_ERR_INVALID.
 * A bake always runs the interpreter and changes no frame, scratch or compiled-program state: a frame uploaded before it renders
 * as it would have. */
/* validation only, no context: the status and, in `message`, the reason for program `program` of `set` (everything
 * rxr_check_shaders refuses for the set, plus the rule above for that program) */
int rxr_check_bake(const rxr_shader_set *set, uint32_t program, char *message, uint32_t message_capacity);
/* n bakes of width x height each, bake i over programs[i] of the resident set (rxr_set_shaders; a program may repeat), in ONE
 * launch.  pixels: n * width * height * 4 floats (RenderBuffer.pixels), rgba: n * width * height * 4 bytes (as_rgba_bytes); either
 * may be NULL.  width, height in [1, RXR_BAKE_MAX_DIM] and n * width * height <= RXR_BAKE_MAX_TEXELS, else RXR_ERR_INVALID; n == 0
 * does nothing.  Host memory, blocking; a program that does what makes the reference panic (or exceeds the interpreter's
 * instruction bound): RXR_ERR_INVALID, the message names the program and the texel.  Multi-device handles: member 0.
 * Replaces: rs.shade + as_rgba_bytes in Chunk::add_shader, src/chunk.rs:110-116. */
#define RXR_BAKE_MAX_DIM 16384u
#define RXR_BAKE_MAX_TEXELS (1u << 28)
int rxr_bake_shaders(rxr_ctx *ctx, const uint32_t *programs, uint32_t n, uint32_t width, uint32_t height, float *pixels, uint8_t *rgba);
/* the same into DEVICE memory (its first and last byte are checked to be device memory of the context's device), queued on hip_stream (NULL = the context's stream);
 * `programs` is host memory and is read before the call returns.  Asynchronous: a program fault is reported by the next
 * rxr_synchronize (RXR_ERR_INVALID).  Multi-device handles: RXR_ERR_UNSUPPORTED (use rxr_member).
 * Replaces: Rusteria::shade, rusteria/src/lib.rs:161-210. */
int rxr_bake_shaders_to(rxr_ctx *ctx, const uint32_t *programs, uint32_t n, uint32_t width, uint32_t height, float *dev_pixels,
                        uint8_t *dev_rgba, void *hip_stream);

/* ---- terrain chunk textures: Terrain::bake_chunk (rusterix_amd/csrc/rxr_terrain.hip) --------------------------------------------
 * chunk.terrain_texture, the texture every RXR_SOURCE_TERRAIN batch samples (src/chunk.rs:135-151), as Terrain::bake_chunk
 * (src/terrain/mod.rs:318-369) makes it for build_chunk_at (:372-399, modifiers == false): side x side RGBA8 with
 * side = chunk_size * pixels_per_tile, row-major, top row first.  Texel (x, y) of chunk (cx, cy):
 *   tile = (cx * chunk_size) as f32 + (x as f32 / pixels_per_tile as f32), world = tile * scale, the blend mode that of the cell
 *   at floor(tile) (:336-344); None: sample_source(world) (:197-245), its alpha included; Blend(r): sample_source_blended_radius
 *   (world, r) (:247-298); BlendOffset(r, off) and Custom(r, _, off): the same at world + off.  Integer texels in, integer bytes
 *   out, every f32 operation once and in the reference's order (no libm): the bytes are the reference's bytes.
 * The quirks are kept: sample_source's cell is floor(world / scale), not floor(tile); its uv is x - trunc(x), plus 1.0 when
 * negative, which can be exactly 1.0; no source is the 135 / 120 checker by cell parity; a blended texel without a valid tap --
 * radius 0 included, whose only weight is 0 / 0 -- is the checker with the colours swapped (120 / 135), taken at the position the
 * function was given; a tap exactly on the rim counts with weight 0; a blended texel has alpha 255.
 * process_batch_modifiers (modifiers == true) needs the map and the ShapeFX graph: host only, not part of this. */
#define RXR_TERRAIN_BLEND_NONE 0u     /* TerrainBlendMode::None                         (src/terrain/chunk.rs:13-18) */
#define RXR_TERRAIN_BLEND_RADIUS 1u   /* Blend(r): sample_source_blended_radius(world_pos, r)                        */
#define RXR_TERRAIN_BLEND_OFFSET 2u   /* BlendOffset(r, off) and Custom(r, _, off): ...(world_pos + off, r)          */
/* cell_blend[i] = kind | radius << 8, radius 0..255 (the reference's u8) */
#define RXR_TERRAIN_MAX_CELLS (1u << 22)  /* cells of the bounding rectangle of one terrain                          */
#define RXR_TERRAIN_MAX_STEPS 64u         /* ceil(radius / (min(scale) * 0.5)): (2 * 64 + 1)^2 = 16 641 taps a texel */
/* validation only, no context: the status rxr_set_terrain would return and, in `message`, the reason.  RXR_ERR_INVALID: a scale
 * that is not finite and > 0 (the reference never leaves its tap loop at scale 0), chunk_size < 1, a non-finite offset, a texture
 * index outside [-1, n_textures), a zero-sized or NULL texture, an unknown blend kind (or bits above the radius), a bounding
 * rectangle of more than RXR_TERRAIN_MAX_CELLS cells, a NULL array.  RXR_ERR_UNSUPPORTED: a cell whose steps exceed
 * RXR_TERRAIN_MAX_STEPS (the host bakes such a terrain itself). */
int rxr_check_terrain(const float scale[2], int32_t chunk_size, const int32_t *cell_xy, const int32_t *cell_texture,
                      const uint32_t *cell_blend, const float *cell_offset, uint32_t n_cells, const rxr_texture *textures,
                      uint32_t n_textures, char *message, uint32_t message_capacity);
/* makes a terrain resident (it stays until the next call; n_cells == 0 removes it: every texel is then a checker texel).  The
 * caller flattens Terrain.chunks' `sources` and `blend_modes` maps (src/terrain/chunk.rs:29-31) into one cell list.
 * cell_texture: -1 wherever sample_source falls through to the checker (get_source is None, the variant is neither TileId nor
 * MaterialId, the lookup or textures.first() failed), else the index of that first texture in `textures`.  A coordinate given
 * twice: the later entry wins.  The library keeps a dense grid over the cells' bounding rectangle; cells outside it have no
 * source and blend None.  Arrays are read before the call returns.  A refused call leaves the resident terrain as it was.
 * Replaces: Terrain::get_source / get_blend_mode, src/terrain/mod.rs:115-145. */
int rxr_set_terrain(rxr_ctx *ctx, const float scale[2], int32_t chunk_size,
                    const int32_t *cell_xy,       /* [n_cells][2] world tile coordinates                                  */
                    const int32_t *cell_texture,  /* [n_cells] index into `textures`, or -1                               */
                    const uint32_t *cell_blend,   /* [n_cells]                                                            */
                    const float *cell_offset,     /* [n_cells][2], read for RXR_TERRAIN_BLEND_OFFSET cells; NULL = zeros  */
                    uint32_t n_cells, const rxr_texture *textures, uint32_t n_textures);
/* n chunks in one call: bake i is side * side * 4 bytes at rgba + i * side * side * 4 -- the bytes of the Texture bake_chunk
 * returns for chunk_coords[i].  RXR_ERR_INVALID: no rxr_set_terrain yet, pixels_per_tile < 1, side > RXR_BAKE_MAX_DIM,
 * n * side * side > RXR_BAKE_MAX_TEXELS, or chunk_coords[i] * chunk_size outside i32 (the reference overflows).  n == 0 does
 * nothing.  Host memory, blocking.  The call is split into launches of bounded work (texels x taps; RXR_TERRAIN_LAUNCH_TAPS in
 * the environment, read at each call, overrides the bound).  Leaves frame state, scratch and the textures of rxr_set_textures
 * alone.  Multi-device handles: member 0, for rxr_set_terrain as well.
 * Replaces: Terrain::bake_chunk, src/terrain/mod.rs:318-369. */
int rxr_bake_terrain(rxr_ctx *ctx, const int32_t *chunk_coords, uint32_t n, int32_t pixels_per_tile, uint8_t *rgba);
/* the same into DEVICE memory (its first and last byte are checked to be memory of the context's device; 4-byte aligned), queued
 * on hip_stream (NULL = the context's stream); chunk_coords is host memory and is read before the call returns.  Asynchronous.
 * Multi-device handles: RXR_ERR_UNSUPPORTED (use rxr_member).
 * Replaces: the rayon rows of Terrain::bake_chunk, src/terrain/mod.rs:331-366. */
int rxr_bake_terrain_to(rxr_ctx *ctx, const int32_t *chunk_coords, uint32_t n, int32_t pixels_per_tile, uint8_t *dev_rgba,
                        void *hip_stream);

/* ---- resident chunk textures (rusterix_amd/csrc/rxr_chunk_tex.hip) ---------------------------------------------------------------
 * chunk.terrain_texture and chunk.shader_textures (src/chunk.rs:36, :53) registered ONCE and rewritten in place, instead of crossing
 * the ABI in every rxr_upload_frame (which scans every texel for its alpha and copies it into the frame blob): what rxr_set_meshes and
 * rxr_update_meshes_to are for chunk geometry.  Both bakes write device memory (rxr_bake_terrain_to, rxr_bake_shaders_to); with a
 * registration their bytes reach the renderer without visiting the host.
 *
 * Registration.  textures[i] is SLOT i; its size is fixed until the next registration.  rgba == NULL reserves a slot of that size filled
 * with zero bytes (not opaque), to be written by an update.  chunk_terrain[c] is the slot of chunk c's terrain_texture or -1 for None;
 * chunk_shader_slots[chunk_shader_first[c] .. chunk_shader_first[c + 1]) are the slots of its shader_textures, -1 for None (a program
 * without `shade`).  A slot may be named by several chunks, or by none.  RXR_ERR_INVALID, with the previous registration left as it
 * was: a side of 0 or above 32768, 2^31 texels or more in all (the limits of a frame's own chunk textures), a slot index that is
 * neither -1 nor below n_textures, chunk_shader_first that does not start at 0 or decreases, a NULL array with a non-zero count.
 * n_chunks == 0 removes the registration.  Blocking; all arrays are read before it returns.  Multi-device handles: every member.
 *
 * Frames.  While a registration is held, rxr_upload_frame wants frame.n_chunks == the registered n_chunks and, in every rxr_chunk,
 * terrain_texture == NULL and n_shader_textures == 0; anything else is RXR_ERR_INVALID and the message says so.  origin, size, the
 * occluders and the program range still come from the frame's rxr_chunk (size == 0 with a terrain slot is refused as before);
 * pixels_per_tile is the slot's width / size.  Such a frame is drawn by the same kernels with the same bytes as the frame that carries
 * the textures: only where the texels live differs.  Registering, removing and updating DROP THE RESIDENT FRAME: upload it again (it
 * then costs no texels).
 *
 * Updates.  slots[i] names the slot source i goes to; source i is its w * h * 4 bytes, the sources lie back to back in the order of
 * `slots` -- the layout rxr_bake_terrain_to writes for n chunks, and rxr_bake_shaders_to's dev_rgba -- so they are 4-byte aligned and
 * no more.  Refused on the host before anything is queued, changing nothing: no registration, a slot out of range, a slot named twice,
 * and for _to a dev_rgba that is not memory of the context's device (first and last byte are checked) or not 4-byte aligned.  n == 0
 * does nothing.  BLOCKING, both forms: they wait for everything the context has queued (renders read the pool), queue
 * k_chunk_tex_commit on hip_stream (NULL = the context's stream) behind the bake that produced dev_rgba, copy n flag words back and
 * synchronise that stream.  The kernel copies and computes each slot's flag "every texel has alpha 255", which decides what
 * add_local's scan decided for a frame's own textures.  Multi-device handles: the host form runs on every member, the _to form is
 * RXR_ERR_UNSUPPORTED (use rxr_member). */
/* validation only, no context: the status rxr_set_chunk_textures would return and, in `message`, the reason */
int rxr_check_chunk_textures(const rxr_texture *textures, uint32_t n_textures, const int32_t *chunk_terrain,
                             const uint32_t *chunk_shader_first, const int32_t *chunk_shader_slots, uint32_t n_chunks, char *message,
                             uint32_t message_capacity);
int rxr_set_chunk_textures(rxr_ctx *ctx, const rxr_texture *textures, uint32_t n_textures, const int32_t *chunk_terrain,
                           const uint32_t *chunk_shader_first, const int32_t *chunk_shader_slots, uint32_t n_chunks);
int rxr_update_chunk_textures(rxr_ctx *ctx, const uint32_t *slots, uint32_t n, const uint8_t *rgba);
int rxr_update_chunk_textures_to(rxr_ctx *ctx, const uint32_t *slots, uint32_t n, const uint8_t *dev_rgba, void *hip_stream);
/* debugging / tests, and a host mirror whose copy went stale: slot's size, its flag and (rgba != NULL) its w * h * 4 bytes.  Any
 * output may be NULL.  Multi-device handles: member 0. */
int rxr_read_chunk_texture(rxr_ctx *ctx, uint32_t slot, uint32_t size[2], uint32_t *all_opaque, uint8_t *rgba);

/* ---- terrain picks: Terrain::ray_terrain_hit (rusterix_amd/csrc/rxr_terrain_hit.hip) ---------------------------------------------
 * "Ray / terrain hit used for editing" (src/terrain/mod.rs:427-479), exact to the bit.  The reference does not intersect the terrain
 * mesh: it marches the height field in up to RXR_TERRAIN_MARCH_STEPS steps of 0.1 along the caller's UN-NORMALISED dir with nearest
 * sampling (sample_height, :148-152: round half away from zero, in WORLD coordinates -- the scale is not applied) and refines the
 * first step with point.y - height < 0.01 by four bisections over bilinear samples (sample_height_bilinear, :155-173).  Kept as it
 * is: t advances by repeated f32 addition (t_10 = 1.0000001, not 1.0); step 0 is always tested, step k >= 1 iff t_k <= max_distance,
 * a NaN max_distance never leaves; `low` of the bisection starts at max(t_k - 0.1, 0); grid_pos divides by the scale although the
 * heights were looked up without it. */
#define RXR_TERRAIN_MARCH_STEPS 1500u
/* validation only, no context: the status rxr_set_terrain_heights would return and, in `message`, the reason.  RXR_ERR_INVALID: a
 * scale that is not finite and > 0, a bounding rectangle of more than RXR_TERRAIN_MAX_CELLS cells, a coordinate outside +-2^30, a
 * NULL array with n_cells > 0. */
int rxr_check_terrain_heights(const float scale[2], const int32_t *cell_xy, const float *cell_height, uint32_t n_cells,
                              char *message, uint32_t message_capacity);
/* makes a terrain's heights resident (they stay until the next call; n_cells == 0 registers the empty terrain, a plane at 0).
 * cell_height[i] is what Terrain::get_height returns for cell_xy[i] (the caller flattens chunk.processed_heights where a chunk has
 * them, else chunk.heights, src/terrain/chunk.rs:81-95); any f32 bit pattern is legal.  A coordinate given twice: the later entry wins.  The library keeps a dense f32 grid over the cells' bounding
 * rectangle; cells outside it and cells not listed are 0.0, the reference's answer -- and, over the same rectangle, which cells
 * were listed (rxr_terrain_meshes: they are the cells of the chunk meshes).  Re-registration waits for queued picks and mesh
 * builds.  Independent of rxr_set_terrain: buffers and
 * scale of its own; either may be registered without the other.  Arrays are read before the call returns.  A refused call leaves
 * the resident heights as they were.  Multi-device handles: member 0.
 * Replaces: Terrain::get_height, src/terrain/mod.rs:82-89. */
int rxr_set_terrain_heights(rxr_ctx *ctx, const float scale[2], const int32_t *cell_xy /* [n_cells][2] world cell coordinates */,
                            const float *cell_height /* [n_cells] */, uint32_t n_cells);
/* n rays against the resident heights, one max_distance for all.  origins / dirs [n][3], dirs un-normalised, as rxr_intersect takes
 * them.  Per ray: hit (1 or 0; required); t = t_hit IN UNITS OF THE CALLER'S dir (FLT_MAX on a miss) -- rxr_intersect's t is along
 * the NORMALISED direction: multiply this one by |dir| before taking the nearer of a mesh hit and a terrain hit; world_pos [n][3] =
 * TerrainHit.world_pos, whose [1] is TerrainHit.height; grid_pos [n][2] = TerrainHit.grid_pos (zeros on a miss).  t, world_pos and
 * grid_pos may be NULL.  Where the reference's world_pos is a NaN (NaN or infinite ray components, NaN heights) this one is a NaN;
 * its sign and payload are the device's.  RXR_ERR_INVALID: no rxr_set_terrain_heights yet, or a NULL required pointer; n_rays == 0 does nothing.
 * Host memory, blocking.  A few rays (a click) run one ray per wave, more run one ray per lane (RXR_TERRAIN_HIT_ROUTE=lane|wave in
 * the environment, read at each call, forces one; the bytes are the same); the call is split into launches of a
 * bounded number of rays (RXR_TERRAIN_HIT_LAUNCH_RAYS overrides the bound).  Changes no frame, scratch, bake or picking state.
 * Multi-device handles: member 0.
 * Replaces: Terrain::ray_terrain_hit, src/terrain/mod.rs:427-479. */
int rxr_terrain_hits(rxr_ctx *ctx, const float *origins, const float *dirs, uint32_t n_rays, float max_distance, uint32_t *hit,
                     float *t, float *world_pos, int32_t *grid_pos);
/* the same on DEVICE arrays (each given array's first and last byte are checked to be memory of the context's device; 4-byte
 * aligned), queued on hip_stream (NULL = the context's stream): the rays of rxr_screen_rays_to go straight in.  Asynchronous.
 * Multi-device handles: RXR_ERR_UNSUPPORTED (use rxr_member). */
int rxr_terrain_hits_to(rxr_ctx *ctx, const float *dev_origins, const float *dev_dirs, uint32_t n_rays, float max_distance,
                        uint32_t *dev_hit, float *dev_t, float *dev_world_pos, int32_t *dev_grid_pos, void *hip_stream);

/* ---- terrain chunk meshes: TerrainChunk::build_mesh (rusterix_amd/csrc/rxr_terrain_mesh.hip) --------------------------------------
 * The Batch3D a chunk's terrain texture is drawn on (src/terrain/chunk.rs:253-297) with its vertex normals
 * (Batch3D::compute_vertex_normals, src/batch/batch3d.rs:771-809), from the resident heights, exact to the bit.  A cell of chunk
 * (cx, cy) -- world cells cx * chunk_size .. + chunk_size - 1, likewise in y -- is PRESENT iff rxr_set_terrain_heights listed it
 * (twice is present; a listed 0.0 is present, an unlisted cell is not): the caller lists the keys of processed_heights.  The
 * reference walks a hash map, so its numbering is whatever the hash gives; this is THE MESH IT BUILDS WHEN THE CELLS ARE VISITED IN
 * ASCENDING (ly, lx), row by row:
 *   per present cell, its corners (0,0), (1,0), (0,1), (1,1) that no earlier cell made get the next vertex indices; a vertex is
 *   [X as f32 * scale.x, get_height(X, Y), Y as f32 * scale.y, 1.0], (X, Y) the corner in world cells; the cell's triangles are
 *   (i0, i2, i1) and (i1, i2, i3).  Normals start at +0.0; per triangle in index order normalized(cross(p1 - p0, p2 - p0)) is added
 *   to its three vertices; each sum is divided by its count and normalised again.
 * Kept as it is: the last row and column of corners read the neighbouring chunks' heights, or 0.0 where no cell is listed; uvs are
 * all [0, 0] and do not cross this boundary; a NaN height gives NaN normals (a NaN is a NaN: sign and payload are the device's); a
 * sum of length zero divides by zero.  build_mesh_d2 and process_batch_modifiers' Colorize pass are host work and not part of
 * this (its Height pass: rxr_flatten_terrain below). */
#define RXR_TERRAIN_MESH_MAX_CHUNK_SIZE 64
/* n chunks in one call, with the fixed strides VS = (chunk_size + 1)^2 vertices and TS = 2 * chunk_size^2 triangles a chunk:
 * counts [n][2] = vertices, triangles of chunk i; vertices [n][VS][4]; indices [n][TS][3], chunk-local (they index chunk i's own
 * vertices); normals [n][VS][3].  Slots past a chunk's counts are NOT written; a chunk without a present cell has counts 0, 0 (the
 * reference returns an empty batch for a chunk without processed_heights: do not ask for such a chunk, or ignore its answer).  The
 * scale is rxr_set_terrain_heights'.  RXR_ERR_INVALID: no rxr_set_terrain_heights yet, chunk_size < 1, a chunk whose cells leave
 * +-2^30, a NULL pointer (all four outputs are required), output sizes that overflow; RXR_ERR_UNSUPPORTED: chunk_size above
 * RXR_TERRAIN_MESH_MAX_CHUNK_SIZE.  n == 0 does nothing.  Host memory, blocking.  The call is split into launches of 256 chunks.
 * Changes no frame, scratch, bake or picking state.  Multi-device handles: member 0.
 * Replaces: TerrainChunk::build_mesh, src/terrain/chunk.rs:253-297, and Batch3D::compute_vertex_normals, src/batch/batch3d.rs:771-809. */
int rxr_terrain_meshes(rxr_ctx *ctx, const int32_t *chunk_coords /* [n][2] */, uint32_t n, int32_t chunk_size,
                       uint32_t *counts, float *vertices, uint32_t *indices, float *normals);
/* the same into DEVICE arrays (each one's first and last byte are checked to be memory of the context's device; 4-byte aligned),
 * queued on hip_stream (NULL = the context's stream); chunk_coords is host memory and is read before the call returns.
 * Asynchronous.  Multi-device handles: RXR_ERR_UNSUPPORTED (use rxr_member). */
int rxr_terrain_meshes_to(rxr_ctx *ctx, const int32_t *chunk_coords, uint32_t n, int32_t chunk_size, uint32_t *dev_counts,
                          float *dev_vertices, uint32_t *dev_indices, float *dev_normals, void *hip_stream);

/* ---- flattened terrain heights: the Height pass of TerrainChunk::process_batch_modifiers (rusterix_amd/csrc/rxr_terrain_flatten.hip) --
 * processed_heights, the map get_height reads and build_mesh walks (src/terrain/chunk.rs:144-208), from the resident heights and a
 * resident list of FLATTEN OPS, exact to the bit.  An op is one Flatten node applied to one sector (ShapeFX::sector_modify_heightmap,
 * src/shapestack/shapefx.rs:414-478) or to one group of linedefs (linedef_modify_heightmap, :682-820).  THE ORDER IS THE CALLER'S: for
 * the reference, the sectors in sorted_sectors_by_area() order, each with the Flatten nodes its graph chain reaches in chain order,
 * then the linedef groups (the reference walks a hash map of groups: the list's order is this library's definition), each with its
 * chain's Flatten nodes.  A sector whose signed_distance is None (a linedef with a missing vertex) makes no op, a linedef with a
 * missing vertex no segment.  INTEGRATION.md says how the shim builds the list.
 * Per chunk: processed = heights.clone(), then every op in order inserts into it.  Every op reads the UNPROCESSED height, never an
 * earlier op's result: per cell the last op that writes wins; a cell no op writes keeps its height and its presence; a cell an op
 * writes becomes PRESENT even where the terrain had no height.  All f32, one operation per reference operation, nothing fused; the
 * casts are Rust's saturating `as i32` (NaN gives 0).  With the chunk's bounds B = origin as f32 .. origin as f32 + (size as f32 -
 * 1.0), BBox::intersects / contains / expand as src/map/bbox.rs writes them (expand(a) moves each side by a * 0.5):
 *   sector op    applies to the chunk iff B intersects box.expanded(2.0), the sector's bounding_box moved by 1 -- NOT by the bevel.  Cell
 *                (x, y) is written iff x lies in floor(R.min.x) as i32 ..= ceil(R.max.x) as i32, R = box after expand(bevel), likewise
 *                y; B after expand(bevel) contains p = (x as f32, y as f32); sd < bevel * 4.0; and B contains p.  sd is
 *                Sector::signed_distance (src/map/sector.rs:308-333): min_dist from f32::MAX over the edges, t = dot(p - v0, edge) /
 *                dot(edge, edge) clamped as f32::clamp (a NaN stays), dist = |p - (v0 + edge * t)|, f32::min (which drops a NaN), negated
 *                when is_inside (:272-305, over the edges' START points; fewer than three: outside).  Value: original * (1 - s) +
 *                floor_height * s, s = smoothstep(0, bevel, bevel - sd) (:2258-2261), original = the unprocessed height, or floor_height
 *                where the cell is absent.
 *   linedef op   its segments for the chunk are those whose box.expanded(2.0) intersects B, in list order -- a filter PER CHUNK, so two
 *                neighbouring chunks may see different closest segments.  Cell (tx, ty) is written iff it lies in tile_min .. tile_max,
 *                EXCLUSIVE at the top, tile_min = floor((B.min - bevel * scale) / scale) as i32, tile_max = ceil((B.max + bevel * scale)
 *                / scale) as i32 (with bevel == 0 the chunk's last row and column are never written); the chunk has a segment; NOT
 *                dist > bevel for the closest segment to ((tx as f32 + 0.5) * scale.x, (ty as f32 + 0.5) * scale.y) (a NaN distance
 *                writes); and B contains (tx as f32, ty as f32).  closest_segment takes the first segment unconditionally and a later one
 *                only under dist < best: a degenerate FIRST segment (NaN) is never displaced.  Value: original * (1 - blend) + height *
 *                blend, height = height_start * (1 - t) + height_end * t, blend = smoothstep(0, bevel, bevel - dist), original = the
 *                unprocessed height, or `height` where the cell is absent.
 * Any f32 bit pattern is legal in heights, parameters and geometry; a NaN result is a NaN, its sign and payload are the device's.
 * Not kept: beyond +-2^24, where `x as f32` rounds, B can contain cells of a NEIGHBOURING chunk, which the reference inserts under keys
 * outside 0 .. size - 1 that nothing reads back through get_height; only the chunk's own size x size cells are computed here.
 * The Colorize pass (ShapeFX node graphs per texel of the baked texture) stays on the host. */
#define RXR_TERRAIN_FLATTEN_SECTOR 0u
#define RXR_TERRAIN_FLATTEN_LINEDEFS 1u
#define RXR_TERRAIN_FLATTEN_OP_FLOATS 6u       /* bevel, floor_height, then the sector's bounding_box: min x, min y, max x, max y
                                                  (a linedef op reads the bevel alone)                                              */
#define RXR_TERRAIN_FLATTEN_RECORD_FLOATS 10u  /* x0, y0, x1, y1 -- a sector's edge in linedef order, or a segment --, then for a
                                                  segment height_start, height_end and its linedef's bounding_box: min x, min y,
                                                  max x, max y (a sector op reads the first four alone)                            */
#define RXR_TERRAIN_FLATTEN_MAX_OPS 1024u
#define RXR_TERRAIN_FLATTEN_MAX_RECORDS (1u << 16)   /* records of the pool, and the sum of the ops' range lengths (ranges may overlap) */
#define RXR_TERRAIN_FLATTEN_MAX_SEGMENTS (1u << 14)  /* the sum of the LINEDEF ops' range lengths: a chunk's segment list lies in LDS  */
#define RXR_TERRAIN_HEIGHTS_REGISTERED 0u
#define RXR_TERRAIN_HEIGHTS_PROCESSED 1u
/* validation only, no context: the status rxr_set_terrain_flatten would return and, in `message`, the reason.  RXR_ERR_UNSUPPORTED:
 * n_ops above RXR_TERRAIN_FLATTEN_MAX_OPS, n_records or the sum of the range lengths above RXR_TERRAIN_FLATTEN_MAX_RECORDS, the sum of
 * the linedef ops' range lengths above RXR_TERRAIN_FLATTEN_MAX_SEGMENTS.
 * RXR_ERR_INVALID: a NULL array with a non-zero count, a kind that is neither RXR_TERRAIN_FLATTEN_SECTOR nor _LINEDEFS, a range
 * (first, count) that does not lie inside the pool.  An empty range is legal (a sector without edges has distance f32::MAX). */
int rxr_check_terrain_flatten(const uint32_t *op_kinds, const float *op_params, const uint32_t *op_ranges, uint32_t n_ops,
                              const float *records, uint32_t n_records, char *message, uint32_t message_capacity);
/* makes the op list resident (it stays until the next call; n_ops == 0 clears it: a flatten then copies the registered cells).
 * What does not depend on the cell is computed here, once, in the reference's f32 operations: an edge's v1 - v0 and dot(edge, edge),
 * the differences of is_inside, bevel * 4.0, the boxes moved by 1 and the sector's integer ranges.  Re-registration waits for queued
 * flattens.  Independent of rxr_set_terrain_heights.  Arrays are read before the call returns.  A refused call leaves the resident
 * list as it was.  Multi-device handles: member 0.
 * Replaces: the map walk of process_batch_modifiers per chunk, src/terrain/chunk.rs:153-208. */
int rxr_set_terrain_flatten(rxr_ctx *ctx, const uint32_t *op_kinds /* [n_ops] */,
                            const float *op_params /* [n_ops][RXR_TERRAIN_FLATTEN_OP_FLOATS] */,
                            const uint32_t *op_ranges /* [n_ops][2] first record, records */, uint32_t n_ops,
                            const float *records /* [n_records][RXR_TERRAIN_FLATTEN_RECORD_FLOATS] */, uint32_t n_records);
/* The library keeps a second grid and mask next to the registered ones, over the same bounding rectangle: the PROCESSED heights, a copy
 * of the registered grid after every rxr_set_terrain_heights (where the caller now registers chunk.heights, the unprocessed map).  For
 * the n named chunks this computes every cell's processed height and presence from the registered grid and the resident ops, writes
 * them into the processed grid (cells outside the rectangle are returned but not kept) and into heights [n][chunk_size * chunk_size]
 * and present (the same shape, 1 / 0), row by row; an absent cell's height is 0.0, get_height's answer.  Either array may be NULL.
 * No rxr_set_terrain_flatten yet is zero ops.  RXR_ERR_INVALID: no rxr_set_terrain_heights yet, chunk_size < 1, a chunk whose cells
 * leave +-2^30, a chunk named twice, NULL chunk_coords; RXR_ERR_UNSUPPORTED: chunk_size above RXR_TERRAIN_MESH_MAX_CHUNK_SIZE.  A
 * refused call queues nothing; n == 0 does nothing.  Host memory, blocking.  The call is split into launches of at most 256 chunks
 * (RXR_TERRAIN_FLATTEN_LAUNCH_CHUNKS in the environment, read at each call, lowers the bound).  Changes no frame, scratch, bake or mesh
 * state.  Multi-device handles: member 0.
 * Replaces: the Height pass of TerrainChunk::process_batch_modifiers, src/terrain/chunk.rs:144-208. */
int rxr_flatten_terrain(rxr_ctx *ctx, const int32_t *chunk_coords /* [n][2] */, uint32_t n, int32_t chunk_size, float *heights,
                        uint8_t *present);
/* the same into DEVICE arrays (each one's first and last byte are checked to be memory of the context's device; dev_heights 4-byte
 * aligned; NULL = not wanted), queued on hip_stream (NULL = the context's stream); chunk_coords is host memory and is read before the
 * call returns.  Asynchronous.  The processed grid is written in stream order: picks and mesh builds queued before it have read the
 * grid when it is written, those queued after it under RXR_TERRAIN_HEIGHTS_PROCESSED read what it wrote, on whichever streams they
 * run.  Multi-device handles: RXR_ERR_UNSUPPORTED (use rxr_member). */
int rxr_flatten_terrain_to(rxr_ctx *ctx, const int32_t *chunk_coords, uint32_t n, int32_t chunk_size, float *dev_heights,
                           uint8_t *dev_present, void *hip_stream);
/* which grid and mask rxr_terrain_hits[_to] and rxr_terrain_meshes[_to] read from now on: RXR_TERRAIN_HEIGHTS_REGISTERED (the default:
 * what rxr_set_terrain_heights listed) or RXR_TERRAIN_HEIGHTS_PROCESSED.  A choice of pointer on the host; calls already queued are
 * not affected.  It stays across rxr_set_terrain_heights.  Anything else is RXR_ERR_INVALID.  Multi-device handles: member 0. */
int rxr_set_terrain_height_source(rxr_ctx *ctx, uint32_t source);

/* ---- vertex normals: Batch3D::compute_vertex_normals (rusterix_amd/csrc/rxr_normals.hip) ------------------------------------------
 * The smooth normals of n meshes of ANY topology (src/batch/batch3d.rs:771-809), exact to the bit, in the strided layout
 * rxr_terrain_meshes[_to] writes and rxr_update_meshes[_to] reads, so the three chain with no repacking: counts [n][2] = vertices,
 * triangles of mesh i; vertices [n][vertex_stride][4] (w is not read); indices [n][triangle_stride][3], mesh-local; normals
 * [n][vertex_stride][3].  Every f32 operation once, in the reference's order, nothing fused:
 *   per triangle t, normal = normalized(cross(p1 - p0, p2 - p0)) -- vek's cross; the dot product left to right, a square root and
 *   three divisions, all correctly rounded.  Per vertex the sum STARTS AT +0.0 (a lone face normal with a -0.0 component comes out as
 *   +0.0) and takes the normals of the triangles that name it IN ASCENDING TRIANGLE INDEX; a vertex named twice by one triangle is
 *   added twice and counted twice.  With count > 0 the normal is normalized(sum / (count as f32)), with count == 0 it is
 *   (+0.0, +0.0, +0.0).
 * Kept as it is: a degenerate triangle is 0 / 0 = NaN in all three components and poisons its three vertices (a NaN is a NaN: sign and
 * payload are the device's); a sum of length zero divides by zero.  Float addition is not associative: the device adds a vertex's
 * normals in one thread, in that order, without atomics.
 * Written: exactly the first counts[i][0] normals of mesh i; slots past a mesh's counts are NOT written (and never read).
 * Two routes, chosen per call from triangle_stride: at or below the bound (RXR_VERTEX_NORMALS_SMALL_MAX in the environment, read at
 * each call, overrides it; 0 sends everything through the general route; a workgroup holds at most 6825 triangles) one workgroup per
 * mesh with the triangles in LDS, above it face normals in scratch, one stable sort of the corners by (mesh, vertex) and one thread
 * per vertex over its segment.  The bytes are the same.  The call is split into launches of a bounded number of triangle and vertex
 * slots, at least one mesh (RXR_VERTEX_NORMALS_LAUNCH_SLOTS overrides the bound).  Changes no frame, pool, picking or mesh state.
 * Replaces: Batch3D::compute_vertex_normals, src/batch/batch3d.rs:771-809 (Scene::compute_static_normals / compute_dynamic_normals,
 * src/scene.rs:203-215, call it per batch). */
#define RXR_VERTEX_NORMALS_ROUTE_SMALL 1
#define RXR_VERTEX_NORMALS_ROUTE_GENERAL 2
/* what rxr_vertex_normals refuses in its counts and indices, without a context: RXR_OK, or RXR_ERR_INVALID and in `message` (cut to
 * message_capacity, NUL-terminated; may be NULL) the first offending mesh and why -- a count above its stride, an index not below its
 * mesh's vertex count -- or: NULL counts / indices with non-zero work, byte sizes that overflow. */
int rxr_check_vertex_normals(const uint32_t *counts, const uint32_t *indices, uint32_t n, uint32_t vertex_stride, uint32_t triangle_stride,
                             char *message, uint32_t message_capacity);
/* Host memory, blocking.  Validates before anything is queued: whatever rxr_check_vertex_normals refuses, or NULL vertices / normals
 * with vertex_stride > 0, is RXR_ERR_INVALID and NOTHING IS WRITTEN.  n == 0 does nothing.  Multi-device handles: member 0. */
int rxr_vertex_normals(rxr_ctx *ctx, uint32_t n, const uint32_t *counts /* [n][2] vertices, triangles */,
                       const float *vertices /* [n][VS][4] */, const uint32_t *indices /* [n][TS][3], mesh-local */,
                       float *normals /* [n][VS][3] */, uint32_t vertex_stride, uint32_t triangle_stride);
/* the same on DEVICE arrays (each one's first and last byte are checked to be memory of the context's device; 4-byte aligned; an array
 * of 0 bytes is not looked at), queued on hip_stream (NULL = the context's stream): behind a producer of vertices and before
 * rxr_update_meshes_to on one stream, no geometry crosses PCIe.  Asynchronous.  The counts are device memory, so this form cannot
 * refuse after the fact; instead it never reads out of range: a mesh whose counts exceed the strides is SKIPPED WHOLE (none of its
 * normals are written), a triangle with an index at or above its mesh's vertex count contributes to no vertex.  dev_refused [n] (may
 * be NULL) receives per mesh the number of triangles refused that way: 0 for a clean mesh, 0xFFFFFFFF for a skipped one.
 * RXR_ERR_INVALID: a pointer that fails the check, byte sizes that overflow.  Multi-device handles: RXR_ERR_UNSUPPORTED (use rxr_member). */
int rxr_vertex_normals_to(rxr_ctx *ctx, uint32_t n, const uint32_t *dev_counts, const float *dev_vertices,
                          const uint32_t *dev_indices, float *dev_normals, uint32_t *dev_refused /* [n], may be NULL */,
                          uint32_t vertex_stride, uint32_t triangle_stride, void *hip_stream);

/* ---- generated terrain heights: TerrainGenerator::sample_height_at (rusterix_amd/csrc/rxr_terrain_gen.hip) ------------------------
 * The height field the 3D chunk builder and the region server evaluate (src/chunkbuilder/terrain_generator.rs:57-163, :488-509):
 * per point the maximum of a smoothstep cone per control vertex times the map-edge falloff (interpolate_height_at, :650-714,
 * calculate_map_edge_falloff, :718-743), plus the ridge sectors' heights by the distance to their polygon edges
 * (calculate_ridge_height_at, :513-550), pulled towards the road and river linedefs in list order (apply_linedef_smoothing,
 * :555-623).  Every f32 operation once, in the reference's order, divisions and square roots correctly rounded: the bits are the
 * reference's, except behind a powf (the ridge and linedef falloffs), which is the device's libm call.  Kept as it is: the
 * exact-match scan (magnitude < 1e-6) runs over ALL control points before the cones, the first in list order wins and returns
 * height * edge_factor without the cones (ridges and linedefs still apply); with no control point the base is 0.0 without the edge
 * factor; the maximum starts at +0.0 and takes a contribution only under `>` (negative and NaN contributions never count);
 * f32::min skips a NaN, so a ridge without edges is at distance +inf and contributes 0.0; clamp(0.0, 1.0) keeps a NaN and -0.0;
 * ridge contributions are added and linedefs folded in list order, a linedef only when its influence > 0.0, the over-influence
 * correction last.  TerrainConfig's idw_power and max_influence_distance are read by nothing in the reference and do not cross this
 * boundary; apply_exclusions is rxr_generated_meshes below and partition_by_tiles rxr_generated_tile_meshes behind it
 * (mesh_fix_winding never swaps such a mesh); the blend batches stay host work. */
#define RXR_TERRAIN_GEN_CONTROL_POINT_FLOATS 4u /* x, y, height, smoothness (the caller has applied config.smoothness's default)   */
#define RXR_TERRAIN_GEN_RIDGE_FLOATS 4u         /* height, plateau_width, falloff_distance, falloff_steepness                      */
#define RXR_TERRAIN_GEN_RIDGE_EDGE_FLOATS 4u    /* x0, y0, x1, y1, in the sector's linedef order                                    */
#define RXR_TERRAIN_GEN_LINEDEF_FLOATS 9u       /* the reference's tuple of seven: start (x, y), end (x, y), start_height,
                                                   end_height, width, falloff_distance, falloff_steepness                          */
#define RXR_TERRAIN_GEN_MAX_CONTROL_POINTS (1u << 16)
#define RXR_TERRAIN_GEN_MAX_RIDGES (1u << 12)
#define RXR_TERRAIN_GEN_MAX_RIDGE_EDGES (1u << 16)
#define RXR_TERRAIN_GEN_MAX_LINEDEFS (1u << 14)
/* validation only, no context: the status rxr_set_terrain_generator would return and, in `message`, the reason.
 * RXR_ERR_UNSUPPORTED: a count above its RXR_TERRAIN_GEN_MAX_*.  RXR_ERR_INVALID: a NULL array with a non-zero count, a NULL
 * map_box, ridge_edge_offsets that do not start at 0, decrease or do not end at n_ridge_edges, edges without a ridge. */
int rxr_check_terrain_generator(const float *control_points, uint32_t n_control_points, const float *ridges, uint32_t n_ridges,
                                const uint32_t *ridge_edge_offsets, const float *ridge_edges, uint32_t n_ridge_edges,
                                const float *linedefs, uint32_t n_linedefs, const float map_box[4], char *message,
                                uint32_t message_capacity);
/* makes the lists TerrainGenerator::generate collects (:255-294) resident, flattened by the caller (they stay until the next call).
 * The caller skips a sector or an edge the reference would skip for a missing id.  map_box: (min.x, min.y, max.x, max.y) after the
 * reference's flip of y, or its +-100 fallback.  Every count may be 0 and any f32 bit pattern is legal in a record.  What does not
 * depend on the point (a segment's direction, squared length and degenerate test, a control point's doubled radius, a linedef's
 * height difference) is computed here, once, in the reference's f32 operations.  Re-registration waits for queued evaluations.
 * Independent of rxr_set_terrain and rxr_set_terrain_heights.  Arrays are read before the call returns.  A refused call leaves
 * the resident records as they were.  Multi-device handles: member 0.
 * Replaces: collect_control_points / collect_ridge_sectors / collect_terrain_linedefs per call, :57-154, :325-435. */
int rxr_set_terrain_generator(rxr_ctx *ctx, const float *control_points /* [n_control_points][4] */, uint32_t n_control_points,
                              const float *ridges /* [n_ridges][4] */, uint32_t n_ridges,
                              const uint32_t *ridge_edge_offsets /* [n_ridges + 1]: ridge r owns edges [r] .. [r + 1] */,
                              const float *ridge_edges /* [n_ridge_edges][4] */, uint32_t n_ridge_edges,
                              const float *linedefs /* [n_linedefs][9] */, uint32_t n_linedefs, const float map_box[4]);
/* n points [n][2] against the resident records: heights [n] = sample_height_at; normals [n][3] (may be NULL) = sample_normal_at
 * (:166-181): the heights at p, p + (0.1, 0.0) and p + (0.0, 0.1) in the same launch, the tangents' cross product, normalised as
 * vek does it.  A NaN where the reference has one; its sign and payload are the device's.  RXR_ERR_INVALID: no
 * rxr_set_terrain_generator yet, or a NULL required pointer; n == 0 does nothing.  Host memory, blocking.  The call is split into
 * launches of bounded work, points x records (RXR_TERRAIN_GEN_LAUNCH_POINTS in the environment, read at each call, overrides the
 * points a launch).  Changes no frame, scratch, bake, picking or mesh state.  Multi-device handles: member 0.
 * Replaces: TerrainGenerator::sample_height_at / sample_normal_at, :57-181; src/server/region.rs:2059-2066. */
int rxr_generated_heights(rxr_ctx *ctx, const float *points, uint32_t n, float *heights, float *normals);
/* the same on DEVICE arrays (each given array's first and last byte are checked to be memory of the context's device; 4-byte
 * aligned), queued on hip_stream (NULL = the context's stream).  Asynchronous.  Multi-device handles: RXR_ERR_UNSUPPORTED. */
int rxr_generated_heights_to(rxr_ctx *ctx, const float *dev_points, uint32_t n, float *dev_heights, float *dev_normals,
                             void *hip_stream);
/* the grids of generate_grid (:460-485) for n chunk boxes [n][4] = (min.x, min.y, max.x, max.y) in one call: with cell_size =
 * 1.0 / subdivisions as f32 and the floor of min / the ceil of max, steps = ceil((max - min) / cell_size) as i32 + 1 per axis and
 * the point (ix, iy) is (min_x + ix as f32 * cell_size, min_y + iy as f32 * cell_size), made on the device.  counts [n][2] =
 * (steps_x, steps_y) of box i, a negative one as 0 (the grid is then empty; an extent whose `as i32` saturates wraps to a negative
 * step with the `+ 1`, as a release build of the reference does: an infinite box is an empty grid, not an error); heights of box i start at heights + i * stride, in
 * the reference's iy-major order; slots past steps_x * steps_y are NOT written.  RXR_ERR_INVALID: no rxr_set_terrain_generator
 * yet, subdivisions == 0, a NULL pointer, a box whose grid exceeds `stride` points (nothing is queued then), sizes that overflow.
 * n == 0 does nothing.  Host memory, blocking.  Launches and state as rxr_generated_heights.  Multi-device handles: member 0.
 * Replaces: generate_grid and interpolate_heights, :460-509. */
int rxr_generated_grids(rxr_ctx *ctx, const float *boxes, uint32_t n, uint32_t subdivisions, uint32_t stride, uint32_t *counts,
                        float *heights);
/* the same into DEVICE arrays, queued on hip_stream (NULL = the context's stream); boxes is host memory and is read before the
 * call returns.  Asynchronous.  Multi-device handles: RXR_ERR_UNSUPPORTED (use rxr_member). */
int rxr_generated_grids_to(rxr_ctx *ctx, const float *boxes, uint32_t n, uint32_t subdivisions, uint32_t stride,
                           uint32_t *dev_counts, float *dev_heights, void *hip_stream);

/* ---- generated terrain meshes: TerrainGenerator::apply_exclusions (rusterix_amd/csrc/rxr_terrain_excl.hip) ----------------------------
 * The vertices of a generated chunk (src/chunkbuilder/terrain_generator.rs:747-825) with the sectors of terrain_mode == 1 cut out.
 * A sector is ACTIVE for a chunk box iff its bounding box intersects the box as given (collect_excluded_sectors, :438-457;
 * BBox::intersects, src/map/bbox.rs:43-48: four <= / >= comparisons, touching counts, a NaN makes it inactive).  A sector with
 * fewer than three vertices is active like any other and holds no point.
 *   no active sector   the SHARED layout: vertex i is grid point i, [x, h, y, 1.0], in grid order; its triangles are the closed form
 *                      triangulate (per cell, row by row, (i0, i2, i1) and (i1, i2, i3))
 *   otherwise          the UNSHARED layout: the triangles of that closed form in its order, but for those whose three corners lie
 *                      inside ONE active sector (corners inside different sectors do not drop a triangle); a kept triangle is its
 *                      three vertices one after the other, its indices base, base + 1, base + 2
 * point_in_sector (:891-950) over the polygon of the sector's vertices in order: inside iff the point lies within 0.01 of an edge
 * of squared length > 0.0 (t clamped as f32::clamp does), or else by the parity of the ray cast, whose crossing abscissa is
 * multiplied, divided, added as written.  Every keep / drop decision, count, x and z are the reference's to the bit; h is the word
 * rxr_generated_grids gives for that grid point (the same device function).  uvs are [x, z] and do not cross this boundary. */
#define RXR_TERRAIN_GEN_MAX_EXCLUDED_SECTORS (1u << 12)
#define RXR_TERRAIN_GEN_MAX_EXCLUSION_VERTICES (1u << 16)
/* validation only, no context: the status rxr_set_terrain_exclusions would return and, in `message`, the reason.
 * RXR_ERR_UNSUPPORTED: a count above its RXR_TERRAIN_GEN_MAX_*.  RXR_ERR_INVALID: a NULL array with a non-zero count,
 * vertex_offsets that do not start at 0, decrease or do not end at n_vertices, vertices without a sector. */
int rxr_check_terrain_exclusions(const float *sector_boxes, const uint32_t *vertex_offsets, const float *vertices,
                                 uint32_t n_sectors, uint32_t n_vertices, char *message, uint32_t message_capacity);
/* makes the map's sectors of terrain_mode == 1 resident, flattened by the caller (they stay until the next call; n_sectors == 0 is
 * legal and clears them).  sector_boxes: (min.x, min.y, max.x, max.y) as the reference's sector.bounding_box computes it; a sector's
 * vertices: its linedefs' start vertices in linedef order, missing linedefs and vertices skipped, possibly none.  Any f32 bit
 * pattern is legal.  What does not depend on the point (an edge's vj - vi, its squared length and the > 0.0 test) is computed here,
 * once, in the reference's f32 operations.  Re-registration waits for queued mesh calls.  Independent of
 * rxr_set_terrain_generator.  Arrays are read before the call returns.  A refused call leaves the resident sectors as they were.
 * Multi-device handles: member 0.
 * Replaces: collect_excluded_sectors per chunk, :438-457, and the vertex walk of point_in_sector per call, :893-900. */
int rxr_set_terrain_exclusions(rxr_ctx *ctx, const float *sector_boxes /* [n_sectors][4] */,
                               const uint32_t *vertex_offsets /* [n_sectors + 1]: sector s owns vertices [s] .. [s + 1] */,
                               const float *vertices /* [n_vertices][2] */, uint32_t n_sectors, uint32_t n_vertices);
/* the meshes of n chunk boxes [n][4] = (min.x, min.y, max.x, max.y) in one call, grids as in rxr_generated_grids.  counts [n][4] =
 * (steps_x, steps_y, active_sectors, n_vertices) of box i; its vertices start at vertices + i * stride * 4, [x, h, y, 1.0] each (the
 * layout rxr_terrain_meshes writes).  active_sectors == 0: the shared layout, n_vertices = steps_x * steps_y; otherwise the unshared
 * one, n_vertices = 3 * kept triangles.  Slots past n_vertices are NOT written.  A grid with a negative or zero step is empty.
 * RXR_ERR_INVALID, before anything is queued: no rxr_set_terrain_generator yet, subdivisions == 0, a NULL pointer, sizes that
 * overflow, a box whose layout can exceed `stride` vertices (6 * (steps_x - 1) * (steps_y - 1) where a sector is active, else
 * steps_x * steps_y).  No rxr_set_terrain_exclusions yet is n_sectors == 0.  n == 0 does nothing.  Host memory, blocking.  The call
 * is cut into rounds of two launches (classification, emission) over a bounded number of points
 * (RXR_TERRAIN_EXCL_LAUNCH_POINTS in the environment, read at each call, overrides it).  Changes no frame, scratch, bake, picking
 * or mesh state.  Multi-device handles: member 0.
 * Replaces: generate_grid, interpolate_heights and apply_exclusions, :460-509, :747-825. */
int rxr_generated_meshes(rxr_ctx *ctx, const float *boxes, uint32_t n, uint32_t subdivisions, uint32_t stride, uint32_t *counts,
                         float *vertices);
/* the same into DEVICE arrays (each one's first and last byte are checked to be memory of the context's device; 4-byte aligned),
 * queued on hip_stream (NULL = the context's stream); boxes is host memory and is read before the call returns.  Asynchronous.
 * Multi-device handles: RXR_ERR_UNSUPPORTED (use rxr_member). */
int rxr_generated_meshes_to(rxr_ctx *ctx, const float *boxes, uint32_t n, uint32_t subdivisions, uint32_t stride,
                            uint32_t *dev_counts, float *dev_vertices, void *hip_stream);

/* ---- generated terrain tile meshes: TerrainGenerator::partition_by_tiles (rusterix_amd/csrc/rxr_terrain_excl.hip) --------------------
 * The last step of TerrainGenerator::generate (src/chunkbuilder/terrain_generator.rs:954-1034) over the (vertices, indices, uvs) of
 * apply_exclusions above, uvs[i] = [v.x, v.z]: one mesh per tile, with its uvs and mesh-local indices, in the strided layout
 * rxr_vertex_normals[_to] and rxr_update_meshes[_to] read -- so that on ONE stream
 *     rxr_generated_tile_meshes_to -> rxr_vertex_normals_to -> rxr_update_meshes_to
 * takes the dirty chunks of a generated terrain to the renderer and no geometry crosses PCIe (moving a control point changes
 * heights and no count: which triangles survive, and which tile one belongs to, depend on x and z alone).
 *   per triangle, in index order   center_u = (uv0[0] + uv1[0] + uv2[0]) / 3.0 -- added left to right, then divided, every operation
 *                      rounded to f32, no reciprocal --, center_v likewise; tile_cell = (center_u.floor() as i32, center_v.floor()
 *                      as i32) (saturating, a NaN is 0); its TILE SLOT is the one registered for that cell, else slot 0.
 *   per tile           its triangles in ascending triangle order; the vertex list is built by FIRST USE, walking those triangles'
 *                      corners in order: a vertex not seen before in this tile gets the next index and is copied with its uv; a vertex
 *                      two tiles share is copied into both.
 * Which tile a cell's pixel source resolves to (tile_from_tile_list, else the default) is the caller's knowledge and stays on the
 * host: the caller numbers its tiles, slot 0 being the default tile, and registers cells with slots.
 * GROUP ORDER.  The reference returns the tiles in the iteration order of a hash map, which is unspecified; here it is defined: the
 * groups of a box are in ASCENDING TILE SLOT, and a group exists iff at least one kept triangle has that slot.
 * mesh_fix_winding (src/chunkbuilder/surface_mesh_builder.rs:201-239), which the reference's consumer runs on every group, never
 * swaps a generated mesh and is not run (DESIGN.md section 21 has the argument, tests/test_terrain_tiles_cpu.py holds it).  The
 * consumer's uv flip, its second grouping by GeoId and the blend batches stay host work.
 * Every count, slot, index, x, z and uv is the reference's to the bit; h is the word rxr_generated_grids gives for that grid point. */
#define RXR_TERRAIN_TILES_MAX_CELLS (1u << 20)
#define RXR_TERRAIN_TILES_MAX_TILES (1u << 12)
#define RXR_TERRAIN_TILES_MAX_GROUPS 64u
/* validation only, no context: the status rxr_set_terrain_tiles would return and, in `message`, the reason.  RXR_ERR_UNSUPPORTED:
 * n_cells above RXR_TERRAIN_TILES_MAX_CELLS, n_tiles above RXR_TERRAIN_TILES_MAX_TILES.  RXR_ERR_INVALID: n_tiles == 0, a NULL array
 * with a non-zero count, a slot >= n_tiles, a cell listed twice. */
int rxr_check_terrain_tiles(const int32_t *cells, const uint32_t *slots, uint32_t n_cells, uint32_t n_tiles, char *message,
                            uint32_t message_capacity);
/* makes the tile overrides resident: cell i = (x, z) of a 1 x 1 world cell has tile slot slots[i] < n_tiles; every other cell has
 * slot 0.  The cells may come in any order (they are sorted here, the device searches them).  n_cells == 0 is legal: everything is
 * slot 0; never called is n_cells == 0, n_tiles == 1.  Replaces the previous map; waits for queued tile-mesh calls.  Independent of
 * rxr_set_terrain_generator and rxr_set_terrain_exclusions.  Arrays are read before the call returns.  A refused call leaves the
 * resident map as it was.  Multi-device handles: member 0. */
int rxr_set_terrain_tiles(rxr_ctx *ctx, const int32_t *cells /* [n_cells][2] */, const uint32_t *slots /* [n_cells] */,
                          uint32_t n_cells, uint32_t n_tiles);
/* the tile meshes of n chunk boxes [n][4] in one call, grids, heights and exclusions as in rxr_generated_meshes.  Mesh slot
 * m = box * max_groups + group:
 *   box_counts  [n][4]                            (steps_x, steps_y, active_sectors, n_groups)
 *   counts      [n * max_groups][2]               (n_vertices, n_triangles); (0, 0) for a group slot at or past n_groups
 *   group_tiles [n * max_groups]                  the group's tile slot; 0xFFFFFFFF past n_groups
 *   vertices    [n * max_groups][vertex_stride][4]      [x, h, z, 1.0]
 *   uvs         [n * max_groups][vertex_stride][2]      [x, z]
 *   indices     [n * max_groups][triangle_stride][3]    mesh-local
 * box_counts, counts and group_tiles are written whole; vertex, uv and index slots past a mesh's counts are NOT written.  A grid
 * without a cell (a step below 2) has no triangle and so no group.
 * Refused before anything is queued, with nothing written -- RXR_ERR_INVALID: no rxr_set_terrain_generator yet, subdivisions == 0,
 * max_groups == 0, a NULL pointer, sizes that overflow, a box with 2 * cells > triangle_stride or whose one group can exceed
 * vertex_stride (cells = (steps_x - 1) * (steps_y - 1); 6 * cells where a sector is active, else steps_x * steps_y: one group can
 * own the whole box), a box that CAN have more than max_groups groups; RXR_ERR_UNSUPPORTED: max_groups above
 * RXR_TERRAIN_TILES_MAX_GROUPS.  The group bound is conservative: slot 0 plus the distinct non-zero slots among the override cells
 * between the floor of the grid's first and the ceil of its last coordinate on both axes -- whether or not slot 0 occurs, and
 * counting override cells whose triangles all end up excluded.  A box can therefore be refused that would have fitted.  (With
 * coordinates so large that a centre's rounding is not small against a third of a cell, every registered slot counts.)
 * n == 0 does nothing.  Host memory, blocking.  Rounds as rxr_generated_meshes: a classification and a tile emission launch each,
 * RXR_TERRAIN_EXCL_LAUNCH_POINTS cuts them too.  Changes no frame, bake, picking or mesh state.  Multi-device handles: member 0.
 * Replaces: generate_grid .. partition_by_tiles, :460-509, :747-879, :954-1034, and mesh_fix_winding per group. */
int rxr_generated_tile_meshes(rxr_ctx *ctx, const float *boxes, uint32_t n, uint32_t subdivisions, uint32_t max_groups,
                              uint32_t vertex_stride, uint32_t triangle_stride, uint32_t *box_counts, uint32_t *counts,
                              uint32_t *group_tiles, float *vertices, float *uvs, uint32_t *indices);
/* the same into DEVICE arrays (each one's first and last byte are checked to be memory of the context's device; 4-byte aligned),
 * queued on hip_stream (NULL = the context's stream); boxes is host memory and is read before the call returns.  Asynchronous.
 * Multi-device handles: RXR_ERR_UNSUPPORTED (use rxr_member). */
int rxr_generated_tile_meshes_to(rxr_ctx *ctx, const float *boxes, uint32_t n, uint32_t subdivisions, uint32_t max_groups,
                                 uint32_t vertex_stride, uint32_t triangle_stride, uint32_t *dev_box_counts, uint32_t *dev_counts,
                                 uint32_t *dev_group_tiles, float *dev_vertices, float *dev_uvs, uint32_t *dev_indices,
                                 void *hip_stream);

/* ---- path tracing the resident scene: Tracer::trace (rusterix_amd/csrc/rxr_trace.hip) ----------------------------------------------
 * The reference's second renderer (src/tracer/trace.rs:105-475 into an AccumBuffer, src/tracer/buffer.rs) over the meshes of
 * rxr_set_meshes and the tiles of rxr_set_textures, as it stands (DESIGN.md section 18 has the derivation):
 *   camera   per pixel (x, y): screen_uv = (x / width, 1 - y / height), jitter = (rand, rand), then the per-pixel part of the camera's
 *            create_ray (src/camera/d3firstp.rs:112-138, d3orbit.rs:117-153, d3iso.rs:159-182) from 14 host-computed floats: position,
 *            forward, right, up (3 each), half_width, half_height -- what create_ray computes before it looks at uv (their tan,
 *            normalized and cross run on the host; half_width includes the aspect; iso: position = the camera's position(), forward =
 *            (center - position).normalized(), right and up = basis()'s, half_height = scale, half_width = scale *
 *            max(width / height, 1e-6)).
 *   hit      Batch3D::intersect(ray, false) per mesh, folded by `hit.t < best.t` in rxr_set_meshes order over the lists RXR_LIST_CHUNK,
 *            _CHUNK_TERRAIN, _STATIC and _DYNAMIC: rxr_intersect's RXR_INTERSECT_FULL under its plain rule, profile ids ignored.  The
 *            opacity and overlay lists are not looked at.  (The reference walks scene.chunks in hash-map order; the mesh order is
 *            this library's definition.  Its intersects_aabb pre-tests only cull and are left out.)
 *   texel    evaluate_hit (:377-475): RXR_SOURCE_PIXEL; a static / dynamic tile at animation_frame % n_textures sampled at the hit's uv
 *            with sample_mode and the mesh's repeat mode; RXR_SOURCE_TERRAIN in a chunk: chunk.sample_terrain_texture at (w.x, w.z) of
 *            ray.at(t) from the chunk's resident terrain texture (rxr_set_chunk_textures; no texture: zero); anything else is zero.  tex_lin = srgb_to_linear(texel) through a table of
 *            256 floats built on the host (rxr_trace_srgb_table); albedo = tex_lin.xyz.
 *   material per mesh (role, modifier, value), role RXR_TRACE_NO_MATERIAL for None: value' = modifier.modify(texel, value)
 *            (src/shapestack/material.rs:80-110; modifiers 0 None, 1 Luminance, 2 Saturation, 3 InvLuminance, 4 InvSaturation); roles
 *            0 Matte: specular_weight = 1 - value', 1 Glossy and 2 Metallic: = value', 3 Transparent: nothing, 4 Emissive: emissive =
 *            tex_lin.xyz * value * 10 (the unmodified value).
 *   bounce   (:272-331) emissive != 0: ret += emissive * throughput, the path ends.  Else ret += (sum of radiance_at(world, normal,
 *            hash_u32(animation_frame)) * 10 over `lights`) * (throughput * (albedo / PI)); p_spec = specular_weight.clamp(0, 1);
 *            rand < p_spec: dir = reflect(dir, normal), throughput *= specular_weight / p_spec; else dir = sample_cosine(normal),
 *            throughput *= (albedo * p_diff) / (p_diff * PI); origin = origin + dir * t + normal * 0.01 WITH THE NEW dir (the reference
 *            assigns ray.dir first); p = max(throughput).clamp(0.001, 1), the path ends when rand > p, else throughput *= 1 / p.  A
 *            miss ends the path and adds nothing (no render graph: the sky of render_miss_d3 is out of scope).
 *   average  per call frame f = first_frame + k: t = 1 / (f + 1), accum = accum * (1 - t) + (ret.x, ret.y, ret.z, 1) * t, unfused.
 * Random numbers: the reference draws from an OS-seeded generator whose stream is unspecified; this one is counter-based, a sample
 * depends on (seed, frame, pixel index y * width + x, slot) alone:
 *   pcg(v): s = v * 747796405 + 2891336453; w = ((s >> ((s >> 28) + 4)) ^ s) * 277803737; return (w >> 22) ^ w      (all u32, wrapping)
 *   u32 = pcg(pcg(pcg(seed + frame) + pixel) + slot);   f32 = (u32 >> 8) as f32 * 2^-24, in [0, 1)                (rand's f32)
 * Slots 0, 1: the jitter; bounce b: 2 + 4 b + (0 specular choice, 1 r1, 2 r2, 3 roulette), spent whether or not the branch runs.
 * No libm function runs on the device before a path's first diffuse bounce (the cos and sin of sample_cosine); up to there every
 * float is the reference's.  acos (spot lights) is the device's as in the rasterizer's exact light loop. */
#define RXR_TRACE_CAMERA_FIRSTP 0
#define RXR_TRACE_CAMERA_ORBIT 1
#define RXR_TRACE_CAMERA_ISO 2
#define RXR_TRACE_CAMERA_FLOATS 14    /* position, forward, right, up (3 each), half_width, half_height */
#define RXR_TRACE_NO_MATERIAL 4294967295u
#define RXR_TRACE_MAX_BOUNCES 8       /* the reference's constant; the generator's slots are laid out for it */
#define RXR_TRACE_MAX_LIGHTS 4096     /* the light list is walked per hit by every path: a bound on a record the kernel takes whole */
/* validation only, no context: what rxr_set_trace_scene checks without looking at the registered meshes.  RXR_ERR_INVALID: lights
 * NULL with n_lights > 0, a light type, material role (0..4 or RXR_TRACE_NO_MATERIAL) or modifier (0..4) out of range, an unknown
 * sample mode, material_kinds given without material_values or the reverse.  RXR_ERR_UNSUPPORTED: n_lights above
 * RXR_TRACE_MAX_LIGHTS. */
int rxr_check_trace_scene(const uint32_t *material_kinds, const float *material_values, uint32_t n_meshes, const rxr_light *lights,
                          uint32_t n_lights, uint32_t sample_mode, char *message, uint32_t message_capacity);
/* what the tracer reads besides meshes and textures (stays until the next call, or the next rxr_set_meshes / rxr_set_textures, which
 * drop it): material_kinds [n_meshes][2] = (role, modifier) and material_values [n_meshes], both NULL for no materials; the lights
 * the reference chains (scene.lights, then scene.dynamic_lights; chunk lights are NOT part of it); the tracer's sample mode;
 * scene.animation_frame; chunk_origin_size [n_chunks][3] = chunk.origin.x, chunk.origin.y, chunk.size of every chunk a terrain-sourced
 * mesh lies in (NULL with n_chunks 0 when there is none; the textures themselves are those of rxr_set_chunk_textures, which drops the
 * trace scene as well).  n_meshes must equal the count of the last rxr_set_meshes (RXR_ERR_INVALID).  RXR_ERR_INVALID as well: a
 * participating mesh whose tile does not exist or has no texture, or whose chunk's size is below 1 (the reference panics), or whose
 * chunk chunk_origin_size does not reach.  RXR_ERR_UNSUPPORTED: a participating mesh of source RXR_SOURCE_TERRAIN while no resident
 * chunk texture is registered for its chunk.  A refused call leaves the previous trace scene as it was.  Blocking.  Multi-device
 * handles: member 0. */
int rxr_set_trace_scene(rxr_ctx *ctx, const uint32_t *material_kinds, const float *material_values, uint32_t n_meshes,
                        const rxr_light *lights, uint32_t n_lights, uint32_t sample_mode, uint64_t animation_frame,
                        const int32_t *chunk_origin_size, uint32_t n_chunks);
/* the 256 floats srgb_to_linear(byte * (1 / 255)) every context uses (trace.rs:14-20; the host's powf, built once per process: ctx
 * may be NULL) */
int rxr_trace_srgb_table(rxr_ctx *ctx, float out[256]);
/* the generator above as the kernels run it, evaluated on the host (no context, no device): a host's CPU path of the same loop and
 * the tests draw from it */
float rxr_trace_rand(uint32_t seed, uint32_t frame, uint32_t pixel, uint32_t slot);
/* n_frames samples of every pixel, averaged into accum (host memory, [height][width][4], in/out) as frames first_frame ..
 * first_frame + n_frames - 1, without going back to the host in between.  camera: RXR_TRACE_CAMERA_FLOATS floats.  RXR_ERR_INVALID:
 * a NULL pointer, width, height or n_frames of 0, more than 2^24 pixels a side or 2^28 in all, an unknown camera kind, no
 * rxr_set_trace_scene for the current meshes.  RXR_ERR_UNSUPPORTED: bounces above RXR_TRACE_MAX_BOUNCES.  A refused call leaves accum
 * untouched.  bounces == 0 averages black.  A trace changes no frame state: a frame uploaded before it renders as it would have.
 * Blocking.  Multi-device handles: member 0.
 * Replaces: Tracer::trace, src/tracer/trace.rs:105-375, once per frame. */
int rxr_trace(rxr_ctx *ctx, uint32_t camera_kind, const float *camera, uint32_t width, uint32_t height, uint32_t first_frame,
              uint32_t n_frames, uint32_t seed, uint32_t bounces, float *accum);
/* the same on DEVICE memory (first and last byte are checked to be memory of the context's device; 16-byte aligned), queued on
 * hip_stream (NULL = the context's stream); camera is host memory and is read before the call returns.  Asynchronous.  Multi-device
 * handles: RXR_ERR_UNSUPPORTED (use rxr_member). */
int rxr_trace_to(rxr_ctx *ctx, uint32_t camera_kind, const float *camera, uint32_t width, uint32_t height, uint32_t first_frame,
                 uint32_t n_frames, uint32_t seed, uint32_t bounces, float *dev_accum, void *hip_stream);
/* AccumBuffer::to_u8_vec (src/tracer/buffer.rs:68-91): per colour channel x <= 0.0031308 ? x * 12.92 : 1.055 * x.powf(1 / 2.4) -
 * 0.055, then (srgb.clamp(0, 1) * 255 + 0.5) as u8; alpha (a.clamp(0, 1) * 255 + 0.5) as u8.  powf is the device's: a channel whose
 * exact value lies within its error of an integer may differ from a host's by one.  accum and rgba ([height][width][4] bytes) are
 * host memory; blocking.  Multi-device handles: member 0. */
int rxr_accum_to_rgba(rxr_ctx *ctx, const float *accum, uint32_t width, uint32_t height, uint8_t *rgba);
/* the same on DEVICE memory, queued on hip_stream (NULL = the context's stream).  Multi-device handles: RXR_ERR_UNSUPPORTED. */
int rxr_accum_to_rgba_to(rxr_ctx *ctx, const float *dev_accum, uint32_t width, uint32_t height, uint8_t *dev_rgba, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* RXR_H */
