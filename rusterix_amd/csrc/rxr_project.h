// rxr_project.h -- data layout of the device-side projection path:
// Batch3D::clip_and_project + Edges::new + bounding box on the GPU.  See rxr_project.hip.
#pragma once
#include <stdint.h>

#ifdef RXR_JIT
#include "rxr.h"  // (hiprtc: the sources are in-memory headers with plain names, rxr_jit.hip)
#else
#include "../../include/rxr.h"
#endif
#include "rxr_device.h"

// Output layout per mesh (capacity based, so that triangle ids keep the reference's submission order
// without a cross-mesh compaction): vertices [vout_base, vout_base + n_verts + 4*n_tris),
// triangles [tout_base, tout_base + 3*n_tris).  The first n_verts / n_tris slots are the originals
// (copied by clip_and_project at batch3d.rs:566-574), the rest receives what near-plane clipping
// appends (:627-686) -- at most 4 vertices and 2 fan triangles per clipped triangle.
struct DevMesh {
    uint32_t vin_base, tin_base;    // into the object-space pools
    uint32_t n_verts, n_tris;
    uint32_t vout_base, tout_base;  // into the projected pools (the pools k_setup3d reads)
    uint32_t cull_mode;
    uint32_t rejected;              // per frame: the AABB frustum test dropped the batch (:493-552)
    float view_model[16];           // per frame: view * transform_3d (:555)
};  // 96 B

// bounding boxes are accumulated with integer atomics on an order-preserving encoding of f32
// One box per 128-byte line: atomics on one cache line serialise in L2, and with eight boxes to a line the 1 M-triangle grid
// queued 3 456 of them per line -- the whole run time of k_proj_vertices.
struct alignas(128) DevBBox {
    uint32_t min_x, min_y, max_x, max_y;
};

// prefix entry of the append scan: low 32 bits = vertices emitted before this triangle, high 32 bits =
// fan triangles emitted before it (both counted over ALL meshes; per-mesh offsets subtract the value
// at the mesh's first triangle)
typedef unsigned long long AppendCount;

#define RXR_PROJ_SCAN_CHUNK 8192u

struct ProjectParams {
    uint32_t n_meshes, n_verts_in, n_tris_in;  // totals over all meshes (object space)
    uint32_t n_tris_out;                       // total triangle capacity (sum of 3 * n_tris)
    uint32_t edges_in_setup;                   // 1: k_setup3d builds the Edges records itself (RasterParams.pm_meshes): no k_proj_edges launch
    float projection[16];
    float width, height;

    const DevMesh *meshes;
    const uint32_t *vin_prefix;   // n_meshes + 1: first object-space vertex of each mesh
    const uint32_t *tin_prefix;   // n_meshes + 1
    const uint32_t *tout_prefix;  // n_meshes + 1 (== the raster path's batch_tri_base)

    const float4 *obj_verts;
    const uint32_t *obj_idx;      // 3 per triangle, mesh-local
    const float2 *obj_uvs;
    const float *obj_normals;     // 3 per vertex

    float4 *view_verts;           // view space, indexed like the projected pool
    float4 *pv;                   // projected_vertices pool (output layout)
    float2 *uv;                   // clipped_uvs pool
    float *nrm;                   // clipped_normals pool
    uint32_t *idx;                // clipped_indices pool, 3 per triangle slot, mesh-local
    rxr_edges *edges;             // Edges pool, one per triangle slot
    uint8_t *edge_vis;            // per original triangle: edge_visibility (:582-618)
    AppendCount *append;          // per original triangle: this triangle's (verts, tris) then, after the scan, the exclusive prefix
    AppendCount *chunk_tot;       // scan scratch
    AppendCount *chunk_base;
    uint32_t *ticket;             // [0] scan last-block ticket (cleared by the last block); [1] "some triangle of the frame is clipped" (k_proj_init clears, k_clip_count raises)
    DevBBox *bbox;                // per mesh
    uint32_t *mesh_live;          // per mesh and frame: triangle slots in use = originals + appended fans (0 for a rejected mesh);
                                  // the slots behind them are dead: k_proj_edges, k_setup3d and k_fill skip whole workgroups of them
};

#if defined(__HIPCC__) || defined(RXR_JIT)
// (edges_from_xy, rxr_device.h: Edges::new behind the winding swap of the cull mode, shared with the host)
RXR_HD __forceinline__ rxr_edges edges_from_vertices(uint32_t cull_mode, bool evis, float4 v0, float4 v1, float4 v2) {
    return edges_from_xy(cull_mode, evis, v0.x, v0.y, v1.x, v1.y, v2.x, v2.y);
}
#endif

// ---- the 2D half: Batch2D::project (src/batch/batch2d.rs:373-425) + the Prim2D records rxr_upload_frame builds on the host ----------
struct DevMesh2D {
    uint32_t vin_base, n_verts;     // into the object-space 2D pools
    uint32_t mode;                  // RXR_MODE_*
    uint32_t line_color;            // Lines / LineStrip / LineLoop: the packed colour of every segment (:911-915)
};
struct Prim2DSrc {
    uint32_t mesh;                  // registered 2D mesh = batch index of the frame
    uint32_t ia, ib, ic;            // mesh-local vertex indices: a triangle's three, a segment's two
};
struct Project2DParams {
    uint32_t n_meshes, n_verts, n_prims, has_matrix;
    float m[9];                     // vek column-major Mat3 (m[c * 3 + r])
    float width, height;
    uint32_t ref_tile;              // the reference's tile_size (the box test of risky batches, rxr_device.h rxr_ref_tile_span)
    const DevMesh2D *meshes;
    const uint32_t *vin_prefix;     // n_meshes + 1
    const float2 *obj_verts, *obj_uvs;
    const Prim2DSrc *src;
    DevBBox *bbox;                  // per mesh and frame
    struct Prim2D *out;             // the frame blob's Prim2D records
    uint32_t *d2_box;               // min_x, max_x, min_y, max_y of the non-empty pixel boxes (RasterParams.d2_box_dev)
    uint32_t *bad_line;             // pinned status word: a segment end point beyond +-2^30 (the host builder refuses the frame)
};

// ---- rxr_update_meshes (include/rxr.h): some registered meshes' geometry replaced in place, counts unchanged ---------------------------
#define RXR_MESH_UPDATE_LAUNCH 256u   // named meshes per launch (1 KiB of kernel arguments)
// what k_mesh_check finds out about one named mesh; the host reads the records back and refuses the call if any status is set
enum : uint32_t { MESH_UPD_BAD_VERTS = 1u, MESH_UPD_BAD_TRIS = 2u, MESH_UPD_BAD_INDEX = 4u };
struct MeshCheckRec {
    uint32_t status;         // MESH_UPD_* (0: accepted)
    uint32_t bad_triangle;   // MESH_UPD_BAD_INDEX: the first triangle with a vertex index >= the vertex count
    float lo[3], hi[3];      // the object-space box of the new vertices (batch3d.rs:494-507): +-inf without a non-NaN coordinate
};  // 32 B
struct MeshUpdateArgs {
    const DevMesh *meshes;       // the registration's static array (bases and counts)
    // the caller's arrays in the layout of rxr_terrain_meshes, from this launch's first named mesh on
    const uint32_t *counts;      // [n][2]
    const float *vertices;       // [n][vstride][4]
    const uint32_t *indices;     // [n][tstride][3], mesh-local
    const float *normals;        // [n][vstride][3]
    uint32_t vstride, tstride;
    MeshCheckRec *rec;           // [n]
    // the pools (ProjectParams): object space at vin_base / tin_base, the static originals of the output pools at vout_base / tout_base
    float4 *obj_verts;
    uint32_t *obj_idx;
    float *obj_normals;
    float *nrm;
    uint32_t *idx;
    uint32_t mesh[RXR_MESH_UPDATE_LAUNCH];   // the named meshes, rxr_set_meshes order
};

// ---- rxr_resize_meshes (include/rxr.h): some registered meshes' geometry replaced when their counts change ------------------------------
// what k_mesh_resize_check finds out about one named mesh: MeshCheckRec plus the two counts (the host reads the caller's counts nowhere else)
enum : uint32_t { MESH_RSZ_BAD_VSTRIDE = 8u, MESH_RSZ_BAD_TSTRIDE = 16u };   // next to MESH_UPD_BAD_INDEX
struct MeshResizeRec {
    uint32_t status;         // MESH_RSZ_* | MESH_UPD_BAD_INDEX (0: accepted)
    uint32_t bad_triangle;   // MESH_UPD_BAD_INDEX: the first triangle with a vertex index >= the new vertex count
    float lo[3], hi[3];      // the object-space box of the new vertices: +-inf without a non-NaN coordinate
    uint32_t n_verts, n_tris;
};  // 40 B
struct MeshResizeCheckArgs {
    const uint32_t *counts;      // [n][2]
    const float *vertices;       // [n][vstride][4]
    const uint32_t *indices;     // [n][tstride][3], mesh-local
    uint32_t vstride, tstride;
    MeshResizeRec *rec;          // [n]
};
// k_mesh_repack: the NEW object pools from the old ones and the caller's arrays.  source [n_meshes][2]: for a named mesh
// (RXR_MESH_RESIZE_NAMED | its slot k in the caller's arrays, unused), for any other (its OLD vin_base, its OLD tin_base) -- bases are
// below 2^31 (rxr_set_meshes' limit), so the top bit is free.  The table lives in device memory: no cut at a number of named meshes.
#define RXR_MESH_RESIZE_NAMED 0x80000000u
struct MeshRepackArgs {
    uint32_t n_meshes, n_verts, n_tris;      // of the NEW registration
    const DevMesh *meshes;                   // the new static table (bases and counts)
    const uint32_t *vin_prefix, *tin_prefix; // the new prefix arrays, n_meshes + 1
    const uint32_t *source;
    // the old pools
    const uint4 *old_verts;
    const uint32_t *old_idx;
    const uint2 *old_uvs;
    const uint32_t *old_normals;
    // the caller's arrays (words: a NaN keeps its payload), 4-byte aligned; uvs may be null: [0, 0]
    const uint32_t *vertices, *uvs, *indices, *normals;
    uint32_t vstride, tstride;
    // the new pools
    uint4 *new_verts;
    uint32_t *new_idx;
    uint2 *new_uvs;
    uint32_t *new_normals;
};
