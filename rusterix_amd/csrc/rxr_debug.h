/* rxr_debug.h -- the test entry points of librxr_hip.so: every rxr_debug_* function a .hip file of this directory defines, declared once.
 * They are NOT part of the product ABI (include/rxr.h; only rxr_debug_d3_rows is declared there) and are not mirrored into the Rust
 * shim.  Every defining file includes this header, so the compiler rejects a definition that disagrees; the C tests (tests/abi_*.c)
 * include it, and tools/gen_ffi.py parses it into rusterix_amd/abi.py's DEBUG_SIGNATURES.  Plain C, block comments only (the parser). */
#ifndef RXR_DEBUG_H
#define RXR_DEBUG_H

#include "../../include/rxr.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- rxr_api.hip ---- */

/* tests: what rxr_upload_frame found out about the resident frame's extent: out[0] = content rows known, out[1], out[2] = the rows,
 * out[3] = row spans in use (1: from the host's boxes, 2: completed on the device) */
int rxr_debug_content(rxr_ctx *ctx, uint32_t *out);

/* tests: the scratch words the next launch assumes clear, read back after the context's streams have drained.  Checked:
 *   buffer 0: every word of d_bin_count -- bin_count (rxr_device.h RasterParams.bin_count: "all-zero between launches", k_raster hands its
 *             bin back) and k_blockscan's per-block group counts behind it (RasterParams.blk_cnt: "all-zero between launches: k_blockscan
 *             hands it back"); the rest of the allocation is zeroed when it is made (rxr_upload_frame) and never written;
 *   buffer 1: words CNT_LARGE and CNT_TICKET of the 3D counter set `parity` (render_impl: "counter set `parity` is clean (cleared by the
 *             previous launch's k_scan)"; the next launch adds to those two with atomics, CNT_ENTRIES / CNT_OVERFLOW it writes before use);
 *   buffer 2: the same words of the 2D set 2 + parity2d (cleared likewise by the previous 2D k_scan);
 *   buffer 3: every word of d_bin2d_count (RasterParams.bin2d_count: "own zero-invariant buffer, like bin_count").
 * out[0] = number of non-zero words, out[1..3] = buffer, word index, value of the first one (all 0 when clean).  A context whose last launch
 * sequence was cut short (scratch_dirty) is reported as it is: its next launch restores the invariants anyway.  Finding dirt marks the
 * context dirty, so that its next launch clears the buffers instead of building on them (a failed check leaves nothing behind). */
int rxr_debug_scratch(rxr_ctx *ctx, uint32_t *out);

/* tests (host only, no device): rxr_ref_tile_span (quick == 0) / rxr_ref_tile_span_quick of n boxes [lo, lo + extent] on one axis;
 * out: p0, p1 per box */
void rxr_debug_tile_spans(const float *lo, const float *extent, uint32_t n, uint32_t size, uint32_t ts, float pad, int quick, uint32_t *out);

/* tests: what the last banded rxr_render_download sent over PCIe and what the host wrote itself (bytes) */
int rxr_debug_download_bytes(rxr_ctx *ctx, uint64_t *out2);

/* tests: the device projection's two ticket words (rxr_project.h) after the context's streams have drained: out2[0] = k_proj_scan's
 * arrival counter (0 between frames: the workgroup that arrives last hands it back), out2[1] = "a triangle of the last device-projected
 * frame appends" (proj_init_item clears it, clip_count_item raises it: 0 lets k_proj_scan and k_clip_emit leave at once) */
int rxr_debug_projection_ticket(rxr_ctx *ctx, uint32_t *out2);

/* tests (host only, no device): the layout arithmetic of rxr_resize_meshes (rxr_mesh_resize.h, rxr_resize_bases) as the library
 * compiled it, over counts [n][2]: bases [n][4] = vin, tin, vout, tout base of every mesh, totals [4]; returns n, or the index of the
 * first mesh with which a total reaches 2^31 output slots */
uint32_t rxr_debug_resize_bases(const uint32_t *counts, uint32_t n, uint32_t *bases, uint64_t *totals);

/* tools/mesh_resize_bench.py: us2[0] = the stream time of the last accepted resize's k_mesh_repack, us2[1] = the time of one
 * device-to-device copy of *bytes (what that kernel wrote) between the two object blobs, after a warm-up copy */
int rxr_debug_resize_repack(rxr_ctx *ctx, float *us2, uint64_t *bytes);

/* tests / tools: the object-space pools the context holds, whole: totals[2] = vertices, triangles; each array (may be NULL) takes
 * min(total, capacity) items of vertices [4], uvs [2], indices [3], normals [3] */
int rxr_debug_object_pools(rxr_ctx *ctx, uint64_t *totals, float *vertices, float *uvs, uint32_t *indices, float *normals, uint64_t capacity_vertices,
                           uint64_t capacity_triangles);

/* tests: how the resident frame's 3D arrays arrived -- 0 plain rxr_upload_frame, 1 streamed and copied, 2 streamed out of page-locked
 * memory */
int rxr_debug_stream_info(rxr_ctx *ctx);

/* tests: how many launch sequences rxr_synchronize has rendered again after a list overflow (a plain context or a member) */
uint32_t rxr_debug_rerenders(rxr_ctx *ctx);

/* tests: the symbol name of the raster kernel of the context's most recent raster launch ("k_raster_rows_cut_rl", "k_raster_jit", ...;
 * "" when the last frame launched none); a multi-device handle answers for member 0 */
const char *rxr_debug_last_raster_kernel(rxr_ctx *ctx);

/* tests: what the context's most recent render did for the set-up records of a small frame: 0 nothing (no 3D pass, the fused
 * mode), 1 it read the records rxr_upload_frame made on the host, 2 it launched k_setup3d; a multi-device handle answers for member 0 */
uint32_t rxr_debug_last_setup_route(rxr_ctx *ctx);

/* tests: the resident host-projected frame's set-up records (n x 96 and n x 80 bytes, n = *n_tris <= capacity_tris) as k_setup3d writes them
 * for the whole-frame band -- into zeroed scratch: it leaves the records of a workgroup without a drawable triangle alone -- and, when the
 * frame carries them, as rxr_upload_frame made them on the host, read back from the frame blob.  Returns 1 with both pairs filled, 0 when
 * the frame has no host-made records (only the device's pair is filled), a negative status otherwise (all four pointers are required).
 * CLOBBERS the context's scratch records (zeroed, then whole-frame records): harmless, since every render that reads scratch launches
 * k_setup3d into it first. */
int rxr_debug_setup_records(rxr_ctx *ctx, void *host_setup, void *host_shade, void *dev_setup, void *dev_shade, uint32_t capacity_tris, uint32_t *n_tris);

/* what the run-time compiler did with the last program set of this context (rxr_jit.hip); "" when it was not asked */
const char *rxr_debug_jit_info(rxr_ctx *ctx);

/* device-free half of the run-time compiler, for tests without a GPU: validates + flattens the set like rxr_check_shaders, generates
 * the C++ of its programs (copied to `source`, truncated to its capacity) and, with compile != 0, runs hiprtc for gfx950.
 * Returns RXR_OK, the validation status, or RXR_ERR_UNSUPPORTED with the reason in `message` when the set is not covered. */
int rxr_debug_jit_generate(const rxr_shader_set *set, int compile, char *source, uint32_t source_capacity, char *message, uint32_t message_capacity);

/* ---- rxr_selftest.hip ---- */

/* tests: ONE public helper of rxr_exact_math.h on n operand tuples of the caller's choosing (host, n x 4 floats), every result handed
 * back as raw bits (host, n x 4 floats; unused operand and result slots are zero).  Tuple i is evaluated by lane i % 64 of wave i / 64
 * in workgroups of 256: the helpers vote per wave, so the caller decides which operands share a vote; the last wave may be partial.
 * Kinds, operands -> results:
 *    0 div1_known          (n, d)           -> q, with ok = in_window(n) && in_window(d)
 *    1 div1_static         (n, d)           -> q, with ok = true: only operands a call site claims statically
 *    2 div2                (n0, n1, d)      -> q0, q1
 *    3 div2_pre            (n0, n1, d)      -> q0, q1, with r = denominator_part(d) as the row-mode kernels compute it
 *    4 div3                (n0, n1, n2, d)  -> q0, q1, q2
 *    5 div3_self           (n0, n1, n2, d)  -> q0, q1, q2, qd
 *    6 normalize3          (x, y, z)        -> ox, oy, oz, magnitude
 *    7 normalize3_z        (x, y, z)        -> ox, oy, oz
 *    8 normalize3_relaxed  (x, y, z)        -> ox, oy, oz, magnitude
 *    9 sqrt_exact          (x)              -> root
 *   10 pow_exp2_log2       (x, k)           -> power
 *   11 sat_u32             (x)              -> the integer, as bits
 *   12 wave_max_nonneg     (v)              -> the wave's maximum, in every lane
 *   13 wave_inclusive_add  (integer bits)   -> the prefix sum, as bits
 * Stages through device memory on the context's stream and blocks.  RXR_ERR_INVALID (results untouched): a NULL pointer, n == 0, an
 * unknown kind, n % 64 != 0 for kinds 12 and 13 (every lane must be active).  A multi-device handle answers as member 0. */
int rxr_debug_exact_math(rxr_ctx *ctx, uint32_t kind, const float *operands, uint32_t n, float *results);

/* ---- rxr_kernels.hip ---- */

/* ONLY in a library built with -DRXR_PHASE_TIMING=1 (no ordinary build defines it, so the symbol is normally absent): the sums of
 * the raster kernel's 16 phase counters over its workgroups; reset != 0 clears them */
int rxr_debug_phase_read(unsigned long long *out16, int reset);

/* ---- rxr_jit.hip ---- */

/* tests (no device needed): the clean-up of stale job directories under `parent`, and where this process keeps its own */
void rxr_debug_jit_sweep(const char *parent);
/* the environment a background compiler would be started with, one "NAME=value" per line; returns the length needed */
int rxr_debug_jit_child_env(const char *tmpdir, char *out, uint32_t capacity);
int rxr_debug_jit_job_parent(char *out, uint32_t capacity);

/* rxr_jitc's half: generated source file -> code object file (no device needed) */
int rxr_debug_jit_compile_file(const char *src_path, const char *arch, int level, const char *out_path);

/* ---- rxr_bake.hip ---- */

/* tests: the kernel of the context's most recent bake launch -- 1 k_bake (per-lane stack depths), 2 k_bake_s (static depths), 0 when
 * the context has launched no bake; a multi-device handle answers for member 0 */
uint32_t rxr_debug_last_bake_kernel(rxr_ctx *ctx);

/* ---- rxr_terrain.hip ---- */

uint32_t rxr_debug_terrain_launches(rxr_ctx *ctx);

/* ---- rxr_terrain_hit.hip ---- */

/* test-only: the symbol name of the last call's march kernel ("" before any) and, in *launches, its launches */
const char *rxr_debug_terrain_hit_kernel(rxr_ctx *ctx, uint32_t *launches);
uint32_t rxr_debug_terrain_hit_few_rays(void);

/* ---- rxr_terrain_mesh.hip ---- */

/* test-only: the k_terrain_mesh launches of the last mesh call */
uint32_t rxr_debug_terrain_mesh_launches(rxr_ctx *ctx);

/* ---- rxr_terrain_flatten.hip ---- */

/* test-only: the k_terrain_flatten launches of the last flatten call */
uint32_t rxr_debug_terrain_flatten_launches(rxr_ctx *ctx);

/* ---- rxr_terrain_gen.hip ---- */

/* test-only: the launches of the last evaluation call */
uint32_t rxr_debug_terrain_gen_launches(rxr_ctx *ctx);

/* ---- rxr_terrain_excl.hip ---- */

/* test-only: the rounds (one classification and one tile emission launch each) of the last tile-mesh call */
uint32_t rxr_debug_terrain_tile_launches(rxr_ctx *ctx);

/* test-only: the rounds (one classification and one emission launch each) of the last mesh call */
uint32_t rxr_debug_terrain_excl_launches(rxr_ctx *ctx);

/* ---- rxr_chunk_tex.hip ---- */

/* tests: the kernel's constants (sources per launch, texels per segment, segments of one source in flight) and the
 * k_chunk_tex_commit launches of the last registration or update */
void rxr_debug_chunk_tex_constants(uint32_t out[3]);
uint32_t rxr_debug_chunk_tex_launches(rxr_ctx *ctx);

/* ---- rxr_normals.hip ---- */

/* test-only: the route of the last vertex-normals call (0: none yet) and, through `launches`, how many launches it made (small:
 * k_nrm_small launches; general: rounds of faces, sort and gather) */
uint32_t rxr_debug_vertex_normals(rxr_ctx *ctx, uint32_t *launches);

/* test-only: the small route's bound as compiled (the environment's override is not applied) and what an override is cut to */
void rxr_debug_vertex_normals_constants(uint32_t out[3]);

/* ---- rxr_ray_accel.hip ---- */

/* tests: the box tree as it stands after the context's streams have drained (no build, no refresh is started): *n_nodes = its nodes,
 * leaves first, and, where `nodes` is not NULL, min(*n_nodes, capacity) of them as eight floats each: lo[3], kappa, hi[3], maxabs.
 * *n_nodes = 0 when no tree stands. */
int rxr_debug_ray_accel_nodes(rxr_ctx *ctx, float *nodes, uint64_t capacity, uint64_t *n_nodes);

#ifdef __cplusplus
}
#endif

#endif /* RXR_DEBUG_H */
