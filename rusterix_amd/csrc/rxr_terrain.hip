// rxr_terrain.hip -- terrain chunk textures: Terrain::bake_chunk (src/terrain/mod.rs:318-369) with sample_source (:197-245) and
// sample_source_blended_radius (:247-298), the texture build_chunk_at (:372-399) stores in chunk.terrain_texture.  include/rxr.h:
// rxr_check_terrain, rxr_set_terrain, rxr_bake_terrain, rxr_bake_terrain_to.
//
// Semantics, per texel (x, y) of chunk (cx, cy) at `ppt` pixels per tile -- one f32 operation per reference operation, in its order,
// nothing fused (the build's -ffp-contract=off), so the bytes are the reference's:
//   tile = (cx * chunk_size) as f32 + (x as f32 / ppt as f32); world = tile * scale; blend mode of the cell at floor(tile) as i32.
//   sample_source(p): q = p / scale; cell = floor(q) as i32 (saturating); uv = q - trunc(q), + 1.0 when negative (can be exactly 1.0);
//     a cell with a texture: texel (round(u * (w - 1)), round(v * (h - 1))), round half away from zero, `as usize`, clamped; valid.
//     Else ((x & 1) ^ (y & 1)) == 0 ? 135 : 120 with alpha 255; not valid.
//   None: sample_source(world), alpha included.
//   Blend(r) / BlendOffset(r, off): p = world (+ off); step = min(scale) * 0.5; steps = ceil(r / step) as i32; for dy, for dx in
//     -steps..=steps: o = d as f32 * step; dist2 = ox * ox + oy * oy; skipped when dist2 > r * r; a valid tap adds pixel * weight per
//     channel and weight to weight_sum, weight = t * t, t = 1 - dist2 / (r * r).  weight_sum > 0: round(sum / weight_sum) as u8, alpha
//     255.  Else (no valid tap, or r == 0, whose one weight is 0 / 0): ((x ^ y) & 1) == 0 ? 120 : 135 at the cell of p.
//
// Kernel: a workgroup is ONE wave that owns an 8 x 8 block of texels inside one tile cell (ceil(ppt / 8)^2 blocks a cell; lanes past
// the cell's edge repeat its last column / row and store nothing).  One thread owns one texel and runs its taps in the reference's
// order: a texel's sum is never split.  The blend cell comes from floor(tile) in f32, which for large chunk coordinates is not the
// cell the block was cut from: the wave votes, and when every lane sees the same blend cell (the rule) mode, radius and offset are
// wave-uniform -- a None wave takes one sample per lane and leaves, a blended wave runs the SEPARABLE set-up:
//   * the tap position along x depends on (texel column, dx) alone, along y on (texel row, dy): for its 8 columns and 8 rows the wave
//     computes (p + d * step) / scale, floor, the grid column / row (-1 outside the grid) and uv once -- 16 * (2 * steps + 1) divisions
//     instead of 64 * 2 * (2 * steps + 1)^2 -- into LDS;
//   * the weight of a tap depends on (dx, dy, r, step) alone: rxr_set_terrain fills one table per radius in use (k_terrain_weights,
//     the same operations; -1 marks a skipped tap, a weight is never negative), read through wave-uniform addresses.
//   The inner loop is then two LDS reads, the cell's texture index, the texture record, two multiply-round-clamp, one texel and seven
//   multiply / adds: no division.  The operations on each value are the reference's, so the bits are.
// Otherwise (lanes disagree, or RXR_TERRAIN_NAIVE=1 in the environment, the A-B switch of tools/terrain_bench.py) every lane runs the
// plain transcription, every tap with its own divisions.
// A call is cut into launches of bounded work (texels x taps, estimated per cell from the host's copy of the blend words;
// RXR_TERRAIN_LAUNCH_TAPS overrides the bound) and of at most TERRAIN_LAUNCH_CHUNKS chunks, whose coordinates travel as kernel
// arguments: nothing a queued launch reads can change under it except the resident terrain, which rxr_set_terrain replaces only
// after rxr_quiesce.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "rxr_debug.h"
#include "rxr_query.h"
#include "rxr_exact_math.h"

#define TERRAIN_BLOCK 8u            // a wave's texel block is TERRAIN_BLOCK x TERRAIN_BLOCK
#define TERRAIN_LAUNCH_CHUNKS 64u   // chunk coordinates per launch (kernel arguments)
// 2^32 texel-taps a launch: at the 0.63 - 0.87 ps a tap of kernel time measured on one MI355X (profiles/terrain/README.md, from a
// kernel trace) a full launch runs 2.7 - 3.7 ms, and about twice that through the per-lane path.
// The work is an ESTIMATE: it takes each block's blend cell to be the cell the block was cut from, so where f32 rounding moves
// texels into a neighbouring cell (chunk coordinates beyond about 2^20 tiles) a launch can exceed the bound by the difference
// between the two cells' tap counts -- at most 16 641 taps a texel, the refusal's limit.
#define TERRAIN_DEFAULT_LAUNCH_TAPS (1ull << 32)

struct TerrainCell {   // one cell of the dense grid
    int32_t tex;       // index into TerrainTex, or -1
    uint32_t blend;    // kind | radius << 8
    float ox, oy;      // BlendOffset's offset
};
struct TerrainTex {
    uint32_t first, w, h;   // first: index of texel (0, 0) in the pool
    float wm1, hm1;         // w as f32 - 1.0, h as f32 - 1.0
    uint32_t pad[3];
};

struct TerrainArgs {
    const TerrainCell *cells;
    const TerrainTex *tex;
    const uint32_t *texels;    // packed r | g << 8 | b << 16 | a << 24
    const uint32_t *weights;   // [256] table offset (in words from here) by radius, 0: none; then the tables
    int32_t x0, y0;            // the grid's first cell
    uint32_t gw, gh;           // its size (0: no cells)
    float sx, sy;
    int32_t chunk_size, ppt;
    uint32_t side, bpc_x, bpc, blocks_per_chunk;   // blocks a cell along one axis, a cell, a chunk
    uint32_t first_block;      // of this launch, counted from the first block of coords[0]
    uint32_t max_steps, naive;
    uint32_t *out;             // texel (0, 0) of the bake of coords[0]
    int32_t coords[TERRAIN_LAUNCH_CHUNKS][2];
};

namespace {

__device__ __forceinline__ float fdiv(float n, float d) { return rxm::div1_known(n, d, rxm::in_window(n) && rxm::in_window(d)); }

// Rust's `x as i32`: saturating, NaN -> 0
__host__ __device__ __forceinline__ int32_t sat_i32(float x) {
    if (!(x >= -2147483648.0f)) return x != x ? 0 : INT32_MIN;
    if (x >= 2147483648.0f) return INT32_MAX;
    return (int32_t)x;
}

__device__ __forceinline__ uint32_t gray(uint32_t v) { return v | (v << 8) | (v << 16) | 0xFF000000u; }

// the cell of the dense grid at world tile (x, y), or null
__device__ __forceinline__ const TerrainCell *cell_at(const TerrainArgs &A, int32_t x, int32_t y) {
    const uint32_t gx = (uint32_t)x - (uint32_t)A.x0, gy = (uint32_t)y - (uint32_t)A.y0;
    return (gx < A.gw && gy < A.gh) ? A.cells + ((size_t)gy * A.gw + gx) : nullptr;
}

// Texture::sample_nearest (src/texture.rs:307-323)
__device__ __forceinline__ uint32_t texel_of(const TerrainArgs &A, int32_t tex, float u, float v) {
    const TerrainTex T = A.tex[tex];
    const uint32_t tx = min(rxm::sat_u32(roundf(u * T.wm1)), T.w - 1u), ty = min(rxm::sat_u32(roundf(v * T.hm1)), T.h - 1u);
    return A.texels[T.first + ty * T.w + tx];
}

// sample_source (:197-245): the pixel, and whether a texture gave it
__device__ __forceinline__ uint32_t sample_source(const TerrainArgs &A, float wx, float wy, bool &valid) {
    const float qx = fdiv(wx, A.sx), qy = fdiv(wy, A.sy);
    const int32_t x = sat_i32(floorf(qx)), y = sat_i32(floorf(qy));
    float u = qx - truncf(qx), v = qy - truncf(qy);
    if (u < 0.0f) u = u + 1.0f;
    if (v < 0.0f) v = v + 1.0f;
    const TerrainCell *c = cell_at(A, x, y);
    const int32_t tex = c ? c->tex : -1;
    valid = tex >= 0;
    if (valid) return texel_of(A, tex, u, v);
    return gray((((x & 1) ^ (y & 1)) == 0) ? 135u : 120u);
}

// the end of sample_source_blended_radius (:280-297)
__device__ __forceinline__ uint32_t blended_result(const TerrainArgs &A, float px, float py, float sr, float sg, float sb, float ws) {
    if (ws > 0.0f) {
        float r, g, b;
        rxm::div3(sr, sg, sb, ws, r, g, b);
        return min(rxm::sat_u32(roundf(r)), 255u) | (min(rxm::sat_u32(roundf(g)), 255u) << 8) | (min(rxm::sat_u32(roundf(b)), 255u) << 16) | 0xFF000000u;
    }
    const int32_t x = sat_i32(floorf(fdiv(px, A.sx))), y = sat_i32(floorf(fdiv(py, A.sy)));
    return gray((((x ^ y) & 1) == 0) ? 120u : 135u);
}

// sample_source_blended_radius (:247-298) as written: every tap with its own divisions
__device__ __forceinline__ uint32_t blended_naive(const TerrainArgs &A, float px, float py, float radius) {
    float sr = 0.0f, sg = 0.0f, sb = 0.0f, ws = 0.0f;
    const float step = fminf(A.sx, A.sy) * 0.5f;
    const float r2 = radius * radius;
    const int32_t steps = sat_i32(ceilf(fdiv(radius, step)));
    for (int32_t dy = -steps; dy <= steps; ++dy) {
        for (int32_t dx = -steps; dx <= steps; ++dx) {
            const float ox = (float)dx * step, oy = (float)dy * step;
            const float dist2 = ox * ox + oy * oy;
            if (dist2 > r2) continue;
            bool valid;
            const uint32_t p = sample_source(A, px + ox, py + oy, valid);
            if (valid) {
                const float t = 1.0f - fdiv(dist2, r2);
                const float w = t * t;
                sr = sr + (float)(p & 255u) * w;
                sg = sg + (float)((p >> 8) & 255u) * w;
                sb = sb + (float)((p >> 16) & 255u) * w;
                ws = ws + w;
            }
        }
    }
    return blended_result(A, px, py, sr, sg, sb, ws);
}

}  // namespace

// one table: the weight of tap (dx, dy) at [(dy + steps) * (2 * steps + 1) + dx + steps], -1.0 for a tap the reference skips
extern "C" __global__ __launch_bounds__(256) void k_terrain_weights(float *table, int32_t steps, float radius, float step) {
    const int32_t n = 2 * steps + 1;
    const int32_t i = (int32_t)(blockIdx.x * 256u + threadIdx.x);
    if (i >= n * n) return;
    const int32_t dy = i / n - steps, dx = i % n - steps;
    const float ox = (float)dx * step, oy = (float)dy * step;
    const float dist2 = ox * ox + oy * oy;
    const float r2 = radius * radius;
    if (dist2 > r2) {
        table[i] = -1.0f;
        return;
    }
    const float t = 1.0f - fdiv(dist2, r2);
    table[i] = t * t;
}

extern "C" __global__ __launch_bounds__(64) void k_terrain_bake(TerrainArgs A) {
    extern __shared__ uint2 tap_axis[];   // [x: 8 columns][n], then [y: 8 rows][n]: {grid column / row or -1, uv bits}
    const uint32_t gb = A.first_block + blockIdx.x;
    const uint32_t chunk = gb / A.blocks_per_chunk, in_chunk = gb - chunk * A.blocks_per_chunk;
    const uint32_t cell = in_chunk / A.bpc, sub = in_chunk - cell * A.bpc;
    const uint32_t cs = (uint32_t)A.chunk_size, ppt = (uint32_t)A.ppt;
    const uint32_t cell_y = cell / cs, cell_x = cell - cell_y * cs;
    const uint32_t by = sub / A.bpc_x, bx = sub - by * A.bpc_x;
    const uint32_t lx = threadIdx.x & 7u, ly = threadIdx.x >> 3;
    const uint32_t in_x = bx * TERRAIN_BLOCK + lx, in_y = by * TERRAIN_BLOCK + ly;
    const bool stores = in_x < ppt && in_y < ppt;
    const int32_t min_x = A.coords[chunk][0] * A.chunk_size, min_y = A.coords[chunk][1] * A.chunk_size;   // (checked on the host: no overflow)
    const float fppt = (float)A.ppt;
    // a lane past the cell's edge repeats the last column / row: the wave stays whole for the votes and the barrier
    const uint32_t x = cell_x * ppt + min(in_x, ppt - 1u), y = cell_y * ppt + min(in_y, ppt - 1u);
    const float tile_x = (float)min_x + fdiv((float)x, fppt), tile_y = (float)min_y + fdiv((float)y, fppt);
    const float world_x = tile_x * A.sx, world_y = tile_y * A.sy;
    const int32_t tpx = sat_i32(floorf(tile_x)), tpy = sat_i32(floorf(tile_y));
    const TerrainCell *bc = cell_at(A, tpx, tpy);
    const uint32_t blend = bc ? bc->blend : RXR_TERRAIN_BLEND_NONE;
    const uint32_t kind = blend & 255u;
    float px = world_x, py = world_y;
    if (kind == RXR_TERRAIN_BLEND_OFFSET) {
        px = world_x + bc->ox;
        py = world_y + bc->oy;
    }
    const float radius = (float)((blend >> 8) & 255u);
    const bool uniform = !A.naive && rxm::wave_all(tpx == __builtin_amdgcn_readfirstlane(tpx) && tpy == __builtin_amdgcn_readfirstlane(tpy));
    const float step = fminf(A.sx, A.sy) * 0.5f;
    const int32_t steps = kind == RXR_TERRAIN_BLEND_NONE ? 0 : sat_i32(ceilf(fdiv(radius, step)));
    uint32_t pixel;
    if (!uniform || (uint32_t)steps > A.max_steps) {
        bool valid;
        pixel = kind == RXR_TERRAIN_BLEND_NONE ? sample_source(A, world_x, world_y, valid) : blended_naive(A, px, py, radius);
    } else if (__builtin_amdgcn_readfirstlane(kind) == RXR_TERRAIN_BLEND_NONE) {
        bool valid;
        pixel = sample_source(A, world_x, world_y, valid);
    } else {
        // ---- the separable set-up: 8 columns and 8 rows times n tap offsets ----
        const uint32_t ukind = __builtin_amdgcn_readfirstlane(kind);
        const int32_t S = __builtin_amdgcn_readfirstlane(steps);
        const uint32_t n = 2u * (uint32_t)S + 1u;
        const float off_x = ukind == RXR_TERRAIN_BLEND_OFFSET ? bc->ox : 0.0f, off_y = ukind == RXR_TERRAIN_BLEND_OFFSET ? bc->oy : 0.0f;
        for (uint32_t i = threadIdx.x; i < 16u * n; i += 64u) {
            const uint32_t axis = i / (8u * n), r = i - axis * 8u * n;
            const uint32_t line = r / n;
            const int32_t d = (int32_t)(r - line * n) - S;
            const uint32_t in_c = (axis ? by : bx) * TERRAIN_BLOCK + line;
            const uint32_t t = (axis ? cell_y : cell_x) * ppt + min(in_c, ppt - 1u);
            const float scale = axis ? A.sy : A.sx;
            const float tile = (float)(axis ? min_y : min_x) + fdiv((float)t, fppt);
            float p = tile * scale;
            if (ukind == RXR_TERRAIN_BLEND_OFFSET) p = p + (axis ? off_y : off_x);
            const float sp = p + (float)d * step;
            const float q = fdiv(sp, scale);
            const int32_t c = sat_i32(floorf(q));
            float f = q - truncf(q);
            if (f < 0.0f) f = f + 1.0f;
            const uint32_t g = (uint32_t)c - (uint32_t)(axis ? A.y0 : A.x0);
            tap_axis[i] = make_uint2(g < (axis ? A.gh : A.gw) ? g : 0xFFFFFFFFu, __float_as_uint(f));
        }
        __syncthreads();
        const uint2 *tap_x = tap_axis + lx * n, *tap_y = tap_axis + 8u * n + ly * n;
        const uint32_t table = A.weights[__builtin_amdgcn_readfirstlane((blend >> 8) & 255u)];
        const float *weight = (const float *)A.weights + table;
        float sr = 0.0f, sg = 0.0f, sb = 0.0f, ws = 0.0f;
        for (uint32_t iy = 0; iy < n; ++iy) {
            const uint2 ey = tap_y[iy];
            const float v = __uint_as_float(ey.y);
            for (uint32_t ix = 0; ix < n; ++ix) {
                const float w = weight[iy * n + ix];
                if (w < 0.0f) continue;   // dist2 > radius^2 (wave-uniform)
                const uint2 ex = tap_x[ix];
                if ((int32_t)(ex.x | ey.x) < 0) continue;   // outside the grid: no source
                const int32_t tex = A.cells[(size_t)ey.x * A.gw + ex.x].tex;
                if (tex < 0) continue;
                const uint32_t p = texel_of(A, tex, __uint_as_float(ex.y), v);
                sr = sr + (float)(p & 255u) * w;
                sg = sg + (float)((p >> 8) & 255u) * w;
                sb = sb + (float)((p >> 16) & 255u) * w;
                ws = ws + w;
            }
        }
        pixel = blended_result(A, px, py, sr, sg, sb, ws);
    }
    if (stores) A.out[((size_t)chunk * A.side + (cell_y * ppt + in_y)) * A.side + (cell_x * ppt + in_x)] = pixel;
}

namespace {

struct TerrainShape {
    int32_t x0 = 0, y0 = 0;
    uint32_t gw = 0, gh = 0, max_steps = 0;
};

// `steps` of sample_source_blended_radius (:256-258)
int32_t steps_of(const float scale[2], uint32_t radius) {
    const float step = std::min(scale[0], scale[1]) * 0.5f;
    return sat_i32(std::ceil((float)radius / step));
}

// everything rxr_set_terrain refuses; fills `shape`
int check_terrain(const float *scale, int32_t chunk_size, const int32_t *cell_xy, const int32_t *cell_texture, const uint32_t *cell_blend,
                  const float *cell_offset, uint32_t n_cells, const rxr_texture *textures, uint32_t n_textures, TerrainShape &shape, std::string &err) {
    auto bad = [&](int st, const std::string &m) {
        err = m;
        return st;
    };
    if (!scale) return bad(RXR_ERR_INVALID, "NULL scale");
    if (!(std::isfinite(scale[0]) && std::isfinite(scale[1]) && scale[0] > 0.0f && scale[1] > 0.0f))
        return bad(RXR_ERR_INVALID, "scale must be finite and > 0 (the reference never leaves its tap loop at scale 0)");
    if (chunk_size < 1) return bad(RXR_ERR_INVALID, "chunk_size must be at least 1");
    if (n_cells && (!cell_xy || !cell_texture || !cell_blend)) return bad(RXR_ERR_INVALID, "NULL cell array");
    if (n_textures && !textures) return bad(RXR_ERR_INVALID, "NULL texture array");
    for (uint32_t t = 0; t < n_textures; ++t)
        if (!textures[t].rgba || !textures[t].width || !textures[t].height)
            return bad(RXR_ERR_INVALID, "textures[" + std::to_string(t) + "] is NULL or zero-sized");
    int64_t lo[2] = {INT32_MAX, INT32_MAX}, hi[2] = {INT32_MIN, INT32_MIN};
    for (uint32_t i = 0; i < n_cells; ++i) {
        const std::string at = "cell " + std::to_string(i) + " (" + std::to_string(cell_xy[2 * i]) + ", " + std::to_string(cell_xy[2 * i + 1]) + "): ";
        if (cell_texture[i] < -1 || cell_texture[i] >= (int64_t)n_textures) return bad(RXR_ERR_INVALID, at + "texture index " + std::to_string(cell_texture[i]) + " out of range");
        const uint32_t kind = cell_blend[i] & 255u;
        if (kind > RXR_TERRAIN_BLEND_OFFSET || (cell_blend[i] >> 16)) return bad(RXR_ERR_INVALID, at + "unknown blend kind (cell_blend " + std::to_string(cell_blend[i]) + ")");
        if (kind == RXR_TERRAIN_BLEND_OFFSET && cell_offset && !(std::isfinite(cell_offset[2 * i]) && std::isfinite(cell_offset[2 * i + 1])))
            return bad(RXR_ERR_INVALID, at + "the blend offset is not finite");
        for (int a = 0; a < 2; ++a) {
            lo[a] = std::min<int64_t>(lo[a], cell_xy[2 * i + a]);
            hi[a] = std::max<int64_t>(hi[a], cell_xy[2 * i + a]);
        }
    }
    shape = TerrainShape{};
    if (n_cells) {
        const int64_t w = hi[0] - lo[0] + 1, h = hi[1] - lo[1] + 1;
        if (w > RXR_TERRAIN_MAX_CELLS || h > RXR_TERRAIN_MAX_CELLS || w * h > RXR_TERRAIN_MAX_CELLS)
            return bad(RXR_ERR_INVALID, "the cells' bounding rectangle (" + std::to_string(w) + " x " + std::to_string(h) + ") holds more than RXR_TERRAIN_MAX_CELLS cells");
        shape.x0 = (int32_t)lo[0];
        shape.y0 = (int32_t)lo[1];
        shape.gw = (uint32_t)w;
        shape.gh = (uint32_t)h;
    }
    for (uint32_t i = 0; i < n_cells; ++i) {
        if ((cell_blend[i] & 255u) == RXR_TERRAIN_BLEND_NONE) continue;
        const int32_t steps = steps_of(scale, (cell_blend[i] >> 8) & 255u);
        if (steps > (int32_t)RXR_TERRAIN_MAX_STEPS)
            return bad(RXR_ERR_UNSUPPORTED, "cell " + std::to_string(i) + ": radius " + std::to_string((cell_blend[i] >> 8) & 255u) + " takes " + std::to_string(steps) +
                                                " steps of min(scale) * 0.5, more than RXR_TERRAIN_MAX_STEPS (" + std::to_string(RXR_TERRAIN_MAX_STEPS) +
                                                "): bake this terrain on the host");
        shape.max_steps = std::max(shape.max_steps, (uint32_t)steps);
    }
    return RXR_OK;
}

// the argument checks both bake entry points share; `who` starts the message
int bake_check(rxr_ctx *ctx, const char *who, const int32_t *coords, uint32_t n, int32_t ppt) {
    const std::string w = who;
    if (!ctx->terrain_set) return rxr_fail(ctx, RXR_ERR_INVALID, w + ": no terrain is resident (rxr_set_terrain)");
    if (n && !coords) return rxr_fail(ctx, RXR_ERR_INVALID, w + ": NULL chunk_coords");
    if (ppt < 1) return rxr_fail(ctx, RXR_ERR_INVALID, w + ": pixels_per_tile must be at least 1");
    const uint64_t side = (uint64_t)ctx->terrain_chunk_size * (uint64_t)ppt;
    if (side > RXR_BAKE_MAX_DIM) return rxr_fail(ctx, RXR_ERR_INVALID, w + ": chunk_size * pixels_per_tile = " + std::to_string(side) + " exceeds RXR_BAKE_MAX_DIM");
    if ((uint64_t)n * side * side > RXR_BAKE_MAX_TEXELS) return rxr_fail(ctx, RXR_ERR_INVALID, w + ": more than " + std::to_string(RXR_BAKE_MAX_TEXELS) + " texels in one call");
    for (uint32_t i = 0; i < n; ++i)
        for (int a = 0; a < 2; ++a) {
            const int64_t m = (int64_t)coords[2 * i + a] * ctx->terrain_chunk_size;
            // (+ chunk_size stays inside i32 too: the host's per-cell lookups below add cell indices to it)
            if (m < INT32_MIN || m + ctx->terrain_chunk_size > INT32_MAX)
                return rxr_fail(ctx, RXR_ERR_INVALID, w + ": chunk_coords[" + std::to_string(i) + "] * chunk_size leaves i32 (the reference overflows)");
        }
    return RXR_OK;
}

// the whole bake into device memory, queued on `s`
int bake_run(rxr_ctx *ctx, const int32_t *coords, uint32_t n, int32_t ppt, uint8_t *dev_rgba, hipStream_t s) {
    uint64_t bound = TERRAIN_DEFAULT_LAUNCH_TAPS;
    if (const char *e = getenv("RXR_TERRAIN_LAUNCH_TAPS")) {
        const unsigned long long v = strtoull(e, nullptr, 10);
        if (v) bound = v;
    }
    const char *naive = getenv("RXR_TERRAIN_NAIVE");
    const uint32_t cs = (uint32_t)ctx->terrain_chunk_size, side = cs * (uint32_t)ppt;
    TerrainArgs A{};
    A.cells = (const TerrainCell *)ctx->d_terrain_cells.p;
    A.tex = (const TerrainTex *)ctx->d_terrain_tex.p;
    A.texels = (const uint32_t *)ctx->d_terrain_texels.p;
    A.weights = (const uint32_t *)ctx->d_terrain_weights.p;
    A.x0 = ctx->terrain_x0;
    A.y0 = ctx->terrain_y0;
    A.gw = ctx->terrain_gw;
    A.gh = ctx->terrain_gh;
    A.sx = ctx->terrain_scale[0];
    A.sy = ctx->terrain_scale[1];
    A.chunk_size = ctx->terrain_chunk_size;
    A.ppt = ppt;
    A.side = side;
    A.bpc_x = ((uint32_t)ppt + TERRAIN_BLOCK - 1u) / TERRAIN_BLOCK;
    A.bpc = A.bpc_x * A.bpc_x;
    A.blocks_per_chunk = cs * cs * A.bpc;   // (<= side * side <= 2^28)
    A.max_steps = ctx->terrain_max_steps;
    A.naive = naive && naive[0] == '1';
    const size_t lds = (size_t)16 * (2 * A.max_steps + 1) * sizeof(uint2);
    bool any_blend = false;
    for (uint32_t b : ctx->terrain_blend) any_blend |= (b & 255u) != RXR_TERRAIN_BLEND_NONE;
    // taps per texel of cell `cell` of chunk c, as the kernel will count them when the blend cell is the cell the block was cut from
    auto taps_of = [&](const int32_t *c, uint32_t cell) -> uint64_t {
        if (!any_blend) return 1;
        const int64_t x = (int64_t)c[0] * ctx->terrain_chunk_size + cell % cs - ctx->terrain_x0, y = (int64_t)c[1] * ctx->terrain_chunk_size + cell / cs - ctx->terrain_y0;
        if (x < 0 || y < 0 || x >= ctx->terrain_gw || y >= ctx->terrain_gh) return 1;
        const uint32_t b = ctx->terrain_blend[(size_t)y * ctx->terrain_gw + x];
        if ((b & 255u) == RXR_TERRAIN_BLEND_NONE) return 1;
        const uint64_t nn = 2ull * (uint64_t)steps_of(ctx->terrain_scale, (b >> 8) & 255u) + 1ull;
        return nn * nn;
    };
    const int rc = rxr_query_begin(ctx, ctx->lane[Q_TERRAIN], s);
    if (rc != RXR_OK) return rc;
    ctx->terrain_launches = 0;
    for (uint32_t c0 = 0; c0 < n; c0 += TERRAIN_LAUNCH_CHUNKS) {
        const uint32_t nc = std::min(n - c0, TERRAIN_LAUNCH_CHUNKS);
        memcpy(A.coords, coords + 2 * (size_t)c0, (size_t)nc * 2 * sizeof(int32_t));
        A.out = (uint32_t *)dev_rgba + (size_t)c0 * side * side;
        const uint32_t total = nc * A.blocks_per_chunk;
        uint32_t b = 0;
        while (b < total) {
            const uint32_t start = b;
            uint64_t budget = bound;
            while (b < total) {
                const uint32_t chunk = b / A.blocks_per_chunk, in_chunk = b - chunk * A.blocks_per_chunk;
                const uint64_t cost = 64ull * taps_of(A.coords[chunk], in_chunk / A.bpc);
                const uint32_t left = A.bpc - in_chunk % A.bpc;
                uint32_t k = (uint32_t)std::min<uint64_t>(left, budget / cost);
                if (!k) {
                    if (b != start) break;
                    k = 1;   // (a launch takes at least one block)
                }
                b += k;
                budget -= std::min(budget, k * cost);
                if (k < left) break;
            }
            A.first_block = start;
            hipLaunchKernelGGL(k_terrain_bake, dim3(b - start), dim3(64), lds, s, A);
            HIPCHK(ctx, hipGetLastError());
            ++ctx->terrain_launches;
        }
    }
    return rxr_query_end(ctx, ctx->lane[Q_TERRAIN], s);
}

}  // namespace

extern "C" {

int rxr_check_terrain(const float scale[2], int32_t chunk_size, const int32_t *cell_xy, const int32_t *cell_texture, const uint32_t *cell_blend,
                      const float *cell_offset, uint32_t n_cells, const rxr_texture *textures, uint32_t n_textures, char *message,
                      uint32_t message_capacity) {
    TerrainShape shape;
    std::string err;
    const int rc = check_terrain(scale, chunk_size, cell_xy, cell_texture, cell_blend, cell_offset, n_cells, textures, n_textures, shape, err);
    rxr_copy_message(err, message, message_capacity);
    return rc;
}

int rxr_set_terrain(rxr_ctx *ctx, const float scale[2], int32_t chunk_size, const int32_t *cell_xy, const int32_t *cell_texture,
                    const uint32_t *cell_blend, const float *cell_offset, uint32_t n_cells, const rxr_texture *textures, uint32_t n_textures) {
    if (!ctx) return RXR_ERR_INVALID;
    if (ctx->group)
        return rxr_as_member0(ctx, [&](rxr_ctx *m) { return rxr_set_terrain(m, scale, chunk_size, cell_xy, cell_texture, cell_blend, cell_offset, n_cells, textures, n_textures); });
    TerrainShape shape;
    std::string err;
    int rc = check_terrain(scale, chunk_size, cell_xy, cell_texture, cell_blend, cell_offset, n_cells, textures, n_textures, shape, err);
    if (rc != RXR_OK) return rxr_fail(ctx, rc, "rxr_set_terrain: " + err);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if ((rc = rxr_quiesce(ctx)) != RXR_OK) return rc;   // queued bakes read what is replaced here
    ctx->terrain_set = false;
    // the dense grid; a coordinate given twice: the later entry wins
    const size_t n_grid = (size_t)shape.gw * shape.gh;
    std::vector<TerrainCell> grid(n_grid, TerrainCell{-1, RXR_TERRAIN_BLEND_NONE, 0.0f, 0.0f});
    bool radius_used[256] = {};
    for (uint32_t i = 0; i < n_cells; ++i) {
        TerrainCell &c = grid[(size_t)((int64_t)cell_xy[2 * i + 1] - shape.y0) * shape.gw + (size_t)((int64_t)cell_xy[2 * i] - shape.x0)];
        c.tex = cell_texture[i];
        c.blend = cell_blend[i];
        const bool off = (cell_blend[i] & 255u) == RXR_TERRAIN_BLEND_OFFSET && cell_offset;
        c.ox = off ? cell_offset[2 * i] : 0.0f;
        c.oy = off ? cell_offset[2 * i + 1] : 0.0f;
    }
    ctx->terrain_blend.resize(n_grid);
    for (size_t i = 0; i < n_grid; ++i) {
        ctx->terrain_blend[i] = grid[i].blend;
        if ((grid[i].blend & 255u) != RXR_TERRAIN_BLEND_NONE) radius_used[(grid[i].blend >> 8) & 255u] = true;
    }
    // the textures: records and one pool of packed texels
    std::vector<TerrainTex> tex(n_textures);
    size_t n_texels = 0;
    for (uint32_t t = 0; t < n_textures; ++t) {
        if (n_texels + (size_t)textures[t].width * textures[t].height > 0xFFFFFFFFull) return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_set_terrain: more than 2^32 source texels");
        tex[t] = TerrainTex{(uint32_t)n_texels, textures[t].width, textures[t].height, (float)textures[t].width - 1.0f, (float)textures[t].height - 1.0f, {0, 0, 0}};
        n_texels += (size_t)textures[t].width * textures[t].height;
    }
    std::vector<uint32_t> texels(n_texels);
    for (uint32_t t = 0; t < n_textures; ++t) memcpy(texels.data() + tex[t].first, textures[t].rgba, (size_t)tex[t].w * tex[t].h * 4);
    // the weight tables: offsets by radius, then the tables
    std::vector<uint32_t> head(256, 0u);
    size_t words = 256;
    for (uint32_t r = 0; r < 256; ++r)
        if (radius_used[r]) {
            const size_t nn = 2 * (size_t)steps_of(scale, r) + 1;
            head[r] = (uint32_t)words;
            words += nn * nn;
        }
    hipStream_t s = ctx->stream;
    if ((rc = rxr_ensure(ctx, ctx->d_terrain_cells, std::max<size_t>(n_grid * sizeof(TerrainCell), 256))) != RXR_OK) return rc;
    if ((rc = rxr_ensure(ctx, ctx->d_terrain_tex, std::max<size_t>(tex.size() * sizeof(TerrainTex), 256))) != RXR_OK) return rc;
    if ((rc = rxr_ensure(ctx, ctx->d_terrain_texels, std::max<size_t>(n_texels * 4, 256))) != RXR_OK) return rc;
    if ((rc = rxr_ensure(ctx, ctx->d_terrain_weights, words * 4)) != RXR_OK) return rc;
    if (n_grid) HIPCHK(ctx, hipMemcpyAsync(ctx->d_terrain_cells.p, grid.data(), n_grid * sizeof(TerrainCell), hipMemcpyHostToDevice, s));
    if (!tex.empty()) HIPCHK(ctx, hipMemcpyAsync(ctx->d_terrain_tex.p, tex.data(), tex.size() * sizeof(TerrainTex), hipMemcpyHostToDevice, s));
    if (n_texels) HIPCHK(ctx, hipMemcpyAsync(ctx->d_terrain_texels.p, texels.data(), n_texels * 4, hipMemcpyHostToDevice, s));
    HIPCHK(ctx, hipMemcpyAsync(ctx->d_terrain_weights.p, head.data(), 256 * 4, hipMemcpyHostToDevice, s));
    const float step = std::min(scale[0], scale[1]) * 0.5f;
    for (uint32_t r = 0; r < 256; ++r)
        if (radius_used[r]) {
            const int32_t steps = steps_of(scale, r);
            const uint32_t nn = (uint32_t)(2 * steps + 1) * (uint32_t)(2 * steps + 1);
            hipLaunchKernelGGL(k_terrain_weights, dim3((nn + 255u) / 256u), dim3(256), 0, s, (float *)ctx->d_terrain_weights.p + head[r], steps, (float)r, step);
            HIPCHK(ctx, hipGetLastError());
        }
    HIPCHK(ctx, hipStreamSynchronize(s));   // (the host vectors above are read until here)
    ctx->terrain_scale[0] = scale[0];
    ctx->terrain_scale[1] = scale[1];
    ctx->terrain_chunk_size = chunk_size;
    ctx->terrain_x0 = shape.x0;
    ctx->terrain_y0 = shape.y0;
    ctx->terrain_gw = shape.gw;
    ctx->terrain_gh = shape.gh;
    ctx->terrain_max_steps = shape.max_steps;
    ctx->terrain_set = true;
    return RXR_OK;
}

int rxr_bake_terrain(rxr_ctx *ctx, const int32_t *chunk_coords, uint32_t n, int32_t pixels_per_tile, uint8_t *rgba) {
    if (!ctx) return RXR_ERR_INVALID;
    if (ctx->group) return rxr_as_member0(ctx, [&](rxr_ctx *m) { return rxr_bake_terrain(m, chunk_coords, n, pixels_per_tile, rgba); });
    int rc = bake_check(ctx, "rxr_bake_terrain", chunk_coords, n, pixels_per_tile);
    if (rc != RXR_OK) return rc;
    if (!n) return RXR_OK;
    if (!rgba) return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_bake_terrain: NULL rgba");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t side = (size_t)ctx->terrain_chunk_size * (size_t)pixels_per_tile;
    QueryIO io{ctx, ctx->lane[Q_TERRAIN]};
    const unsigned i_rgba = io.out(rgba, (size_t)n * side * side * 4);
    if ((rc = io.upload()) != RXR_OK) return rc;
    if ((rc = bake_run(ctx, chunk_coords, n, pixels_per_tile, io.dev<uint8_t>(i_rgba), ctx->stream)) != RXR_OK) return rc;
    return io.download();
}

int rxr_bake_terrain_to(rxr_ctx *ctx, const int32_t *chunk_coords, uint32_t n, int32_t pixels_per_tile, uint8_t *dev_rgba, void *hip_stream) {
    if (!ctx) return RXR_ERR_INVALID;
    if (ctx->group) return rxr_fail(ctx, RXR_ERR_UNSUPPORTED, "rxr_bake_terrain_to on a multi-device context: device pointers and streams belong to ONE device (use rxr_member)");
    int rc = bake_check(ctx, "rxr_bake_terrain_to", chunk_coords, n, pixels_per_tile);
    if (rc != RXR_OK) return rc;
    if (!n) return RXR_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t side = (size_t)ctx->terrain_chunk_size * (size_t)pixels_per_tile, bytes = (size_t)n * side * side * 4;
    if (!dev_rgba || ((uintptr_t)dev_rgba & 3u)) return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_bake_terrain_to: dev_rgba must be 4-byte aligned device memory");
    if (!rxr_on_device(ctx, dev_rgba, bytes)) return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_bake_terrain_to: dev_rgba is not device memory of the context's device (or is too small)");
    return bake_run(ctx, chunk_coords, n, pixels_per_tile, dev_rgba, hip_stream ? (hipStream_t)hip_stream : ctx->stream);
}

uint32_t rxr_debug_terrain_launches(rxr_ctx *ctx) {
    if (!ctx) return 0;
    if (ctx->group) return rxr_debug_terrain_launches(rxr_member(ctx, 0));
    return ctx->terrain_launches;
}

}  // extern "C"
