// rxr_render.hip -- the render half of the C ABI (include/rxr.h; host side, compiled by hipcc): the launch sequence of one render
// (render_impl, a list of named phases), the rxr_render_* entry points over it, kernel profiling, rxr_synchronize with its repairs, and
// the download, whose rectangle geometry lives in rxr_download_plan.h.  No kernel is defined here and there is no CPU fallback.
// Compiled as the tail of rxr_api.hip's translation unit (included there, not a source of the build); it includes what it uses itself.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <thread>
#include <vector>

#include "rxr_ctx.h"
#include "rxr_download_plan.h"

// (rxr_launch_setup: declared in rxr_api.hip, above in this translation unit)
extern "C" void rxr_launch_project(const ProjectParams *P, hipStream_t s);
extern "C" void rxr_launch_project2d(const Project2DParams *P, hipStream_t s);
extern "C" void rxr_launch_scan(const ScanArgs *A, hipStream_t s);
extern "C" void rxr_launch_bin2d_count(const RasterParams *P, hipStream_t s);
extern "C" void rxr_launch_bin2d_fill(const RasterParams *P, hipStream_t s);
extern "C" void rxr_launch_fill(const RasterParams *P, hipStream_t s);
extern "C" void rxr_launch_blockscan(const RasterParams *P, hipStream_t s);
extern "C" void rxr_launch_blockscan2d(const RasterParams *P, hipStream_t s);
extern "C" void rxr_launch_fill_words(uint32_t *dst, uint64_t n_words, uint32_t value, hipStream_t s);
extern "C" void rxr_launch_fill_outside_spans(const RasterParams *P, hipStream_t s);
extern "C" void rxr_launch_spans_from_meshes(const RasterParams *P, uint32_t n_tile_rows, const uint32_t *d2_box, uint2 *host_copy, hipStream_t s);
extern "C" const char *rxr_launch_raster_grid(const RasterParams *P, uint32_t grid_x, hipStream_t s);
extern "C" int rxr_raster_takes_spans(const RasterParams *P);

// the rows [c0, c1) of a contiguous band spec that the resident frame can draw in, rounded out to tile rows (false: not known -- all of them)
static bool content_band(const rxr_ctx *ctx, const RenderSpec &spec, uint32_t &c0, uint32_t &c1) {
    c0 = spec.row0;
    c1 = spec.row1;
    if (!(ctx->content_known && spec.tile_stride == 1u && !spec.compact && spec.row0 < spec.row1)) return false;
    c0 = std::min(std::max(ctx->content_row0 / RXR_TILE_H * RXR_TILE_H, spec.row0), spec.row1);
    c1 = std::max(std::min((ctx->content_row1 + RXR_TILE_H - 1u) / RXR_TILE_H * RXR_TILE_H, spec.row1), c0);
    // (an empty tile costs the raster launch about half a nanosecond of the chip's time, a fill launch two to three microseconds: the teapot
    // at 1080p lost 5 us of set-up to save 3 of raster.  Fewer than content_min_tiles() empty tiles: the whole band is rastered)
    const size_t saved_tiles = (size_t)((c0 - spec.row0) + (spec.row1 - c1)) / RXR_TILE_H * ctx->P.tiles_x;
    if (saved_tiles < content_min_tiles()) {
        c0 = spec.row0;
        c1 = spec.row1;
        return false;
    }
    return true;
}

// k_scan's arguments for the 3D bins of a launch, or (d2) for its 2D bins: the same fields with and without the 2d suffix
static ScanArgs scan_args(const RasterParams &P, bool d2) {
    const uint32_t n = P.tiles_x * P.tiles_y;
    if (d2) return {n, P.list2d_capacity, P.bin2d_count, P.bin2d_offset, P.bin2d_cursor, P.chunk2d_tot, P.chunk2d_base, P.counters2d, P.counters2d_next, P.host_status2d};
    return {n, P.list_capacity, P.bin_count, P.bin_offset, P.bin_cursor, P.chunk_tot, P.chunk_base, P.counters, P.counters_next, P.host_status};
}

namespace {

// A render in bands (contiguous band specs only): ONE pre-pass over the spec's rows, then the raster kernel in n_bands launches over
// consecutive groups of tile rows, events[k] recorded behind band k -- the caller ships finished rows while the next ones render
// (rxr_render_download).  The bins are those of the one pre-pass (RasterParams.bin_row0); every bin is still handed back zeroed by its
// own tile's workgroup; the frame is byte-identical to one launch (tests/test_gpu_parity.py).
struct RenderBands {
    uint32_t n_bands;
    hipEvent_t *events;      // [n_bands]
    uint32_t *row_of;        // [n_bands + 1], out: band k covers the rows [row_of[k], row_of[k + 1])
    hipEvent_t spans_event;  // device-projected sparse frames: recorded behind k_spans_from_meshes, which then also writes the completed
    bool spans_recorded;     // row-span table to the second half of ctx->h_row_spans; out: whether that happened in this call
};

// What one launch sequence knows.  Its phases are the member functions, in the order render_impl runs them; those that can fail return an
// rxr_status; each leaves what the later ones need in here.
struct Render {
    rxr_ctx *const ctx;
    const RenderSpec &spec;
    void *const dev_pixels;
    const hipStream_t s;
    const bool retry;               // rxr_synchronize renders the last launch again
    RenderBands *const bands;       // null: one raster launch
    RasterParams P = ctx->P;        // the working copy (clamp_to_content)
    ProfSlot *slot = nullptr;       // (take_profile_slot)
    uint32_t fill_a0 = 0, fill_a1 = 0, fill_b0 = 0, fill_b1 = 0;  // rows [a0, a1) above and [b0, b1) below the content
    bool use_spans = false;         // the raster kernel looks the row-span table up
    bool d3 = false;                // (small_frame_records)
    bool prepass = false, blockscan = false, dev_spans = false, project2d = false, projected2d = false;  // (prepass3d)
    bool prepass2d_ran = false;

    size_t n_bins() const { return (size_t)P.tiles_x * P.tiles_y; }
    uint32_t widest_span(uint32_t first_row, uint32_t n_rows) const {
        uint32_t w = 1u;
        for (uint32_t r = first_row; r < first_row + n_rows && r < RXR_MAX_TILE_ROWS; ++r) w = std::max(w, ctx->h_row_spans[r].y - ctx->h_row_spans[r].x);
        return w;
    }
    const char *launch_raster() { return rxr_launch_raster_grid(&P, use_spans ? widest_span(P.tile_y0, P.tiles_y) : 0u, s); }

    // every launch sequence uses the context's one set of scratch buffers (records, bins, counters): a render on another
    // stream than the previous one is ordered behind it
    // (the event is recorded here, at the switch, on the PREVIOUS stream -- it then covers that stream's renders and whatever the
    // caller queued behind them, a superset -- and not behind every launch sequence: an event record is a barrier packet that idles
    // the GPU for microseconds, and a caller that stays on one stream never needs it)
    int order_streams() {
        if (ctx->rendered && ctx->last_stream != s) {
            HIPCHK(ctx, hipEventRecord(ctx->ev_render, ctx->last_stream));
            HIPCHK(ctx, hipStreamWaitEvent(s, ctx->ev_render, 0));
        }
        if (retry) ctx->rerenders++;
        if (!ctx->upload_ordered_on || ctx->upload_ordered_on != s) {
            if (s != ctx->stream) {
                // the upload ran on the context stream: order the external stream behind it (once per upload)
                HIPCHK(ctx, hipEventRecord(ctx->ev_upload, ctx->stream));
                HIPCHK(ctx, hipStreamWaitEvent(s, ctx->ev_upload, 0));
            }
            ctx->upload_ordered_on = s;
        }
        return RXR_OK;
    }

    // Rows that nothing of the frame can reach (ctx->content_row0 / 1) take the miss colour from a fill at memory speed; the pre-pass and
    // the raster kernel are launched over the tile rows in between only.  A sparse frame pays for its empty tiles otherwise: a workgroup
    // each that fetches its bin's length to learn that there is nothing to do -- on the 1 M-triangle grid (the 84 tile rows above the grid
    // are empty) 0.575 -> 0.531 ms for the band alone (tools/band_probe.py, profiles/r04).  Contiguous bands only (not the stripe
    // launches of a multi-GPU share).
    void clamp_to_content() {
        P.row0 = spec.row0;
        P.row1 = spec.row1;
        P.tile_y0 = spec.tile_y0;
        P.tile_stride = spec.tile_stride;
        P.tiles_y = spec.tiles_y;
        P.compact = spec.compact ? 1u : 0u;
        P.out = (uint32_t *)dev_pixels;
        P.out_row_stride = P.width;
        P.out_base_row = (spec.external && !spec.compact) ? (int64_t)spec.row0 : 0;
        uint32_t c0 = 0, c1 = 0;
        if (content_band(ctx, spec, c0, c1)) {
            fill_a0 = spec.row0; fill_a1 = c0; fill_b0 = c1; fill_b1 = spec.row1;
            P.row0 = c0;
            P.row1 = c1;
            P.tile_y0 = c0 / RXR_TILE_H;
            P.tiles_y = c1 > c0 ? (c1 + RXR_TILE_H - 1u) / RXR_TILE_H - P.tile_y0 : 0u;
        }
        P.row_spans = nullptr;
        use_spans = ctx->spans_active && fill_a0 < fill_b1 /* (the clamp above applied) */ && P.tiles_y;
    }

    // Kernel timing is opt-in (rxr_profile_begin): per-dispatch start / stop events (rxr_launch.h), no event record on the stream.
    // Without it rxr_stats' *_us fields stay zero.
    void take_profile_slot() {
        const bool timed = !retry && !ctx->prof.empty() && (ctx->prof_calls++ % ctx->prof_stride) == 0u;  // (a re-render after a list overflow takes no profiling slot)
        if (timed) {
            slot = &ctx->prof[ctx->prof_next % ctx->prof.size()];
            slot->n = 0;
            slot->raster_first = RXR_PROF_MAX_KERNELS;
            ctx->prof_next++;
        }
        ctx->last_prof = slot;
    }

    // small scenes: one staging round of k_raster holds every triangle -> no set-up / binning launches at all
    void small_frame_records() {
        d3 = P.tiles_y && (P.flags & RXR_FLAG_D3_ACTIVE);
        P.fused_small = (d3 && P.n_tris3d <= RXR_STAGE_TRIS) ? ctx->small_mode : 0u;
        if (P.kernel_level != KL_COMMON && P.fused_small == 1u) P.fused_small = 2u;  // k_raster_vm reads the records k_setup3d writes
        ctx->last_setup_route = 0u;
        if (d3 && P.fused_small) {
            if (ctx->frame_uses_meshes) rxr_launch_project(&ctx->PP, s);
            // The frame's own records, made by rxr_upload_frame for the band [0, height), serve every render whose band starts on a tile row
            // and ends on one or at the frame's height: the only words of a record that depend on the band are its pixel box's min_y / max_y,
            // and whatever reads them (visit, the tile reject and covers_plainly of scan_implicit) compares them with rows of launched tiles or
            // of pixels inside the band -- with the same answer under the whole-frame clamp.  Under any other band a tile's set of active lanes,
            // and with it the wave votes of the relaxed paths, would differ: such a render keeps the launch with its own clamp.
            const bool band_on_tiles = P.row0 % RXR_TILE_H == 0u && (P.row1 % RXR_TILE_H == 0u || P.row1 == P.height);
            if (P.fused_small == 2u && ctx->host_records && band_on_tiles) {
                P.tri_setup = (TriSetup *)((uint8_t *)ctx->d_frame.p + ctx->off_host_setup);  // (read only: no launch of this render writes records)
                P.tri_shade = (TriShade *)((uint8_t *)ctx->d_frame.p + ctx->off_host_shade);
                ctx->last_setup_route = 1u;
            } else if (P.fused_small == 2u) {
                rxr_launch_setup(&P, s);  // records only; no counters, bins or lists are touched
                ctx->last_setup_route = 2u;
            }
        }
        use_spans = use_spans && rxr_raster_takes_spans(&P) != 0;  // (the kernel this launch gets must be one that looks the table up)
    }

    void fill_outside_content() {
        if (use_spans) {
            // the pixels to the left and right of each tile row's span, and -- in the same launch: their spans are empty -- the rows above
            // and below the content (one launch of 13 us where two fills of whole rows and one of row ends took 16 and two more gaps)
            P.row_spans = (const uint2 *)ctx->d_row_spans.p;
            RasterParams Pf = P;
            Pf.row0 = spec.row0;
            Pf.row1 = spec.row1;
            Pf.tile_y0 = spec.tile_y0;
            Pf.tiles_y = spec.tiles_y;
            rxr_launch_fill_outside_spans(&Pf, s);
            return;
        }
        for (int part = 0; part < 2; ++part) {  // the rows outside the content: the 3D miss colour [0, 0, 0, 255] (:420-461)
            const uint32_t a = part ? fill_b0 : fill_a0, b = part ? fill_b1 : fill_a1;
            if (a < b) rxr_launch_fill_words(P.out + (size_t)((int64_t)a - P.out_base_row) * P.out_row_stride, (uint64_t)(b - a) * P.out_row_stride, 0xFF000000u, s);
        }
    }

    void project_meshes() {
        rxr_launch_project(&ctx->PP, s);  // clip_and_project + Edges + boxes on the device
        if (!dev_spans) return;
        if (project2d) {  // (its union box belongs to the table)
            rxr_launch_project2d(&ctx->PP2, s);
            projected2d = true;
        }
        const hipEvent_t spans_event = bands ? bands->spans_event : nullptr;
        P.row_spans = (const uint2 *)ctx->d_row_spans.p;
        rxr_launch_spans_from_meshes(&P, (P.height + RXR_TILE_H - 1u) / RXR_TILE_H, project2d ? ctx->PP2.d2_box : nullptr,
                                     spans_event ? ctx->h_row_spans + RXR_MAX_TILE_ROWS : nullptr, s);
        if (spans_event && hipEventRecord(spans_event, s) == hipSuccess) bands->spans_recorded = true;
        rxr_launch_fill_outside_spans(&P, s);
    }

    // The 3D pre-pass.  Mid-sized scenes: k_setup3d (records and boxes only) + k_blockscan; the counters are not touched (the clean set
    // stays clean, the large list stays empty: every block of bins looks at every triangle) -- the scatter form counts its wide groups in
    // the clean counter set and clears the other one, as k_scan does.  Otherwise k_setup3d, k_scan, k_fill: counter set `parity` is clean
    // (cleared by the previous launch's k_scan); this launch's k_scan clears the other set.  bin_count is clean because k_raster hands
    // every bin back zeroed -- under row spans every bin that a triangle is counted into lies inside its row's span (make_setup clips the
    // pixel boxes to the batch's reference tiles, from which the spans are made), so its workgroup runs and hands it back too.
    // (the pinned status words are never written by the host while launches may be in flight: earlier queued k_scan
    // launches write them; rxr_synchronize clears them once the streams have drained)
    int prepass3d() {
        prepass = d3 && !P.fused_small;
        // (device-projected frames: the spans are completed on the device, behind the projection -- see rxr_upload_frame)
        dev_spans = prepass && ctx->dev_spans && ctx->frame_uses_meshes && spec.tile_stride == 1u && !spec.compact && rxr_raster_takes_spans(&P) != 0;
        // device-projected 2D batches: Batch2D::project + the Prim2D records, before anything reads them
        // (a frame without 2D primitives never reads what they would write: no launch)
        project2d = ctx->frame_uses_meshes2d && P.tiles_y && (P.flags & RXR_FLAG_D2_ACTIVE) && ctx->PP2.n_prims;
        if (prepass && ctx->scratch_dirty) {
            // a previous launch sequence was cut short: restore the all-zero invariants explicitly
            HIPCHK(ctx, hipMemsetAsync(ctx->d_bin_count.p, 0, ctx->d_bin_count.cap, s));
            HIPCHK(ctx, hipMemsetAsync(ctx->d_counters.p, 0, ctx->d_counters.cap, s));
        }
        blockscan = prepass && !ctx->blockscan_off && n_bins() * ctx->blockscan_cap <= (size_t)P.list_capacity;
        ctx->last_used_blockscan = blockscan;
        if (!prepass) return RXR_OK;
        ctx->scratch_dirty = true;
        if (blockscan) P.blockscan_cap = ctx->blockscan_cap;
        P.counters = (uint32_t *)ctx->d_counters.p + (size_t)ctx->parity * CNT_WORDS;
        P.counters_next = (uint32_t *)ctx->d_counters.p + (size_t)(ctx->parity ^ 1u) * CNT_WORDS;
        if (!blockscan || P.blockscan_scatter) ctx->parity ^= 1u;
        if (ctx->frame_uses_meshes) project_meshes();
        rxr_launch_setup(&P, s);
        ctx->last_setup_route = 2u;
        if (blockscan) {
            rxr_launch_blockscan(&P, s);
        } else {
            const ScanArgs A = scan_args(P, false);
            rxr_launch_scan(&A, s);
            rxr_launch_fill(&P, s);
        }
        return RXR_OK;
    }

    // 2D binning pre-pass (many 2D primitives): count -> scan -> fill; k_raster sorts each tile's list
    int prepass2d() {
        if (project2d && !projected2d) rxr_launch_project2d(&ctx->PP2, s);
        prepass2d_ran = P.tiles_y && (P.flags & RXR_FLAG_D2_ACTIVE) && P.binned2d;
        if (!prepass2d_ran) return RXR_OK;
        if (ctx->scratch2d_dirty) {
            HIPCHK(ctx, hipMemsetAsync(ctx->d_bin2d_count.p, 0, ctx->d_bin2d_count.cap, s));
            HIPCHK(ctx, hipMemsetAsync((uint32_t *)ctx->d_counters.p + 2 * CNT_WORDS, 0, 2 * CNT_WORDS * sizeof(uint32_t), s));
        }
        ctx->scratch2d_dirty = true;
        const bool blockscan2d = !ctx->blockscan2d_off && n_bins() * RXR_BLOCKSCAN_CAP <= (size_t)P.list2d_capacity;
        ctx->last_used_blockscan2d = blockscan2d;
        P.counters2d = (uint32_t *)ctx->d_counters.p + (size_t)(2u + ctx->parity2d) * CNT_WORDS;
        if (blockscan2d) {  // the counters stay clean (no large list, no ticket); the raster kernel skips its per-tile sort
            P.blockscan2d_cap = RXR_BLOCKSCAN_CAP;
            rxr_launch_blockscan2d(&P, s);
            return RXR_OK;
        }
        P.counters2d_next = (uint32_t *)ctx->d_counters.p + (size_t)(2u + (ctx->parity2d ^ 1u)) * CNT_WORDS;
        ctx->parity2d ^= 1u;
        rxr_launch_bin2d_count(&P, s);
        const ScanArgs A = scan_args(P, true);
        rxr_launch_scan(&A, s);
        rxr_launch_bin2d_fill(&P, s);
        return RXR_OK;
    }

    int raster() {
        if (slot) slot->raster_first = slot->n;
        ctx->last_raster_kernel = "";  // (a frame that launches none: empty, or only filled)
        if (!(bands && bands->n_bands > 1u && spec.tile_stride == 1u && !spec.compact)) {
            if (!rxr_jit_launch(ctx, &P, s)) ctx->last_raster_kernel = launch_raster();
            return RXR_OK;
        }
        const uint32_t n = bands->n_bands;
        uint32_t *const row_of = bands->row_of;
        for (uint32_t k = 0; k <= n; ++k) row_of[k] = k ? spec.row1 : spec.row0;  // (a frame without content: one band of filled rows)
        const uint32_t rows_all = P.tiles_y, first_row = P.tile_y0, r0_all = P.row0, r1_all = P.row1;
        for (uint32_t k = 0; k < n; ++k) {
            const uint32_t a = (uint32_t)((uint64_t)rows_all * k / n), b = (uint32_t)((uint64_t)rows_all * (k + 1u) / n);
            P.bin_row0 = a;
            P.tile_y0 = first_row + a;
            P.tiles_y = b - a;
            P.row0 = std::max(r0_all, (first_row + a) * (uint32_t)RXR_TILE_H);
            P.row1 = std::min(r1_all, (first_row + b) * (uint32_t)RXR_TILE_H);
            // (the first and the last band take the filled rows above / below the content with them)
            row_of[k] = k ? P.row0 : spec.row0;
            row_of[k + 1u] = k + 1u < n ? P.row1 : spec.row1;
            if (P.tiles_y && !rxr_jit_launch(ctx, &P, s)) ctx->last_raster_kernel = launch_raster();
            HIPCHK(ctx, hipEventRecord(bands->events[k], s));
        }
        return RXR_OK;
    }

    int finish() {
        HIPCHK(ctx, hipGetLastError());
        ctx->scratch_dirty = false;  // the raster launch that hands the bins back is queued
        ctx->scratch2d_dirty = false;
        ctx->rendered = true;
        ctx->last_had_prepass = prepass;
        ctx->last_had_prepass2d = prepass2d_ran;
        ctx->launches_since_sync++;
        ctx->last_spec = spec;
        ctx->last_out = dev_pixels;
        ctx->last_stream = s;
        ctx->stats.tiles_x = P.tiles_x;
        ctx->stats.tiles_y = P.tiles_y;
        ctx->stats.n_triangles3d = P.n_tris3d;
        ctx->stats.n_triangles2d = ctx->n_tris2d;
        return RXR_OK;
    }
};

// (every kernel this thread launches until the guard goes takes a start / stop pair of the slot: rxr_launch.h)
struct TimesGuard {
    explicit TimesGuard(ProfSlot *p) { rxr_launch_times = p; }
    ~TimesGuard() { rxr_launch_times = nullptr; }
};

}  // namespace

static int render_impl(rxr_ctx *ctx, const RenderSpec &spec, void *dev_pixels, hipStream_t s, bool retry, RenderBands *bands = nullptr) {
    if (!ctx) return RXR_ERR_INVALID;
    if (!ctx->has_frame) return rxr_fail(ctx, RXR_ERR_INVALID, "render: no frame uploaded");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    Render R{ctx, spec, dev_pixels, s, retry, bands};
    int rc;
    if ((rc = R.order_streams()) != RXR_OK) return rc;
    R.clamp_to_content();
    R.take_profile_slot();
    TimesGuard times_guard(R.slot);  // (cleared on every return path below)
    R.small_frame_records();
    R.fill_outside_content();
    if ((rc = R.prepass3d()) != RXR_OK) return rc;
    if ((rc = R.prepass2d()) != RXR_OK) return rc;
    if ((rc = R.raster()) != RXR_OK) return rc;
    return R.finish();
}

static int band_spec(rxr_ctx *ctx, uint32_t row0, uint32_t row1, bool external, RenderSpec &spec) {
    if (!ctx->has_frame) return rxr_fail(ctx, RXR_ERR_INVALID, "render: no frame uploaded");
    if (row0 > row1 || row1 > ctx->P.height) return rxr_fail(ctx, RXR_ERR_INVALID, "render: bad row range");
    spec.row0 = row0;
    spec.row1 = row1;
    spec.tile_y0 = row0 / RXR_TILE_H;
    spec.tile_stride = 1;
    spec.tiles_y = row1 > row0 ? (row1 + RXR_TILE_H - 1) / RXR_TILE_H - spec.tile_y0 : 0;
    spec.compact = false;
    spec.external = external;
    return RXR_OK;
}

// (who: the entry point's name, for the message)
static int stripes_spec(rxr_ctx *ctx, const char *who, uint32_t first, uint32_t stride, RenderSpec &spec) {
    if (!ctx->has_frame) return rxr_fail(ctx, RXR_ERR_INVALID, "render: no frame uploaded");
    if (stride == 0) return rxr_fail(ctx, RXR_ERR_INVALID, std::string(who) + ": stride 0");
    const uint32_t n_stripes = (ctx->P.height + RXR_TILE_H - 1) / RXR_TILE_H;
    spec.row0 = 0;
    spec.row1 = ctx->P.height;
    spec.tile_y0 = first;
    spec.tile_stride = stride;
    spec.tiles_y = first < n_stripes ? (n_stripes - first + stride - 1) / stride : 0;
    spec.compact = true;
    spec.external = true;
    return RXR_OK;
}

int rxr_render_rows(rxr_ctx *ctx, uint32_t row0, uint32_t row1) {
    if (!ctx) return RXR_ERR_INVALID;
    if (ctx->group)
        return rxr_fail(ctx, RXR_ERR_UNSUPPORTED, "rxr_render_rows on a multi-device context: use rxr_rasterize / rxr_render_download / rxr_render_gather, or drive the members (rxr_member) yourself");
    RenderSpec spec{};
    int rc = band_spec(ctx, row0, row1, false, spec);
    if (rc != RXR_OK) return rc;
    return render_impl(ctx, spec, ctx->d_fb.p, ctx->stream, false);
}

int rxr_render_rows_to(rxr_ctx *ctx, uint32_t row0, uint32_t row1, void *dev_pixels, void *hip_stream) {
    if (!ctx) return RXR_ERR_INVALID;
    if (!dev_pixels) return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_render_rows_to: dev_pixels is NULL");
    if (ctx->group) return rxr_fail(ctx, RXR_ERR_UNSUPPORTED, "rxr_render_rows_to on a multi-device context: device pointers and streams belong to ONE device (use rxr_member)");
    RenderSpec spec{};
    int rc = band_spec(ctx, row0, row1, true, spec);
    if (rc != RXR_OK) return rc;
    return render_impl(ctx, spec, dev_pixels, hip_stream ? (hipStream_t)hip_stream : ctx->stream, false);
}

int rxr_render_stripes_to(rxr_ctx *ctx, uint32_t first, uint32_t stride, void *dev_pixels, void *hip_stream) {
    if (!ctx) return RXR_ERR_INVALID;
    if (!dev_pixels) return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_render_stripes_to: dev_pixels is NULL");
    if (ctx->group) return rxr_fail(ctx, RXR_ERR_UNSUPPORTED, "rxr_render_stripes_to on a multi-device context: device pointers and streams belong to ONE device (use rxr_member)");
    RenderSpec spec{};
    int rc = stripes_spec(ctx, "rxr_render_stripes_to", first, stride, spec);
    if (rc != RXR_OK) return rc;
    return render_impl(ctx, spec, dev_pixels, hip_stream ? (hipStream_t)hip_stream : ctx->stream, false);
}

int rxr_render_stripes_batch(rxr_ctx *ctx, uint32_t first, uint32_t stride, uint32_t n_frames, void *dev_pixels, size_t frame_stride_bytes,
                             void *hip_stream) {
    if (!ctx) return RXR_ERR_INVALID;
    if (!dev_pixels) return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_render_stripes_batch: dev_pixels is NULL");
    if (ctx->group) return rxr_group_render_stripes_batch(ctx, first, stride, n_frames, dev_pixels, frame_stride_bytes, hip_stream);
    RenderSpec spec{};
    int rc = stripes_spec(ctx, "rxr_render_stripes", first, stride, spec);
    if (rc != RXR_OK) return rc;
    if (n_frames > 1u && frame_stride_bytes < (size_t)spec.tiles_y * RXR_TILE_H * ctx->P.width * 4u)
        return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_render_stripes_batch: frame_stride_bytes is smaller than one compact stripe buffer");
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : ctx->stream;
    for (uint32_t k = 0; k < n_frames; ++k)
        if ((rc = render_impl(ctx, spec, (uint8_t *)dev_pixels + (size_t)k * frame_stride_bytes, s, false)) != RXR_OK) return rc;
    return RXR_OK;
}

int rxr_render_spec(rxr_ctx *ctx, const RenderSpec &spec, void *dev_pixels, hipStream_t s) { return render_impl(ctx, spec, dev_pixels, s, false); }

int rxr_profile_begin(rxr_ctx *ctx, uint32_t max_frames) {
    if (!ctx) return RXR_ERR_INVALID;
    if (ctx->group) return rxr_profile_begin(rxr_member(ctx, 0), max_frames);  // kernel timing of a multi-device context: member 0's
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc = rxr_synchronize(ctx);
    if (rc != RXR_OK) return rc;
    for (ProfSlot &p : ctx->prof)
        for (hipEvent_t e : p.ev)
            if (e) (void)hipEventDestroy(e);
    ctx->prof.clear();
    ctx->last_prof = nullptr;
    ctx->prof_next = 0;
    ctx->prof_calls = 0;
    if (max_frames > 65536) max_frames = 65536;
    ctx->prof.assign(max_frames, ProfSlot{});  // (the events of a slot are created when a render first needs them: rxr_launch.h)
    return RXR_OK;
}

int rxr_profile_stride(rxr_ctx *ctx, uint32_t stride) {
    if (!ctx || stride == 0) return RXR_ERR_INVALID;
    if (ctx->group) return rxr_profile_stride(rxr_member(ctx, 0), stride);
    ctx->prof_stride = stride;
    ctx->prof_calls = 0;
    return RXR_OK;
}

int rxr_profile_read(rxr_ctx *ctx, float *setup_us, float *raster_us, uint32_t capacity, uint32_t *n_out) {
    if (!ctx || !n_out) return RXR_ERR_INVALID;
    if (ctx->group) return rxr_profile_read(rxr_member(ctx, 0), setup_us, raster_us, capacity, n_out);
    int rc = rxr_synchronize(ctx);
    if (rc != RXR_OK) return rc;
    uint32_t n = (uint32_t)std::min<size_t>(std::min<size_t>(ctx->prof_next, ctx->prof.size()), capacity);
    for (uint32_t i = 0; i < n; ++i) {
        float a = 0, b = 0;
        if (!rxr_prof_slot_us(ctx->prof[i], &a, &b)) return rxr_fail(ctx, RXR_ERR_HIP, "rxr_profile_read: a kernel's start / stop events could not be read");
        if (setup_us) setup_us[i] = a;
        if (raster_us) raster_us[i] = b;
    }
    *n_out = n;
    ctx->prof_next = 0;
    return RXR_OK;
}

// rxr_synchronize: a sticky status word that is an error -- RXR_OK when there is none
static int report_faults(rxr_ctx *ctx, uint32_t *hc) {
    if (hc[HS_VM_FAULT]) {
        // a fragment's program did what makes the reference panic (rxr_vm.h, VMF_*)
        static const char *const what[] = {"", "stack underflow", "stack overflow", "local index out of range", "global index out of range",
                                           "call depth", "loop depth", "instruction limit (runaway loop)", "clamp with min > max",
                                           "call of a missing function", "bad opcode", "too many locals"};
        uint32_t code = hc[HS_VM_FAULT];
        hc[HS_VM_FAULT] = 0;
        return rxr_fail(ctx, RXR_ERR_INVALID, std::string("shader program fault: ") + (code < sizeof(what) / sizeof(what[0]) ? what[code] : "?"));
    }
    if (hc[HS_BAD_LINE2D]) {
        hc[HS_BAD_LINE2D] = 0;
        return rxr_fail(ctx, RXR_ERR_UNSUPPORTED, "batch2d: line end point NaN or beyond +-2^30");
    }
    if (hc[HS_STAIRCASE]) {
        hc[HS_STAIRCASE] = 0;
        return rxr_fail(ctx, RXR_ERR_UNSUPPORTED,
                        "four or more groups of opacity batches nest as prefix minima in one pixel: the device keeps three per pixel (surface_id, "
                        "rasterizer.rs:314-357, :1044-1048) and had to drop one; the frame may differ from the reference");
    }
    return RXR_OK;
}

// Waits for everything this context has queued and reports what the launches since the previous call left in the pinned
// status words.  Those words are sticky (the device only sets / raises them), so an overflow or a program fault of ANY
// launch since the last call is seen, not only the last one's:
//   - a bin list overflowed: the lists are grown; the LAST launch is rendered again (its output is then complete); if
//     earlier launches were queued in between (an asynchronous caller that does not synchronize per frame) their frames
//     were shipped incomplete and the call returns RXR_ERR_OVERFLOW to say so;
//   - a fragment's program faulted, or an opacity staircase dropped an entry: an error, see the messages.
int rxr_synchronize(rxr_ctx *ctx) {
    if (!ctx) return RXR_ERR_INVALID;
    if (ctx->group) return rxr_group_synchronize(ctx);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    bool earlier_incomplete = false;
    for (int attempt = 0; attempt < 4; ++attempt) {
        int rc = rxr_quiesce(ctx);
        if (rc != RXR_OK) return rc;
        const uint32_t launches = ctx->launches_since_sync;
        ctx->launches_since_sync = 0;
        if (ctx->h_bake_fault && ctx->h_bake_fault[0]) return rxr_bake_report_fault(ctx);  // a queued bake's program faulted (rxr_bake.hip)
        if (!ctx->rendered) return RXR_OK;
        uint32_t *hc = ctx->h_counters;
        if (hc[HS_VM_FAULT] == VMF_JIT_PALETTE_MISS) {
            // not a fault of the program: a compiled set met a palette slot without a colour, where the reference pushes nothing -- only
            // the interpreter's dynamic stack follows that.  The set runs interpreted from now on; the last launch is rendered again, an
            // earlier one of this batch of launches was incomplete (reported like an overflow).
            hc[HS_VM_FAULT] = 0;
            ctx->jit_palette_miss = true;
            ctx->jit_info = "not compiled: a PaletteIndex met a missing or empty palette slot (the interpreter follows the reference's shorter stack)";
            if (launches > 1u) earlier_incomplete = true;
            if ((rc = render_impl(ctx, ctx->last_spec, ctx->last_out, ctx->last_stream, true)) != RXR_OK) return rc;
            continue;
        }
        if ((rc = report_faults(ctx, hc)) != RXR_OK) return rc;
        ctx->stats.n_bin_entries = (ctx->last_had_prepass && !ctx->last_used_blockscan) ? hc[CNT_ENTRIES] : 0u;  // (k_blockscan does not count its entries)
        const bool over3d = hc[CNT_OVERFLOW] != 0, over2d = hc[CNT_WORDS + CNT_OVERFLOW] != 0;
        if (!over3d && !over2d) {
            float a = 0, b = 0;
            if (ctx->last_prof && rxr_prof_slot_us(*ctx->last_prof, &a, &b)) {
                ctx->stats.setup_us = a;
                ctx->stats.raster_us = b;
                ctx->stats.total_us = a + b;
            }
            if (earlier_incomplete)
                return rxr_fail(ctx, RXR_ERR_OVERFLOW,
                                "a bin list overflowed in a launch that was not the last one before this rxr_synchronize: that frame was "
                                "incomplete (the lists have been grown and the last launch rendered again)");
            return RXR_OK;
        }
        if (launches > 1u) earlier_incomplete = true;
        if (over2d && ctx->last_used_blockscan2d) {
            // a block of bins or a bin had more 2D primitives than k_blockscan2d keeps: count / scan / fill (and the per-tile sort) for this frame
            ctx->blockscan2d_off = true;
            ctx->blockscan2d_bad.add(ctx->P.n_prims2d, (size_t)ctx->P.tiles_x * ((ctx->P.height + RXR_TILE_H - 1) / RXR_TILE_H));
            hc[CNT_WORDS + CNT_OVERFLOW] = hc[CNT_WORDS + HS_MAX_ENTRIES] = 0;
        } else if (over2d) {
            const size_t seen = std::max(hc[CNT_WORDS + HS_MAX_ENTRIES], hc[CNT_WORDS + CNT_ENTRIES]);
            if ((rc = rxr_ensure(ctx, ctx->d_list2d, (seen + seen / 2 + 1024) * sizeof(uint32_t))) != RXR_OK) return rc;
            ctx->list2d_capacity = (uint32_t)std::min<size_t>(ctx->d_list2d.cap / sizeof(uint32_t), 0xFFFFFFF0u);
            ctx->P.bin2d_list = (uint32_t *)ctx->d_list2d.p;
            ctx->P.list2d_capacity = ctx->list2d_capacity;
            hc[CNT_WORDS + CNT_OVERFLOW] = hc[CNT_WORDS + HS_MAX_ENTRIES] = 0;
        }
        if (over3d && ctx->last_used_blockscan) {
            // a block of bins or a bin had more candidates than k_blockscan keeps: this frame takes the general pipeline
            ctx->blockscan_off = true;
            ctx->blockscan_bad.add(ctx->P.n_tris3d, (size_t)ctx->P.tiles_x * ((ctx->P.height + RXR_TILE_H - 1) / RXR_TILE_H));
            hc[CNT_OVERFLOW] = hc[HS_MAX_ENTRIES] = 0;
        } else if (over3d) {
            const size_t seen = std::max(hc[HS_MAX_ENTRIES], hc[CNT_ENTRIES]);
            if ((rc = rxr_ensure(ctx, ctx->d_list, (seen + seen / 2 + 1024) * sizeof(uint32_t))) != RXR_OK) return rc;
            ctx->list_capacity = (uint32_t)std::min<size_t>(ctx->d_list.cap / sizeof(uint32_t), 0xFFFFFFF0u);
            ctx->P.bin_list = (uint32_t *)ctx->d_list.p;
            ctx->P.list_capacity = ctx->list_capacity;
            hc[CNT_OVERFLOW] = hc[HS_MAX_ENTRIES] = 0;
        }
        // the same launch again, now with room (the streams are idle: see rxr_quiesce above)
        if ((rc = render_impl(ctx, ctx->last_spec, ctx->last_out, ctx->last_stream, true)) != RXR_OK) return rc;
    }
    return rxr_fail(ctx, RXR_ERR_OOM, "bin list kept overflowing");
}

int rxr_download_rows(rxr_ctx *ctx, uint8_t *pixels, uint32_t row0, uint32_t row1) {
    if (!ctx || !pixels) return RXR_ERR_INVALID;
    if (ctx->group) return rxr_fail(ctx, RXR_ERR_UNSUPPORTED, "rxr_download_rows on a multi-device context: use rxr_rasterize / rxr_render_download");
    if (!ctx->has_frame || row0 > row1 || row1 > ctx->P.height) return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_download_rows: bad row range or no frame");
    int rc = rxr_synchronize(ctx);
    if (rc != RXR_OK) return rc;
    size_t off = (size_t)row0 * ctx->P.width * 4, bytes = (size_t)(row1 - row0) * ctx->P.width * 4;
    if (bytes) {
        HIPCHK(ctx, hipMemcpyAsync(pixels + off, (uint8_t *)ctx->d_fb.p + off, bytes, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    return RXR_OK;
}

int rxr_rasterize(rxr_ctx *ctx, const rxr_frame *frame, uint8_t *pixels) {
    if (!ctx || !pixels) return RXR_ERR_INVALID;
    int rc = rxr_upload_frame(ctx, frame);
    if (rc != RXR_OK) return rc;
    return rxr_render_download(ctx, pixels);
}

// rxr_render_download of a frame that is not pipelined: one render, then one download
static int render_then_download(rxr_ctx *ctx, uint8_t *pixels) {
    const uint32_t H = ctx->P.height;
    int rc;
    static const bool timing = getenv("RXR_E2E_TIMING") != nullptr;  // diagnostics (tools/e2e_probe.py): where a large frame's call goes
    if (timing) {
        using clk = std::chrono::steady_clock;
        HIPCHK(ctx, hipSetDevice(ctx->device));
        const auto t0 = clk::now();
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));  // the tail of the upload's host->device copies
        const auto t1 = clk::now();
        rc = rxr_render_rows(ctx, 0, H);
        if (rc != RXR_OK) return rc;
        rc = rxr_synchronize(ctx);
        if (rc != RXR_OK) return rc;
        const auto t2 = clk::now();
        rc = rxr_download_rows(ctx, pixels, 0, H);
        const auto t3 = clk::now();
        auto ms = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
        fprintf(stderr, "rxr_e2e_timing h2d_tail_ms=%.3f kernels_ms=%.3f download_ms=%.3f\n", ms(t0, t1), ms(t1, t2), ms(t2, t3));
        return rc;
    }
    rc = rxr_render_rows(ctx, 0, H);
    if (rc != RXR_OK) return rc;
    return rxr_download_rows(ctx, pixels, 0, H);
}

// [0, 0, 0, 255] per fill pixel, written by helper threads while the device renders and the link is busy (they start BEFORE the copies
// are queued: a copy into pageable memory keeps the calling thread until it has landed).  Every return path of the owner, errors
// included, waits for the helpers: they write the caller's buffer.
namespace {
struct FillHelpers {
    std::vector<std::thread> threads;
    FillHelpers(const std::vector<DownloadRect> &fills, uint8_t *pixels, uint32_t W, size_t n_px) {
        const uint32_t n_threads = n_px >= (12u << 20) ? 8u : (n_px >= (4u << 20) ? 4u : (n_px ? 1u : 0u));
        threads.reserve(n_threads);
        for (uint32_t t = 0; t < n_threads; ++t) {
            try {
                threads.emplace_back([&fills, pixels, W, t, n_threads] { rxr_write_fills(pixels, W, fills, t, n_threads); });
            } catch (...) {  // (no thread to be had: this share is written here and now -- nothing may leave through the C ABI)
                rxr_write_fills(pixels, W, fills, t, n_threads);
            }
        }
    }
    void join() {
        for (std::thread &th : threads)
            if (th.joinable()) th.join();
    }
    ~FillHelpers() { join(); }
};
}  // namespace

// every band's copies behind its event, on the copy stream (ascending rows; every strip lies inside one band)
static int queue_band_copies(rxr_ctx *ctx, const std::vector<DownloadRect> &copies, const uint32_t *row_of, uint32_t n_bands, uint8_t *pixels) {
    const uint32_t W = ctx->P.width;
    size_t ci = 0;
    for (uint32_t k = 0; k < n_bands; ++k) {
        HIPCHK(ctx, hipStreamWaitEvent(ctx->copy_stream, ctx->ev_band[k], 0));
        for (; ci < copies.size() && copies[ci].r0 < row_of[k + 1]; ++ci) {
            const DownloadRect &c = copies[ci];
            const size_t off = ((size_t)c.r0 * W + c.x0) * 4;
            if (c.x0 == 0u && c.x1 == W) {
                HIPCHK(ctx, hipMemcpyAsync(pixels + off, (uint8_t *)ctx->d_fb.p + off, (size_t)(c.r1 - c.r0) * W * 4, hipMemcpyDeviceToHost, ctx->copy_stream));
            } else {
                HIPCHK(ctx, hipMemcpy2DAsync(pixels + off, (size_t)W * 4, (uint8_t *)ctx->d_fb.p + off, (size_t)W * 4, (size_t)(c.x1 - c.x0) * 4, c.r1 - c.r0,
                                             hipMemcpyDeviceToHost, ctx->copy_stream));
            }
        }
    }
    return RXR_OK;
}

// The download of a 4K frame over PCIe takes longer than rendering it, so frames of 4 Mpixel and more are rastered in bands of tile
// rows and every finished band travels to the caller's buffer while the next ones render; rendering in bands is byte-identical to
// one launch (tested).  Measured: 3840x2160 0.90 -> 0.76 ms per call; at 1920x1080 the extra launches cost more than the overlap
// gains (0.26 -> 0.31 ms), hence the threshold.  Rounds 1-3 made four whole launch sequences of it and therefore served frames
// without a pre-pass only; since round 4 ONE pre-pass (projection, set-up, bins) is followed by four raster launches over its bins
// (render_impl, RasterParams.bin_row0), which serves binned and device-projected frames as well: the 8K frame of 1 M triangles
// downloads 133 MB in 2.4 ms behind 0.6 ms of kernels that used to come first.  A list overflow is repaired by rxr_synchronize as
// ever (lists grown, the whole frame rendered again); the frame is then downloaded once more.
int rxr_render_download(rxr_ctx *ctx, uint8_t *pixels) {
    if (!ctx || !pixels) return RXR_ERR_INVALID;
    if (ctx->group) return rxr_group_render_download(ctx, pixels);
    if (!ctx->has_frame) return rxr_fail(ctx, RXR_ERR_INVALID, "rxr_render_download: no frame uploaded");
    const uint32_t W = ctx->P.width, H = ctx->P.height;
    static const bool no_pipeline = getenv("RXR_NO_DOWNLOAD_PIPELINE") != nullptr;  // A-B runs
    if (no_pipeline || (size_t)W * H < (1u << 22)) return render_then_download(ctx, pixels);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // 1. the render, in bands
    constexpr uint32_t n_bands = 4;
    uint32_t row_of[n_bands + 1] = {};
    RenderSpec spec{};
    int rc = band_spec(ctx, 0, H, false, spec);
    if (rc != RXR_OK) return rc;
    const uint32_t rerenders_before = ctx->rerenders;
    RenderBands bands{n_bands, ctx->ev_band, row_of, ctx->ev_band[7], false};
    if ((rc = render_impl(ctx, spec, ctx->d_fb.p, ctx->stream, false, &bands)) != RXR_OK) return rc;
    // 2. Rows outside the frame's content are the miss colour on the device AND need not cross PCIe: the caller's rows are written here,
    // by the host, while the device renders and the content rows travel (the 8K frame of the box grid: 40 of 133 MB that are not
    // downloaded; the link is what bounds this call).
    uint32_t c0 = 0, c1 = H;
    bool clipped = content_band(ctx, spec, c0, c1);
    const uint2 *const back = ctx->h_row_spans + RXR_MAX_TILE_ROWS;
    if (bands.spans_recorded) {
        // device-projected meshes: the content is known once the projection has run -- the device hands its row-span table back a
        // fraction of a millisecond into the frame (k_spans_from_meshes writes a copy into page-locked memory, an event behind it),
        // long before the first band is rastered; this thread would only wait for the bands otherwise
        HIPCHK(ctx, hipEventSynchronize(ctx->ev_band[7]));
        if (rxr_table_content_rows((const uint32_t *)back, H, ctx->P.tiles_x, content_min_tiles(), c0, c1)) clipped = true;
    }
    // 3. ... and inside the content rows the columns outside the tile rows' spans (host-projected frames: the table of rxr_upload_frame;
    // device-projected ones: the table the device has just handed back): which rectangles travel, which the host writes
    const uint2 *table = bands.spans_recorded ? back : (ctx->spans_active && ctx->content_known ? ctx->h_row_spans : nullptr);
    if (getenv("RXR_NO_COLUMN_TRIM")) table = nullptr;  // A-B runs, tests (read per call)
    const DownloadPlan plan = rxr_plan_download(W, H, row_of, n_bands, c0, c1, clipped, content_min_tiles(), (const uint32_t *)table, RXR_MAX_TILE_ROWS);
    ctx->last_download_bytes = plan.link_bytes;
    ctx->last_host_fill_bytes = plan.host_bytes;
    // 4. - 6. the fills start, the copies are queued, the fills are joined (before anything below can write the same bytes again: the
    // repaired frame's download)
    FillHelpers helpers(plan.fills, pixels, W, (size_t)(plan.host_bytes / 4u));
    if ((rc = queue_band_copies(ctx, plan.copies, row_of, n_bands, pixels)) != RXR_OK) return rc;
    helpers.join();
    // 7. and 8.
    HIPCHK(ctx, hipStreamSynchronize(ctx->copy_stream));
    rc = rxr_synchronize(ctx);  // (program faults and list overflows are reported / repaired here)
    if (rc != RXR_OK) return rc;
    if (ctx->rerenders != rerenders_before) return rxr_download_rows(ctx, pixels, 0, H);  // the bands that travelled were incomplete
    return RXR_OK;
}

int rxr_get_stats(rxr_ctx *ctx, rxr_stats *out) {
    if (!ctx || !out) return RXR_ERR_INVALID;
    if (ctx->group) return rxr_group_get_stats(ctx, out);
    *out = ctx->stats;
    return RXR_OK;
}

void *rxr_device_framebuffer(rxr_ctx *ctx) { return (ctx && !ctx->group) ? ctx->d_fb.p : nullptr; }
