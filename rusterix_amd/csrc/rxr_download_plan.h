// rxr_download_plan.h -- the integer geometry of the banded rxr_render_download (rxr_render.hip): which rectangles of the frame cross
// PCIe and which the host writes itself.  Host only and free of HIP, so that tests/download_plan_main.cpp runs it without a device.
#ifndef RXR_DOWNLOAD_PLAN_H
#define RXR_DOWNLOAD_PLAN_H

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "rxr_device.h"  // RXR_TILE_W / RXR_TILE_H

struct DownloadRect {
    uint32_t r0, r1, x0, x1;  // pixel rows [r0, r1), pixel columns [x0, x1)
};

struct DownloadPlan {
    std::vector<DownloadRect> fills, copies;         // the host writes the miss colour / the link carries; copies in ascending rows, each inside one band
    uint64_t link_bytes = 0, host_bytes = 0;
};

// The content rows [c0, c1) of a frame of H rows from a row-span table the device handed back (pairs [x, y) of tile columns per tile row):
// the rows of its non-empty entries.  False, c0 and c1 untouched, when that leaves out fewer than min_tiles tiles (as content_band: a few
// rows are not worth the fills).
static inline bool rxr_table_content_rows(const uint32_t *back, uint32_t H, uint32_t tiles_x, size_t min_tiles, uint32_t &c0, uint32_t &c1) {
    const uint32_t n_rows = (H + RXR_TILE_H - 1u) / RXR_TILE_H;
    uint32_t r0 = n_rows, r1 = 0;
    for (uint32_t r = 0; r < n_rows; ++r)
        if (back[2u * r] < back[2u * r + 1u]) {
            r0 = std::min(r0, r);
            r1 = r + 1u;
        }
    const uint32_t d0 = r0 < r1 ? r0 * RXR_TILE_H : 0u, d1 = r0 < r1 ? std::min(r1 * (uint32_t)RXR_TILE_H, H) : 0u;
    if ((size_t)(d0 + (H - d1)) / RXR_TILE_H * tiles_x < min_tiles) return false;
    c0 = d0;
    c1 = d1;
    return true;
}

// A W x H frame rastered in n_bands bands of rows [row_of[k], row_of[k + 1]), its content in rows [c0, c1) (clipped: the rows outside
// them are the miss colour).  Inside the content rows the columns outside the tile rows' spans (table: n_table pairs [x, y) of tile
// columns, or null) are the miss colour as well: each band travels as two strips over the union of its tile rows' spans, the host writes
// what lies to the left and right.  Strips, not tile rows: a 2D copy costs about 13 us of its own (tools/microbench/copy2d.hip: 91 MB of
// whole rows 1.64 ms; the same trapezoid in 4 / 24 / 93 strips 1.18 / 1.33 / 2.05 ms).
// (the table says where anything CAN be drawn whether or not the launches used it: a frame whose content reaches from the first row to
// the last is not clamped in rows, but its row ends are still the miss colour)
static inline DownloadPlan rxr_plan_download(uint32_t W, uint32_t H, const uint32_t *row_of, uint32_t n_bands, uint32_t c0, uint32_t c1, bool clipped,
                                             size_t min_tiles, const uint32_t *table, uint32_t n_table) {
    DownloadPlan D;
    std::vector<DownloadRect> &fills = D.fills, &copies = D.copies;
    if (clipped) {
        fills.push_back({0u, c0, 0u, W});
        fills.push_back({c1, H, 0u, W});
    }
    constexpr uint32_t n_sub = 2;
    size_t trimmed_px = 0;
    for (uint32_t k = 0; k < n_bands; ++k) {
        const uint32_t a = std::max(row_of[k], c0), b = std::min(row_of[k + 1], c1);
        if (b <= a) continue;
        const uint32_t ta = a / RXR_TILE_H, tb = (b + RXR_TILE_H - 1u) / RXR_TILE_H;  // tile rows of the band
        for (uint32_t j = 0; j < (table ? n_sub : 1u); ++j) {
            const uint32_t t0 = table ? ta + (tb - ta) * j / n_sub : ta, t1 = table ? ta + (tb - ta) * (j + 1u) / n_sub : tb;
            const uint32_t r0 = std::max(a, t0 * (uint32_t)RXR_TILE_H), r1 = std::min(b, t1 * (uint32_t)RXR_TILE_H);
            if (r1 <= r0) continue;
            uint32_t x0 = 0u, x1 = W;
            if (table) {
                uint32_t lo = 0xFFFFFFFFu, hi = 0u;
                for (uint32_t t = t0; t < t1 && t < n_table; ++t)
                    if (table[2u * t] < table[2u * t + 1u]) {
                        lo = std::min(lo, table[2u * t]);
                        hi = std::max(hi, table[2u * t + 1u]);
                    }
                if (lo >= hi) {  // nothing in these rows at all
                    fills.push_back({r0, r1, 0u, W});
                    trimmed_px += (size_t)(r1 - r0) * W;
                    continue;
                }
                x0 = std::min(lo * (uint32_t)RXR_TILE_W, W);
                x1 = std::min(hi * (uint32_t)RXR_TILE_W, W);
                if ((size_t)(x1 - x0) * 10u >= (size_t)W * 9u) {  // (nearly the whole width: one contiguous copy is cheaper than a strided one)
                    x0 = 0u;
                    x1 = W;
                }
                trimmed_px += (size_t)(r1 - r0) * (W - (x1 - x0));
            }
            copies.push_back({r0, r1, x0, x1});
        }
    }
    if (table && trimmed_px < min_tiles * (size_t)(RXR_TILE_W * RXR_TILE_H)) {  // (8 MB by default) not worth the strided copies and the fills: whole rows, as without a table
        copies.clear();
        fills.resize(clipped ? 2u : 0u);
        for (uint32_t k = 0; k < n_bands; ++k) {
            const uint32_t a = std::max(row_of[k], c0), b = std::min(row_of[k + 1], c1);
            if (b > a) copies.push_back({a, b, 0u, W});
        }
    }
    for (const DownloadRect &c : copies)
        if (!(c.x0 == 0u && c.x1 == W)) {
            fills.push_back({c.r0, c.r1, 0u, c.x0});
            fills.push_back({c.r0, c.r1, c.x1, W});
        }
    size_t n_px = 0;
    for (const DownloadRect &f : fills) n_px += f.r1 > f.r0 && f.x1 > f.x0 ? (size_t)(f.r1 - f.r0) * (f.x1 - f.x0) : 0u;
    for (const DownloadRect &c : copies) D.link_bytes += (uint64_t)(c.r1 - c.r0) * (c.x1 - c.x0) * 4u;
    D.host_bytes = (uint64_t)n_px * 4u;
    return D;
}

// Share `me` of `of` of the fills, into the caller's W pixels wide frame: [0, 0, 0, 255] per pixel (:420-461).  Rows are dealt round
// robin; the buffer may be unaligned: bytes then.
static inline void rxr_write_fills(uint8_t *pixels, uint32_t W, const std::vector<DownloadRect> &fills, uint32_t me, uint32_t of) {
    const bool aligned = ((uintptr_t)pixels & 3u) == 0u;
    uint32_t turn = 0;
    for (const DownloadRect &f : fills) {
        if (f.r1 <= f.r0 || f.x1 <= f.x0) continue;
        for (uint32_t r = f.r0; r < f.r1; ++r, ++turn) {
            if (turn % of != me) continue;
            uint8_t *p = pixels + ((size_t)r * W + f.x0) * 4;
            const size_t n = f.x1 - f.x0;
            if (aligned) std::fill((uint32_t *)p, (uint32_t *)p + n, 0xFF000000u);
            else
                for (size_t i = 0; i < n; ++i) { p[4 * i] = 0; p[4 * i + 1] = 0; p[4 * i + 2] = 0; p[4 * i + 3] = 255; }
        }
    }
}

#endif  // RXR_DOWNLOAD_PLAN_H
