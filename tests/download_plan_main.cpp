// download_plan_main.cpp -- the rectangle geometry of the banded rxr_render_download (rusterix_amd/csrc/rxr_download_plan.h: which parts of a
// frame cross PCIe and which the host writes) as a program of its own.  Built with a host compiler (-O2), and once more with
// -fsanitize=address,undefined; tests/test_download_plan_cpu.py runs both.
//
//   download_plan_main fuzz SEED CASES   seeded frames up to 300x300: content rows on tile rows (or none), row_of as render_impl derives it for
//                                        four bands, a span table (or none) whose spans lie in content tile rows only, min_tiles zero or small;
//                                        checks the six conditions at check_case below, prints one line of counts; exit status 1 with the
//                                        offending case on a miss
//   download_plan_main known             the plan worked out by hand, and a frame without content rows
//   download_plan_main fills             rxr_write_fills into an aligned and an unaligned buffer, split across 1, 4 and 8 workers
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../rusterix_amd/csrc/rxr_download_plan.h"

static const uint32_t TILE = 16u, N_BANDS = 4u;
static_assert(RXR_TILE_W == 16 && RXR_TILE_H == 16, "the hand-made cases assume 16x16 tiles");

// xorshift64*: the same numbers everywhere
struct Rng {
    uint64_t s;
    explicit Rng(uint64_t seed) : s(seed * 0x9E3779B97F4A7C15ull + 0x1234567ull) {
        if (!s) s = 1;
    }
    uint64_t next() {
        s ^= s >> 12;
        s ^= s << 25;
        s ^= s >> 27;
        return s * 0x2545F4914F6CDD1Dull;
    }
    uint32_t below(uint32_t n) { return (uint32_t)(next() >> 33) % n; }
};

struct Case {
    uint32_t W = 0, H = 0, c0 = 0, c1 = 0, row_of[N_BANDS + 1] = {};
    bool clipped = false, has_table = false;
    size_t min_tiles = 0;
    std::vector<uint32_t> table;  // pairs, one per tile row of the frame
    const uint32_t *tab() const { return has_table ? table.data() : nullptr; }
    uint32_t n_tab() const { return (uint32_t)(table.size() / 2u); }
    DownloadPlan plan(size_t mt) const { return rxr_plan_download(W, H, row_of, N_BANDS, c0, c1, clipped, mt, tab(), n_tab()); }
};

// row_of as render_impl's banded raster leaves it: the launch covers the rows [c0, c1) (the spec's rows [0, H) clamped to the content),
// its tile rows are dealt to the bands, the first and the last band take the rows outside the content with them
static void bands_of(Case &C) {
    for (uint32_t k = 0; k <= N_BANDS; ++k) C.row_of[k] = k ? C.H : 0u;  // (a frame without content)
    const uint32_t first_row = C.c0 / TILE, rows_all = C.c1 > C.c0 ? (C.c1 + TILE - 1u) / TILE - first_row : 0u;
    for (uint32_t k = 0; k < N_BANDS; ++k) {
        const uint32_t a = (uint32_t)((uint64_t)rows_all * k / N_BANDS), b = (uint32_t)((uint64_t)rows_all * (k + 1u) / N_BANDS);
        const uint32_t row0 = std::max(C.c0, (first_row + a) * TILE), row1 = std::min(C.c1, (first_row + b) * TILE);
        C.row_of[k] = k ? row0 : 0u;
        C.row_of[k + 1u] = k + 1u < N_BANDS ? row1 : C.H;
    }
}

static Case draw(Rng &R) {
    Case C;
    C.W = 1u + R.below(300u);
    C.H = 1u + R.below(300u);
    const uint32_t n_rows = (C.H + TILE - 1u) / TILE, n_cols = (C.W + TILE - 1u) / TILE;
    C.c0 = 0u;
    C.c1 = C.H;
    const uint32_t kind = R.below(8u);
    if (kind >= 2u) {  // content rows on tile rows; kind 7: none at all
        const uint32_t t0 = R.below(n_rows), t1 = kind == 7u ? t0 : t0 + 1u + R.below(n_rows - t0);
        C.clipped = true;
        C.c0 = t0 * TILE;
        C.c1 = std::min(t1 * TILE, C.H);
    }
    bands_of(C);
    C.has_table = R.below(4u) != 0u;
    C.table.assign(2u * n_rows, 0u);
    const uint32_t style = R.below(3u);  // narrow spans, wide ones, anything
    for (uint32_t t = 0; t < n_rows; ++t) {
        uint32_t x = R.below(2u) ? n_cols : 0u, y = 0u;  // an empty row, as the upload leaves it or all zero
        const bool inside = t * TILE >= C.c0 && t * TILE < C.c1;
        if (inside && R.below(5u) != 0u) {
            if (style == 0u) {
                x = R.below(n_cols);
                y = std::min(n_cols, x + 1u + R.below(3u));
            } else if (style == 1u) {
                x = R.below(2u) ? 0u : R.below(std::max(1u, n_cols / 8u));
                y = n_cols - (R.below(2u) ? 0u : R.below(std::max(1u, n_cols / 8u)));
                if (x >= y) { x = 0u; y = n_cols; }
            } else {
                x = R.below(n_cols);
                y = x + 1u + R.below(n_cols - x);
            }
        }
        C.table[2u * t] = x;
        C.table[2u * t + 1u] = y;
    }
    static const size_t mins[8] = {0, 0, 0, 1, 2, 5, 20, 100};
    C.min_tiles = mins[R.below(8u)];
    return C;
}

struct Tally {
    unsigned long cases = 0, strided = 0, filled_strips = 0, fallback = 0, nine_tenths = 0, no_table = 0, clipped = 0, copies = 0, fills = 0;
};

#define REQUIRE(cond, ...)                       \
    do {                                         \
        if (!(cond)) {                           \
            fprintf(stderr, "download_plan_main: " __VA_ARGS__); \
            fprintf(stderr, " [%s]\n", #cond);   \
            return false;                        \
        }                                        \
    } while (0)

static bool empty(const DownloadRect &r) { return r.r1 <= r.r0 || r.x1 <= r.x0; }

// The pixels inside the content rows that need not travel, counted row by row from the table alone: a row belongs to the upper or the
// lower half of its band's tile rows; it keeps the union of that half's spans, all of its width when that is nine tenths of it, nothing
// when the half has no span
static uint64_t trimmed_by_rows(const Case &C) {
    uint64_t px = 0;
    for (uint32_t y = C.c0; y < C.c1; ++y) {
        uint32_t k = 0;
        while (!(C.row_of[k] <= y && y < C.row_of[k + 1u])) ++k;
        const uint32_t a = std::max(C.row_of[k], C.c0), b = std::min(C.row_of[k + 1u], C.c1);
        const uint32_t ta = a / TILE, tb = (b + TILE - 1u) / TILE, mid = ta + (tb - ta) / 2u, upper = y / TILE < mid;
        uint32_t lo = 0xFFFFFFFFu, hi = 0u;
        for (uint32_t t = upper ? ta : mid; t < (upper ? mid : tb); ++t)
            if (C.table[2u * t] < C.table[2u * t + 1u]) {
                lo = std::min(lo, C.table[2u * t]);
                hi = std::max(hi, C.table[2u * t + 1u]);
            }
        uint32_t kept = lo < hi ? std::min(hi * TILE, C.W) - std::min(lo * TILE, C.W) : 0u;
        if (lo < hi && (uint64_t)kept * 10u >= (uint64_t)C.W * 9u) kept = C.W;
        px += C.W - kept;
    }
    return px;
}

// The conditions (numbers as in tests/test_download_plan_cpu.py):
//  1. every pixel of the frame lies in exactly one rectangle of fills and copies
//  2. copies are in ascending rows, each inside one band
//  3. every pixel inside a tile row's span lies in a copy
//  4. link bytes + host bytes = W * H * 4
//  5. without a table: exactly one whole-width copy per non-empty band
//  6. trimmed pixels under min_tiles * 256: all copies whole-width, fills only the rows outside the content -- otherwise the plan is the
//     one min_tiles = 0 gives; a strip is whole-width although its spans are not only under the nine-tenths rule, and strided copies
//     cover exactly the union of their tile rows' spans
static bool check_case(const Case &C, Tally &T) {
    const uint32_t W = C.W, H = C.H;
    const DownloadPlan D = C.plan(C.min_tiles);
    std::vector<uint8_t> owner((size_t)W * H, 0);  // 1: a copy, 2: a fill
    for (int pass = 0; pass < 2; ++pass)
        for (const DownloadRect &r : pass ? D.fills : D.copies) {
            if (pass && empty(r)) continue;  // (rxr_write_fills skips them)
            REQUIRE(r.r0 < r.r1 && r.r1 <= H && r.x0 < r.x1 && r.x1 <= W, "%s rows [%u, %u) columns [%u, %u) of %ux%u", pass ? "fill" : "copy", r.r0, r.r1, r.x0, r.x1, W, H);
            for (uint32_t y = r.r0; y < r.r1; ++y)
                for (uint32_t x = r.x0; x < r.x1; ++x) {
                    REQUIRE(owner[(size_t)y * W + x] == 0, "pixel (%u, %u) of %ux%u lies in two rectangles", x, y, W, H);  // 1
                    owner[(size_t)y * W + x] = pass ? 2 : 1;
                }
        }
    for (size_t i = 0; i < owner.size(); ++i) REQUIRE(owner[i] != 0, "pixel (%zu, %zu) of %ux%u lies in no rectangle", i % W, i / W, W, H);  // 1
    for (size_t i = 0; i < D.copies.size(); ++i) {  // 2
        const DownloadRect &c = D.copies[i];
        if (i) REQUIRE(D.copies[i - 1].r1 <= c.r0, "copy %zu starts at row %u, before the end of the previous one", i, c.r0);
        bool in_band = false;
        for (uint32_t k = 0; k < N_BANDS; ++k) in_band = in_band || (C.row_of[k] <= c.r0 && c.r1 <= C.row_of[k + 1u]);
        REQUIRE(in_band, "copy %zu, rows [%u, %u), lies in no single band", i, c.r0, c.r1);
    }
    if (C.has_table)  // 3
        for (uint32_t t = 0; t < C.n_tab(); ++t)
            for (uint32_t y = t * TILE; y < std::min((t + 1u) * TILE, H); ++y)
                for (uint32_t x = C.table[2u * t] * TILE; x < std::min(C.table[2u * t + 1u] * TILE, W) && C.table[2u * t] < C.table[2u * t + 1u]; ++x)
                    REQUIRE(owner[(size_t)y * W + x] == 1, "pixel (%u, %u) inside tile row %u's span is not copied", x, y, t);
    REQUIRE(D.link_bytes + D.host_bytes == (uint64_t)W * H * 4u, "%llu + %llu bytes", (unsigned long long)D.link_bytes, (unsigned long long)D.host_bytes);  // 4
    const uint64_t outside_px = C.clipped ? (uint64_t)(C.c0 + (H - C.c1)) * W : 0u;
    size_t n_whole = 0, bands_with_rows = 0;
    for (const DownloadRect &c : D.copies) n_whole += c.x0 == 0u && c.x1 == W;
    for (uint32_t k = 0; k < N_BANDS; ++k) bands_with_rows += std::min(C.row_of[k + 1u], C.c1) > std::max(C.row_of[k], C.c0);
    if (!C.has_table) {  // 5
        REQUIRE(D.copies.size() == bands_with_rows && n_whole == D.copies.size(), "%zu copies, %zu whole-width, for %zu bands with rows", D.copies.size(), n_whole, bands_with_rows);
        REQUIRE(D.host_bytes == outside_px * 4u, "the host writes %llu bytes", (unsigned long long)D.host_bytes);
        T.no_table++;
    } else {  // 6
        const DownloadPlan D0 = C.plan(0);
        const uint64_t trimmed_px = trimmed_by_rows(C);
        REQUIRE(D0.host_bytes / 4u - outside_px == trimmed_px, "min_tiles 0: the host writes %llu pixels inside the content rows, by rows %llu", (unsigned long long)(D0.host_bytes / 4u - outside_px), (unsigned long long)trimmed_px);
        bool any_strided = false, any_filled_strip = false, any_nine_tenths = false;
        if (trimmed_px < C.min_tiles * (uint64_t)(TILE * TILE)) {
            REQUIRE(D.copies.size() == bands_with_rows && n_whole == D.copies.size(), "fallback: %zu copies, %zu whole-width, %zu bands with rows", D.copies.size(), n_whole, bands_with_rows);
            REQUIRE(D.host_bytes == outside_px * 4u, "fallback: the host writes %llu bytes", (unsigned long long)D.host_bytes);
            for (const DownloadRect &f : D.fills) REQUIRE(empty(f) || f.r1 <= C.c0 || f.r0 >= C.c1, "fallback: a fill in the content rows [%u, %u)", f.r0, f.r1);
            T.fallback += trimmed_px != 0u;
        } else {
            REQUIRE(D.copies.size() == D0.copies.size() && D.fills.size() == D0.fills.size() && D.link_bytes == D0.link_bytes, "not the plan of min_tiles 0");
            for (size_t i = 0; i < D.copies.size(); ++i) REQUIRE(!memcmp(&D.copies[i], &D0.copies[i], sizeof(DownloadRect)), "copy %zu is not that of min_tiles 0", i);
            for (const DownloadRect &c : D.copies) {
                uint32_t lo = 0xFFFFFFFFu, hi = 0u;
                for (uint32_t t = c.r0 / TILE; t < (c.r1 + TILE - 1u) / TILE; ++t)
                    if (C.table[2u * t] < C.table[2u * t + 1u]) {
                        lo = std::min(lo, C.table[2u * t]);
                        hi = std::max(hi, C.table[2u * t + 1u]);
                    }
                REQUIRE(lo < hi, "a copy of rows [%u, %u) without a span", c.r0, c.r1);
                const uint32_t x0 = std::min(lo * TILE, W), x1 = std::min(hi * TILE, W);
                if (c.x0 == 0u && c.x1 == W) {
                    if (x0 != 0u || x1 != W) {
                        REQUIRE((uint64_t)(x1 - x0) * 10u >= (uint64_t)W * 9u, "columns [%u, %u) of %u travel whole", x0, x1, W);
                        any_nine_tenths = true;
                    }
                } else {
                    REQUIRE(c.x0 == x0 && c.x1 == x1 && (uint64_t)(x1 - x0) * 10u < (uint64_t)W * 9u, "strided copy of columns [%u, %u), spans [%u, %u)", c.x0, c.x1, x0, x1);
                    any_strided = true;
                }
            }
            for (const DownloadRect &f : D.fills) any_filled_strip = any_filled_strip || (!empty(f) && f.x0 == 0u && f.x1 == W && f.r0 >= C.c0 && f.r1 <= C.c1);
        }
        T.strided += any_strided;
        T.filled_strips += any_filled_strip;
        T.nine_tenths += any_nine_tenths;
    }
    T.cases++;
    T.clipped += C.clipped;
    T.copies += D.copies.size();
    T.fills += D.fills.size();
    return true;
}

static void describe(const Case &C) {
    fprintf(stderr, "  %ux%u, content rows [%u, %u)%s, row_of {%u, %u, %u, %u, %u}, min_tiles %zu, table:", C.W, C.H, C.c0, C.c1, C.clipped ? " (clipped)" : "", C.row_of[0], C.row_of[1],
            C.row_of[2], C.row_of[3], C.row_of[4], C.min_tiles);
    if (!C.has_table) fprintf(stderr, " none");
    else
        for (uint32_t t = 0; t < C.n_tab(); ++t) fprintf(stderr, " [%u, %u)", C.table[2u * t], C.table[2u * t + 1u]);
    fprintf(stderr, "\n");
}

static int fuzz(uint64_t seed, unsigned long cases) {
    Rng R(seed);
    Tally T;
    for (unsigned long c = 0; c < cases; ++c) {
        const Case C = draw(R);
        if (!check_case(C, T)) {
            describe(C);
            return 1;
        }
    }
    printf("cases %lu strided %lu filled_strips %lu fallback %lu nine_tenths %lu no_table %lu clipped %lu copies %lu fills %lu\n", T.cases, T.strided, T.filled_strips, T.fallback,
           T.nine_tenths, T.no_table, T.clipped, T.copies, T.fills);
    return 0;
}

static bool same(const DownloadRect &a, const DownloadRect &b) { return a.r0 == b.r0 && a.r1 == b.r1 && a.x0 == b.x0 && a.x1 == b.x1; }

static bool known_cases() {
    // 160x128, eight tile rows with the span [2, 5): every band of two tile rows travels as two strips of the columns [32, 80)
    Case C;
    C.W = 160; C.H = 128; C.c0 = 0; C.c1 = 128;
    const uint32_t row_of[5] = {0, 32, 64, 96, 128};
    memcpy(C.row_of, row_of, sizeof(row_of));
    C.has_table = true;
    for (int t = 0; t < 8; ++t) { C.table.push_back(2u); C.table.push_back(5u); }
    Tally T;
    if (!check_case(C, T)) return false;
    const DownloadPlan D = C.plan(0);
    REQUIRE(D.copies.size() == 8u && D.fills.size() == 16u, "%zu copies, %zu fills", D.copies.size(), D.fills.size());
    for (uint32_t k = 0; k < 8u; ++k) {
        REQUIRE(same(D.copies[k], DownloadRect{16u * k, 16u * k + 16u, 32u, 80u}), "copy %u", k);
        REQUIRE(same(D.fills[2u * k], DownloadRect{16u * k, 16u * k + 16u, 0u, 32u}) && same(D.fills[2u * k + 1u], DownloadRect{16u * k, 16u * k + 16u, 80u, 160u}), "side fills of copy %u", k);
    }
    REQUIRE(D.link_bytes == 24576u && D.host_bytes == 57344u, "%llu bytes over the link, %llu by the host", (unsigned long long)D.link_bytes, (unsigned long long)D.host_bytes);
    // a frame whose content rows are empty (c0 == c1): nothing travels, two fills cover everything -- with a table and without
    for (int with_table = 0; with_table < 2; ++with_table) {
        Case E;
        E.W = 100; E.H = 70; E.c0 = E.c1 = 32; E.clipped = true;
        bands_of(E);
        REQUIRE(E.row_of[0] == 0u && E.row_of[1] == 32u && E.row_of[3] == 32u && E.row_of[4] == 70u, "row_of of a frame without content");
        E.has_table = with_table != 0;
        E.table.assign(2u * 5u, 0u);
        if (!check_case(E, T)) return false;
        const DownloadPlan F = E.plan(0);
        REQUIRE(F.copies.empty() && F.fills.size() == 2u && same(F.fills[0], DownloadRect{0u, 32u, 0u, 100u}) && same(F.fills[1], DownloadRect{32u, 70u, 0u, 100u}), "%zu copies, %zu fills", F.copies.size(), F.fills.size());
        REQUIRE(F.link_bytes == 0u && F.host_bytes == 100u * 70u * 4u, "%llu bytes by the host", (unsigned long long)F.host_bytes);
    }
    // the content rows of a handed-back table: tile rows 2 and 4 of seven hold something
    uint32_t back[14] = {0, 0, 9, 0, 3, 4, 0, 0, 1, 2, 0, 0, 0, 0}, c0 = 7u, c1 = 9u;
    REQUIRE(rxr_table_content_rows(back, 100u, 10u, 0, c0, c1) && c0 == 32u && c1 == 80u, "content rows [%u, %u)", c0, c1);
    c0 = 7u; c1 = 9u;  // (32 + 20 rows outside: three tile rows of ten tiles saved)
    REQUIRE(rxr_table_content_rows(back, 100u, 10u, 30, c0, c1) && !rxr_table_content_rows(back, 100u, 10u, 31, c0, c1) && c0 == 32u && c1 == 80u, "the min_tiles test");
    uint32_t none[4] = {0, 0, 5, 5};
    REQUIRE(rxr_table_content_rows(none, 20u, 3u, 0, c0, c1) && c0 == 0u && c1 == 0u, "an empty table: rows [%u, %u)", c0, c1);
    return true;
}

static bool fill_writer() {
    const uint32_t W = 37u, H = 29u;
    const std::vector<DownloadRect> fills = {{0u, 5u, 0u, W}, {5u, 5u, 0u, W}, {7u, 19u, 0u, 3u}, {7u, 19u, 30u, W}, {19u, 21u, 4u, 4u}, {22u, 20u, 0u, W}, {28u, H, 1u, 36u}};
    std::vector<uint8_t> want((size_t)W * H, 0);
    for (const DownloadRect &f : fills)
        for (uint32_t y = f.r0; y < f.r1; ++y)
            for (uint32_t x = f.x0; x < f.x1; ++x) want[(size_t)y * W + x] = 1;
    std::vector<uint32_t> store((size_t)W * H + 4u);
    for (uint32_t shift = 0; shift < 2u; ++shift)
        for (uint32_t of : {1u, 4u, 8u}) {
            memset(store.data(), 0xA5, store.size() * 4u);
            uint8_t *const base = (uint8_t *)store.data(), *const pixels = base + 4u + shift;  // (shift 1: unaligned)
            for (uint32_t me = 0; me < of; ++me) rxr_write_fills(pixels, W, fills, me, of);
            for (size_t i = 0; i < store.size() * 4u; ++i) {
                const ptrdiff_t at = (ptrdiff_t)i - (ptrdiff_t)(4u + shift);
                const bool filled = at >= 0 && (size_t)at < (size_t)W * H * 4u && want[(size_t)at / 4u];
                const uint8_t expect = !filled ? 0xA5 : ((size_t)at % 4u == 3u ? 0xFF : 0x00);
                REQUIRE(base[i] == expect, "byte %td of the frame (buffer at +%u, %u workers) is %02X, not %02X", at, shift, of, base[i], expect);
            }
        }
    return true;
}

int main(int argc, char **argv) {
    if (argc == 4 && !strcmp(argv[1], "fuzz")) return fuzz(strtoull(argv[2], nullptr, 10), strtoul(argv[3], nullptr, 10));
    if (argc == 2 && !strcmp(argv[1], "known")) return known_cases() ? (printf("ok\n"), 0) : 1;
    if (argc == 2 && !strcmp(argv[1], "fills")) return fill_writer() ? (printf("ok\n"), 0) : 1;
    fprintf(stderr, "usage: download_plan_main fuzz SEED CASES | download_plan_main known | download_plan_main fills\n");
    return 2;
}
