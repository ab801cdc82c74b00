// d3_rows_main.cpp -- the tile rows a triangle can reach (rxr_tri_tile_rows, rusterix_amd/csrc/rxr_device.h: what rxr_upload_frame asks of
// a small frame's set-up records, and what lets the raster kernel skip the 3D passes of whole tile rows) as a program of its own.
// Built with a host compiler (-O2 -ffp-contract=off), and once more with -fsanitize=address,undefined; tests/test_d3_rows_cpu.py runs both.
//
//   d3_rows_main fuzz SEED CASES      seeded triangles at 16x16, 48x64 and 333x187, seven kinds (below); checks, per record,
//                                       (1) every pixel centre that passes the pixel box and the three !(r < 0) tests -- visit()'s float
//                                           expressions, by brute force over the box -- lies in a tile row inside the range, and
//                                       (2) the binary search returns the range of the linear scan over all tile rows,
//                                       and (3) that the union rxr_upload_frame accumulates is the union of the records' ranges;
//                                     prints one line of counts; exit status 1 with the first offending record on a miss
//   d3_rows_main time FILE WIDTH REPS the union range of the TriSetup records in FILE (96 bytes each), and the nanoseconds one pass takes
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../rusterix_amd/csrc/rxr_device.h"

static const uint32_t TILE = 16u;  // RXR_TILE_H

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
    float uni() { return (float)(next() >> 40) / 16777216.0f; }  // [0, 1)
    float range(float a, float b) { return a + (b - a) * uni(); }
    uint32_t below(uint32_t n) { return (uint32_t)(next() >> 33) % n; }
};

// the record rxr_tri_records makes of three projected vertices (cull mode off: every winding is drawn), band [0, height)
static TriSetup record_of(const float v[3][2], uint32_t width, uint32_t height) {
    TriRecordIn in{};
    for (int k = 0; k < 3; ++k) {
        in.v[k][0] = v[k][0];
        in.v[k][1] = v[k][1];
        in.v[k][2] = 0.5f;
        in.v[k][3] = 1.0f;
    }
    in.E = edges_from_xy(RXR_CULL_OFF, true, v[0][0], v[0][1], v[1][0], v[1][1], v[2][0], v[2][1]);
    in.tex = -1;
    in.width = width;
    in.row0 = 0u;
    in.row1 = height;
    TriSetup S{};
    TriShade H{};
    rxr_tri_records(in, S, H);
    return S;
}

// the range by a scan of every tile row: a row is in when the pixel box meets it and the tile reject, asked of the row, does not fire
static void rows_by_scan(const TriSetup &S, uint32_t width, uint32_t height, uint32_t &t0, uint32_t &t1) {
    t0 = t1 = 0u;
    const uint32_t min_x = S.bx & 0xFFFFu, max_x = S.bx >> 16, min_y = S.by & 0xFFFFu, max_y = S.by >> 16;
    if (!(min_x < max_x && min_y < max_y)) return;
    const uint32_t n_rows = (std::max(height, max_y) + TILE - 1u) / TILE;
    bool any = false;
    for (uint32_t r = 0; r < n_rows; ++r) {
        if (min_y >= (r + 1u) * TILE || max_y <= r * TILE) continue;
        if (rxr_rect_outside_edges(S.ea, S.eb, S.ec, 0u, r * TILE, width, TILE)) continue;
        if (!any) t0 = r;
        any = true;
        t1 = r + 1u;
    }
}

struct Tally {
    unsigned long records = 0, with_rows = 0, empty = 0, pixels = 0, narrowed = 0;
};

static bool check(const TriSetup &S, uint32_t width, uint32_t height, const char *kind, Tally &T) {
    uint32_t t0, t1, s0, s1;
    rxr_tri_tile_rows(S, width, TILE, t0, t1);
    rows_by_scan(S, width, height, s0, s1);
    bool ok = t0 == s0 && t1 == s1;
    const uint32_t min_x = S.bx & 0xFFFFu, max_x = S.bx >> 16, min_y = S.by & 0xFFFFu, max_y = S.by >> 16;
    unsigned long px_in = 0;
    uint32_t bad_x = 0, bad_y = 0;
    bool stray = false;
    for (uint32_t py = min_y; py < max_y && !stray; ++py) {
        const float fy = (float)py + 0.5f;
        for (uint32_t px = min_x; px < max_x; ++px) {
            const float fx = (float)px + 0.5f;
            const float r0 = S.ea[0] * fx + S.eb[0] * fy + S.ec[0];
            const float r1 = S.ea[1] * fx + S.eb[1] * fy + S.ec[1];
            const float r2 = S.ea[2] * fx + S.eb[2] * fy + S.ec[2];
            if (!(r0 < 0.0f) && !(r1 < 0.0f) && !(r2 < 0.0f)) {
                ++px_in;
                const uint32_t row = py / TILE;
                if (!(row >= t0 && row < t1)) {
                    stray = true;
                    bad_x = px;
                    bad_y = py;
                    break;
                }
            }
        }
    }
    ok = ok && !stray;
    T.records++;
    T.pixels += px_in;
    if (t0 < t1) T.with_rows++;
    else T.empty++;
    if (min_y < max_y && t1 - t0 < (max_y + TILE - 1u) / TILE - min_y / TILE) T.narrowed++;
    if (!ok) {
        fprintf(stderr, "d3_rows_main: %s record at %ux%u: search [%u, %u), scan [%u, %u)%s\n", kind, width, height, t0, t1, s0, s1,
                stray ? ", a covered pixel outside the range" : "");
        if (stray) fprintf(stderr, "  pixel (%u, %u)\n", bad_x, bad_y);
        fprintf(stderr, "  box x [%u, %u) y [%u, %u)\n", min_x, max_x, min_y, max_y);
        for (int i = 0; i < 3; ++i) fprintf(stderr, "  edge %d: a %.9g b %.9g c %.9g\n", i, S.ea[i], S.eb[i], S.ec[i]);
    }
    return ok;
}

static int fuzz(uint64_t seed, unsigned long cases) {
    static const uint32_t sizes[3][2] = {{16, 16}, {48, 64}, {333, 187}};
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float specials[] = {nan, inf, -inf};
    Rng R(seed);
    Tally T;
    unsigned long by_kind[7] = {0, 0, 0, 0, 0, 0, 0};
    uint32_t uni[3][4] = {{0xFFFFFFFFu, 0u, 0xFFFFFFFFu, 0u}, {0xFFFFFFFFu, 0u, 0xFFFFFFFFu, 0u}, {0xFFFFFFFFu, 0u, 0xFFFFFFFFu, 0u}};
    for (unsigned long c = 0; c < cases; ++c) {
        const uint32_t *sz = sizes[c % 3u];
        const uint32_t W = sz[0], H = sz[1];
        const float fw = (float)W, fh = (float)H;
        const unsigned kind = (unsigned)((c / 3u) % 7u);
        by_kind[kind]++;
        float v[3][2];
        TriSetup S{};
        const char *name = "";
        switch (kind) {
        case 0:  // ordinary triangles, in and around the frame
            name = "ordinary";
            for (int k = 0; k < 3; ++k) {
                v[k][0] = R.range(-0.3f * fw, 1.3f * fw);
                v[k][1] = R.range(-0.3f * fh, 1.3f * fh);
            }
            S = record_of(v, W, H);
            break;
        case 1: {  // slivers: two vertices far apart, the third a fraction of a pixel off their line
            name = "sliver";
            v[0][0] = R.range(-0.2f * fw, 1.2f * fw);
            v[0][1] = R.range(-0.2f * fh, 1.2f * fh);
            v[1][0] = R.range(-0.2f * fw, 1.2f * fw);
            v[1][1] = R.range(-0.2f * fh, 1.2f * fh);
            const float t = R.uni();
            v[2][0] = v[0][0] + t * (v[1][0] - v[0][0]) + R.range(-0.7f, 0.7f);
            v[2][1] = v[0][1] + t * (v[1][1] - v[0][1]) + R.range(-0.7f, 0.7f);
            S = record_of(v, W, H);
            break;
        }
        case 2: {  // far larger than the frame: vertices, and with them the coefficients, up to 1e30 (c: products of two coordinates)
            name = "huge";
            const float mag = powf(10.0f, R.range(3.0f, 15.0f));
            for (int k = 0; k < 3; ++k) {
                v[k][0] = R.range(-mag, mag) + 0.5f * fw;
                v[k][1] = R.range(-mag, mag) + 0.5f * fh;
            }
            S = record_of(v, W, H);
            const float scale = powf(10.0f, R.range(0.0f, 30.0f - 2.0f * log10f(mag)));  // (one positive factor for a, b and c: the same triangle)
            if (R.below(2u)) {
                for (int i = 0; i < 3; ++i) {
                    S.ea[i] *= scale;
                    S.eb[i] *= scale;
                    S.ec[i] *= scale;
                }
            }
            break;
        }
        case 3: {  // the wall case: a quad half clipped at the near plane -- edges that cross the frame, a box clamped to the full height
            name = "wall";
            const float xa = R.range(-2.0f * fw, 3.0f * fw), xb = R.range(-2.0f * fw, 3.0f * fw);
            const float top_a = R.range(-0.2f * fh, 0.9f * fh), top_b = R.range(-0.2f * fh, 0.9f * fh);
            v[0][0] = xa; v[0][1] = top_a;
            v[1][0] = xb; v[1][1] = top_b;
            v[2][0] = R.below(2u) ? xa : xb; v[2][1] = R.range(50.0f * fh, 5000.0f * fh);
            if (R.below(4u) == 0u) v[R.below(2u)][1] = -R.range(50.0f * fh, 5000.0f * fh);
            S = record_of(v, W, H);
            break;
        }
        case 4:  // zero area (three points of one line, or one point three times) and all-zero records
            name = "degenerate";
            if (R.below(3u) == 0u) break;  // (S stays all-zero)
            v[0][0] = R.range(0.0f, fw);
            v[0][1] = R.range(0.0f, fh);
            if (R.below(2u)) {
                v[1][0] = v[2][0] = v[0][0];
                v[1][1] = v[2][1] = v[0][1];
            } else {
                const float dx = R.range(-fw, fw), dy = R.range(-fh, fh);
                v[1][0] = v[0][0] + dx; v[1][1] = v[0][1] + dy;
                v[2][0] = v[0][0] + 2.0f * dx; v[2][1] = v[0][1] + 2.0f * dy;
            }
            S = record_of(v, W, H);
            break;
        case 5: {  // NaN and +-inf in each coefficient of an ordinary record, one at a time (27 combinations, each at every frame size)
            name = "special";
            for (int k = 0; k < 3; ++k) {
                v[k][0] = R.range(-0.3f * fw, 1.3f * fw);
                v[k][1] = R.range(-0.3f * fh, 1.3f * fh);
            }
            S = record_of(v, W, H);
            if (!(S.bx | S.by)) {  // (off screen: give it the whole frame, the coefficients are what is tested)
                S.bx = W << 16;
                S.by = H << 16;
            }
            const unsigned long n = (by_kind[5] - 1u) / 3u;  // (the same combination at each of the three frame sizes)
            float *coef[3] = {S.ea, S.eb, S.ec};
            coef[(n / 3u) % 3u][n % 3u] = specials[(n / 9u) % 3u];
            break;
        }
        default: {  // several specials and huge coefficients at once, full-height boxes
            name = "mixed";
            for (int i = 0; i < 3; ++i) {
                float *coef[3] = {S.ea, S.eb, S.ec};
                for (int j = 0; j < 3; ++j) {
                    const uint32_t pick = R.below(8u);
                    const float mag = powf(10.0f, R.range(-3.0f, 38.0f));
                    coef[j][i] = pick < 3u ? specials[pick] : (pick == 3u ? 0.0f : (pick == 4u ? -0.0f : (R.below(2u) ? mag : -mag)));
                }
            }
            S.bx = W << 16;
            S.by = R.below(2u) ? (H << 16) : (R.below(H) | (H << 16));
            if ((S.by & 0xFFFFu) >= (S.by >> 16)) S.by = H << 16;
            break;
        }
        }
        if (!check(S, W, H, name, T)) return 1;
        // (3) the union as rxr_upload_frame accumulates it (rxr_union_tile_rows skips a record whose box rows it already holds) is the
        // union of the records' own ranges; a new union every 5 records of a frame size, so that small ones are seen too
        uint32_t *u = uni[c % 3u];
        if ((c / 3u) % 5u == 0u) {
            u[0] = u[2] = 0xFFFFFFFFu;
            u[1] = u[3] = 0u;
        }
        uint32_t t0, t1;
        rxr_tri_tile_rows(S, W, TILE, t0, t1);
        if (t0 < t1) {
            u[2] = std::min(u[2], t0);
            u[3] = std::max(u[3], t1);
        }
        rxr_union_tile_rows(S, W, TILE, u[0], u[1]);
        if (u[0] != u[2] || u[1] != u[3]) {
            fprintf(stderr, "d3_rows_main: %s record at %ux%u: union [%u, %u), union of the ranges [%u, %u)\n", name, W, H, u[0], u[1], u[2], u[3]);
            return 1;
        }
    }
    printf("records %lu with_rows %lu empty %lu narrowed_by_edges %lu covered_pixels %lu\n", T.records, T.with_rows, T.empty, T.narrowed, T.pixels);
    return 0;
}

static int time_file(const char *path, uint32_t width, unsigned long reps) {
    FILE *f = fopen(path, "rb");
    if (!f) return 2;
    std::vector<TriSetup> recs;
    TriSetup S;
    while (fread(&S, sizeof(S), 1, f) == 1) recs.push_back(S);
    fclose(f);
    uint32_t r0 = 0xFFFFFFFFu, r1 = 0u;
    volatile uint32_t sink = 0;
    const auto a = std::chrono::steady_clock::now();
    for (unsigned long k = 0; k < reps; ++k) {
        r0 = 0xFFFFFFFFu;
        r1 = 0u;
        for (const TriSetup &T : recs) rxr_union_tile_rows(T, width, TILE, r0, r1);  // (the loop of rxr_upload_frame)
        sink = sink + r0 + r1;
    }
    const auto b = std::chrono::steady_clock::now();
    const double ns = std::chrono::duration<double, std::nano>(b - a).count() / (double)(reps ? reps : 1);
    if (!(r0 < r1)) r0 = r1 = 0u;
    printf("records %zu range %u %u ns_per_pass %.1f\n", recs.size(), r0, r1, ns);
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 4 && !strcmp(argv[1], "fuzz")) return fuzz(strtoull(argv[2], nullptr, 10), strtoul(argv[3], nullptr, 10));
    if (argc == 5 && !strcmp(argv[1], "time")) return time_file(argv[2], (uint32_t)strtoul(argv[3], nullptr, 10), strtoul(argv[4], nullptr, 10));
    fprintf(stderr, "usage: d3_rows_main fuzz SEED CASES | d3_rows_main time FILE WIDTH REPS\n");
    return 2;
}
