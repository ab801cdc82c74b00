// A stand-alone program over the host half of rxr_set_terrain_flatten (rusterix_amd/csrc/rxr_terrain_flatten_records.h: what the call
// refuses, and the device records it builds), built with -fsanitize=address,undefined and run as a child process by
// tests/test_terrain_flatten_cpu.py.  The arrays are heap blocks of exactly the size the counts name, so a read past a malformed
// range is a report: ranges that end one past the pool, wrap around 2^32 or start behind it, NULL arrays, counts above the bounds,
// then lists the check accepts -- overlapping and empty ranges, a range at the pool's end, NaN and infinite geometry, saturating
// casts -- through `build`, with the blob's sum printed so that nothing is optimised away.  It touches no device.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "../rusterix_amd/csrc/rxr_terrain_flatten_records.h"

namespace {
struct List {
    std::vector<uint32_t> kinds, ranges;
    std::vector<float> params, records;
    void op(uint32_t kind, float bevel, float floor, uint32_t first, uint32_t count, float x0 = 0.0f, float y0 = 0.0f, float x1 = 1.0f, float y1 = 1.0f) {
        kinds.push_back(kind);
        const float p[RXR_TERRAIN_FLATTEN_OP_FLOATS] = {bevel, floor, x0, y0, x1, y1};
        params.insert(params.end(), p, p + RXR_TERRAIN_FLATTEN_OP_FLOATS);
        ranges.push_back(first), ranges.push_back(count);
    }
    void record(float x0, float y0, float x1, float y1, float h0 = 0.0f, float h1 = 0.0f) {
        const float r[RXR_TERRAIN_FLATTEN_RECORD_FLOATS] = {x0, y0, x1, y1, h0, h1, std::fmin(x0, x1), std::fmin(y0, y1), std::fmax(x0, x1), std::fmax(y0, y1)};
        records.insert(records.end(), r, r + RXR_TERRAIN_FLATTEN_RECORD_FLOATS);
    }
    uint32_t n_ops() const { return (uint32_t)kinds.size(); }
    uint32_t n_records() const { return (uint32_t)(records.size() / RXR_TERRAIN_FLATTEN_RECORD_FLOATS); }
    int check(uint32_t *slots, uint32_t *seg_slots, std::string &err) const {
        return rxflat::check(kinds.data(), params.data(), ranges.data(), n_ops(), records.empty() ? nullptr : records.data(), n_records(), slots, seg_slots, err);
    }
};
}  // namespace

int main() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    std::string err;
    uint32_t slots = 0, seg_slots = 0;

    // ---- refused: nothing past a malformed range may be read ----
    const uint32_t bad_ranges[][2] = {{0, 4}, {3, 1}, {4, 1}, {0xFFFFFFFFu, 2}, {2, 0xFFFFFFFFu}, {0x80000000u, 0x80000000u}};
    for (const auto &r : bad_ranges) {
        List l;
        for (int i = 0; i < 3; ++i) l.record((float)i, 0.0f, (float)i + 1.0f, 1.0f);
        l.op(RXR_TERRAIN_FLATTEN_SECTOR, 0.5f, 0.0f, 0, 3);
        l.op(RXR_TERRAIN_FLATTEN_LINEDEFS, 0.5f, 0.0f, r[0], r[1]);
        if (l.check(&slots, &seg_slots, err) != RXR_ERR_INVALID) return 1;
    }
    {
        List l;
        l.record(0, 0, 1, 1);
        l.op(7u, 0.5f, 0.0f, 0, 1);
        if (l.check(nullptr, nullptr, err) != RXR_ERR_INVALID) return 2;
        l.kinds[0] = RXR_TERRAIN_FLATTEN_SECTOR;
        if (rxflat::check(nullptr, l.params.data(), l.ranges.data(), 1, l.records.data(), 1, nullptr, nullptr, err) != RXR_ERR_INVALID) return 3;
        if (rxflat::check(l.kinds.data(), nullptr, l.ranges.data(), 1, l.records.data(), 1, nullptr, nullptr, err) != RXR_ERR_INVALID) return 3;
        if (rxflat::check(l.kinds.data(), l.params.data(), nullptr, 1, l.records.data(), 1, nullptr, nullptr, err) != RXR_ERR_INVALID) return 3;
        if (rxflat::check(l.kinds.data(), l.params.data(), l.ranges.data(), 1, nullptr, 1, nullptr, nullptr, err) != RXR_ERR_INVALID) return 3;
        // counts above the bounds are refused before an array is looked at
        if (rxflat::check(nullptr, nullptr, nullptr, RXR_TERRAIN_FLATTEN_MAX_OPS + 1u, nullptr, 0, nullptr, nullptr, err) != RXR_ERR_UNSUPPORTED) return 4;
        if (rxflat::check(nullptr, nullptr, nullptr, 0, nullptr, RXR_TERRAIN_FLATTEN_MAX_RECORDS + 1u, nullptr, nullptr, err) != RXR_ERR_UNSUPPORTED) return 4;
    }
    {   // the ranges' sum above the bound: two ops over the whole of a full pool
        List l;
        for (uint32_t i = 0; i < RXR_TERRAIN_FLATTEN_MAX_RECORDS; ++i) l.record((float)i, 0.0f, (float)i + 1.0f, 0.0f);
        l.op(RXR_TERRAIN_FLATTEN_SECTOR, 0.5f, 0.0f, 0, RXR_TERRAIN_FLATTEN_MAX_RECORDS);
        if (l.check(&slots, &seg_slots, err) != RXR_OK || slots != RXR_TERRAIN_FLATTEN_MAX_RECORDS || seg_slots != 0) return 5;
        size_t at = 0;
        const std::vector<float> blob = rxflat::build(l.kinds.data(), l.params.data(), l.ranges.data(), l.n_ops(), l.records.data(), slots, &at);
        if (blob.size() != (size_t)(FLATTEN_OP_WORDS + slots * FLATTEN_RECORD_WORDS) * 4 || at != FLATTEN_OP_WORDS * 16) return 5;
        l.op(RXR_TERRAIN_FLATTEN_LINEDEFS, 0.5f, 0.0f, 0, 1);
        if (l.check(&slots, &seg_slots, err) != RXR_ERR_UNSUPPORTED) return 5;
        // ... and the linedef ops' share above its own
        l.kinds[0] = RXR_TERRAIN_FLATTEN_LINEDEFS, l.ranges[1] = RXR_TERRAIN_FLATTEN_MAX_SEGMENTS, l.ranges[3] = 0;
        if (l.check(&slots, &seg_slots, err) != RXR_OK || seg_slots != RXR_TERRAIN_FLATTEN_MAX_SEGMENTS) return 5;
        l.ranges[3] = 1;
        if (l.check(&slots, &seg_slots, err) != RXR_ERR_UNSUPPORTED) return 5;
    }

    // ---- accepted: built ----
    List l;
    l.record(0.0f, 0.0f, 4.0f, 0.0f);
    l.record(4.0f, 0.0f, 4.0f, 4.0f);
    l.record(4.0f, 4.0f, 0.0f, 0.0f);
    l.record(1.0f, 1.0f, 9.0f, 2.0f, 1.0f, 2.0f);
    l.record(nan, -inf, inf, 3.0e38f, nan, inf);
    l.op(RXR_TERRAIN_FLATTEN_SECTOR, 1.0f, 2.0f, 0, 3, 0.0f, 0.0f, 4.0f, 4.0f);
    l.op(RXR_TERRAIN_FLATTEN_SECTOR, 0.25f, 2.0f, 0, 3, 0.0f, 0.0f, 4.0f, 4.0f);       // the same range again (a second Flatten node)
    l.op(RXR_TERRAIN_FLATTEN_SECTOR, 0.5f, 0.0f, 1, 2);                                // a sector of two edges, overlapping
    l.op(RXR_TERRAIN_FLATTEN_SECTOR, inf, nan, 5, 0, nan, -inf, inf, 3.0e38f);         // an empty range at the pool's end; the casts saturate
    l.op(RXR_TERRAIN_FLATTEN_SECTOR, -3.0e38f, 0.0f, 0, 1, -3.0e38f, -3.0e38f, 3.0e38f, 3.0e38f);
    l.op(RXR_TERRAIN_FLATTEN_LINEDEFS, 1.5f, 0.0f, 3, 2);
    l.op(RXR_TERRAIN_FLATTEN_LINEDEFS, 0.0f, 0.0f, 4, 1);
    if (l.check(&slots, &seg_slots, err) != RXR_OK) return 6;
    if (slots != 3 + 3 + 2 + 0 + 1 + 2 + 1 || seg_slots != 3) return 6;
    size_t at = 0;
    const std::vector<float> blob = rxflat::build(l.kinds.data(), l.params.data(), l.ranges.data(), l.n_ops(), l.records.data(), slots, &at);
    if (blob.size() != ((size_t)l.n_ops() * FLATTEN_OP_WORDS + (size_t)slots * FLATTEN_RECORD_WORDS) * 4) return 7;
    // the first op: bevel * 4, bevel * 0.5, the box moved by 1, the integer ranges of the box moved by bevel / 2
    int32_t rg[4];
    memcpy(rg, blob.data() + 8, sizeof rg);
    if (blob[2] != 4.0f || blob[3] != 0.5f || blob[4] != -1.0f || blob[6] != 5.0f || rg[0] != -1 || rg[1] != 5 || rg[2] != -1 || rg[3] != 5) return 8;
    // its first edge's previous vertex is the third edge's start point (4, 4): pj - pi = (4, 4), pj.y = 4
    const float *e0 = blob.data() + at / 4;
    if (e0[2] != 4.0f || e0[3] != 0.0f || e0[4] != 16.0f || e0[5] != 4.0f || e0[6] != 4.0f || e0[7] != 4.0f) return 9;
    // the fourth op's ranges: NaN gives 0, the infinities saturate
    memcpy(rg, blob.data() + 3 * FLATTEN_OP_WORDS * 4 + 8, sizeof rg);
    if (rg[0] != 0 || rg[1] != INT32_MAX || rg[2] != INT32_MIN || rg[3] != INT32_MAX) return 10;
    double sum = 0.0;
    for (float v : blob)
        if (v == v && std::fabs(v) < 1.0e30f) sum += v;
    std::printf("terrain flatten records under sanitizers: clean (checksum %.6f)\n", sum);
    return 0;
}
