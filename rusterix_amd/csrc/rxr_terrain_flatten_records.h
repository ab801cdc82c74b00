// rxr_terrain_flatten_records.h -- the host half of rxr_set_terrain_flatten (rxr_terrain_flatten.hip): what the call refuses and the
// device records it builds from the caller's op list.  Plain C++ without a HIP header, so that tests/terrain_flatten_asan_main.cpp
// drives it under the sanitizers on the CPU.  Everything here that is arithmetic is the reference's own f32 operation on the same
// operands (the build's -ffp-contract=off): computing it once per registration instead of once per cell gives the same bits.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/rxr.h"

// device records, in 16-byte words (float4)
#define FLATTEN_OP_WORDS 4u       // bevel, floor_height, bevel * 4.0, bevel * 0.5 | the sector's box.expanded(2.0): min x, min y, max x, max y
                                  // | the sector's integer ranges: min_x, max_x, min_y, max_y (i32 bits) | first device record, records, kind, 0 (u32 bits)
#define FLATTEN_RECORD_WORDS 3u   // sector edge:  v0.x, v0.y, edge.x, edge.y | dot(edge, edge), pj.x - pi.x, pj.y - pi.y, pj.y | 0
                                  // segment:      a.x, a.y, ab.x, ab.y | dot(ab, ab), height_start, height_end, 0 | its box.expanded(2.0)

namespace rxflat {

// Rust's `x as i32`: saturating, NaN -> 0
inline int32_t as_i32(float x) {
    if (x != x) return 0;
    if (x >= 2147483648.0f) return INT32_MAX;
    if (x <= -2147483648.0f) return INT32_MIN;
    return (int32_t)x;
}

inline float bits_f(uint32_t u) {
    float f;
    memcpy(&f, &u, 4);
    return f;
}

// RXR_OK, or the refusal and in `err` its reason; *slots: the sum of the range lengths, *seg_slots: of the linedef ops' alone
inline int check(const uint32_t *kinds, const float *params, const uint32_t *ranges, uint32_t n_ops, const float *records, uint32_t n_records, uint32_t *slots,
                 uint32_t *seg_slots, std::string &err) {
    auto bad = [&](int code, const std::string &m) {
        err = m;
        return code;
    };
    if (n_ops > RXR_TERRAIN_FLATTEN_MAX_OPS) return bad(RXR_ERR_UNSUPPORTED, std::to_string(n_ops) + " ops exceed RXR_TERRAIN_FLATTEN_MAX_OPS");
    if (n_records > RXR_TERRAIN_FLATTEN_MAX_RECORDS) return bad(RXR_ERR_UNSUPPORTED, std::to_string(n_records) + " records exceed RXR_TERRAIN_FLATTEN_MAX_RECORDS");
    if (n_ops && (!kinds || !params || !ranges)) return bad(RXR_ERR_INVALID, "NULL op array");
    if (n_records && !records) return bad(RXR_ERR_INVALID, "NULL records");
    uint64_t total = 0, segs = 0;
    for (uint32_t i = 0; i < n_ops; ++i) {
        const std::string oi = "op " + std::to_string(i);
        if (kinds[i] != RXR_TERRAIN_FLATTEN_SECTOR && kinds[i] != RXR_TERRAIN_FLATTEN_LINEDEFS)
            return bad(RXR_ERR_INVALID, oi + ": kind " + std::to_string(kinds[i]) + " is neither RXR_TERRAIN_FLATTEN_SECTOR nor RXR_TERRAIN_FLATTEN_LINEDEFS");
        const uint64_t first = ranges[2 * (size_t)i], count = ranges[2 * (size_t)i + 1];
        if (first > n_records || count > n_records - first)
            return bad(RXR_ERR_INVALID, oi + ": its range (" + std::to_string(first) + ", " + std::to_string(count) + ") does not lie inside the pool of " + std::to_string(n_records) + " records");
        total += count;
        if (kinds[i] == RXR_TERRAIN_FLATTEN_LINEDEFS) segs += count;
    }
    if (total > RXR_TERRAIN_FLATTEN_MAX_RECORDS)
        return bad(RXR_ERR_UNSUPPORTED, "the ops' ranges hold " + std::to_string(total) + " records in all, more than RXR_TERRAIN_FLATTEN_MAX_RECORDS");
    if (segs > RXR_TERRAIN_FLATTEN_MAX_SEGMENTS)
        return bad(RXR_ERR_UNSUPPORTED, "the linedef ops' ranges hold " + std::to_string(segs) + " segments in all, more than RXR_TERRAIN_FLATTEN_MAX_SEGMENTS");
    if (slots) *slots = (uint32_t)total;
    if (seg_slots) *seg_slots = (uint32_t)segs;
    return RXR_OK;
}

// the device blob of a list `check` accepted: n_ops * FLATTEN_OP_WORDS float4, then slots * FLATTEN_RECORD_WORDS float4 (op after op: the
// previous edge of is_inside depends on the op's range, and ranges may overlap).  *records_at: the byte offset of the second part
inline std::vector<float> build(const uint32_t *kinds, const float *params, const uint32_t *ranges, uint32_t n_ops, const float *records, uint32_t slots,
                                size_t *records_at) {
    const size_t op_floats = (size_t)n_ops * FLATTEN_OP_WORDS * 4, rec_floats = (size_t)slots * FLATTEN_RECORD_WORDS * 4;
    std::vector<float> blob(op_floats + rec_floats, 0.0f);
    if (records_at) *records_at = op_floats * sizeof(float);
    uint32_t at = 0;   // the op's first device record
    for (uint32_t i = 0; i < n_ops; ++i) {
        const float *p = params + RXR_TERRAIN_FLATTEN_OP_FLOATS * (size_t)i;
        const uint32_t first = ranges[2 * (size_t)i], count = ranges[2 * (size_t)i + 1];
        float *o = blob.data() + (size_t)i * FLATTEN_OP_WORDS * 4;
        const float bevel = p[0];
        o[0] = bevel, o[1] = p[1];
        o[2] = bevel * 4.0f;   // sd < bevel * 4.0
        o[3] = bevel * 0.5f;   // BBox::expand(Vec2::broadcast(bevel)): amount * 0.5
        o[12] = bits_f(at), o[13] = bits_f(count), o[14] = bits_f(kinds[i]);
        if (kinds[i] == RXR_TERRAIN_FLATTEN_SECTOR) {
            // bounding_box(map).expanded(Vec2::broadcast(2.0)): min - 2.0 * 0.5, max + 2.0 * 0.5
            o[4] = p[2] - 1.0f, o[5] = p[3] - 1.0f, o[6] = p[4] + 1.0f, o[7] = p[5] + 1.0f;
            // bounds.expand(bevel), then floor / ceil `as i32`
            const int32_t r[4] = {as_i32(std::floor(p[2] - o[3])), as_i32(std::ceil(p[4] + o[3])), as_i32(std::floor(p[3] - o[3])), as_i32(std::ceil(p[5] + o[3]))};
            memcpy(o + 8, r, sizeof r);
        }
        for (uint32_t k = 0; k < count; ++k) {
            const float *r = records + RXR_TERRAIN_FLATTEN_RECORD_FLOATS * (size_t)(first + k);
            float *d = blob.data() + op_floats + (size_t)(at + k) * FLATTEN_RECORD_WORDS * 4;
            const float ex = r[2] - r[0], ey = r[3] - r[1];   // v1 - v0
            d[0] = r[0], d[1] = r[1], d[2] = ex, d[3] = ey;
            d[4] = ex * ex + ey * ey;                          // edge.dot(edge)
            if (kinds[i] == RXR_TERRAIN_FLATTEN_SECTOR) {
                // is_inside: polygon[i] is this edge's start point, polygon[j] the previous edge's (the last one's for the first)
                const float *j = records + RXR_TERRAIN_FLATTEN_RECORD_FLOATS * (size_t)(first + (k ? k - 1 : count - 1));
                d[5] = j[0] - r[0], d[6] = j[1] - r[1], d[7] = j[1];
            } else {
                d[5] = r[4], d[6] = r[5];
                d[8] = r[6] - 1.0f, d[9] = r[7] - 1.0f, d[10] = r[8] + 1.0f, d[11] = r[9] + 1.0f;   // linedef.bounding_box(map).expanded(2.0)
            }
        }
        at += count;
    }
    return blob;
}

}  // namespace rxflat
