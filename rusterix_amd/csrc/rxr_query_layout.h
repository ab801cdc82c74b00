// rxr_query_layout.h -- where the arrays of a blocking device query lie inside its lane's io buffer (rxr_query.h: QueryIO).  Plain
// arithmetic without a HIP header, so that tests/query_layout_walk.cpp walks it on the CPU.
#pragma once
#include <cassert>
#include <cstddef>

// add(bytes) per array in the caller's order: a section starts on a 16-byte boundary (the shader bake stores float4 texels), an
// absent array (0 bytes) takes no room, and `total` is the end of the last section
struct QueryLayout {
    enum { MAX = 8 };
    size_t off[MAX] = {}, bytes[MAX] = {}, total = 0;
    unsigned n = 0;
    unsigned add(size_t b) {
        assert(n < MAX);
        off[n] = b ? (total + 15) / 16 * 16 : total;
        bytes[n] = b;
        total = off[n] + b;
        return n++;
    }
};
