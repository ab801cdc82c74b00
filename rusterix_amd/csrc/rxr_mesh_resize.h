// rxr_mesh_resize.h -- the host arithmetic of rxr_resize_meshes (include/rxr.h): where every registered mesh lies in the pools once
// some meshes' counts have changed.  Plain C++ without HIP, so that tests/mesh_resize_bases_main.cpp compiles it into a program of its
// own (also under the host sanitizers); rxr_api.hip calls it with the counts it read back from k_mesh_resize_check.
#pragma once
#include <stddef.h>
#include <stdint.h>

// first output slots a registration may not reach (rxr_set_meshes: "meshes too large")
#define RXR_MESH_SLOT_LIMIT (1ull << 31)

// The layout rule of rxr_set_meshes over counts [n][2] = (vertices, triangles): per mesh the exclusive prefix sums
//   vin += nv,  tin += nt,  vout += nv + 4 * nt,  tout += 3 * nt
// into bases [n][4] = (vin_base, tin_base, vout_base, tout_base), and the four grand totals.  Returns n when the totals stay below
// the limit (vout < 2^31 and tout < 2^31, which bounds vin and tin as well), else the index of the first mesh WITH which a total
// reaches it: the bases up to and including that mesh are written, the totals are the sums up to and including it.  Every sum is
// taken in 64 bits and the walk stops at the first excess, so nothing wraps whatever the counts are.
static inline size_t rxr_resize_bases(const uint32_t *counts, size_t n, uint32_t *bases, uint64_t totals[4]) {
    uint64_t vin = 0, tin = 0, vout = 0, tout = 0;
    size_t i = 0;
    for (; i < n; ++i) {
        const uint64_t nv = counts[2 * i], nt = counts[2 * i + 1];
        bases[4 * i + 0] = (uint32_t)vin;
        bases[4 * i + 1] = (uint32_t)tin;
        bases[4 * i + 2] = (uint32_t)vout;
        bases[4 * i + 3] = (uint32_t)tout;
        vin += nv;
        tin += nt;
        vout += nv + 4 * nt;
        tout += 3 * nt;
        if (vout >= RXR_MESH_SLOT_LIMIT || tout >= RXR_MESH_SLOT_LIMIT) break;
    }
    totals[0] = vin;
    totals[1] = tin;
    totals[2] = vout;
    totals[3] = tout;
    return i;
}
