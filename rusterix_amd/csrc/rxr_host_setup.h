// rxr_host_setup.h -- the set-up records of a small host-projected frame, built on the host (rxr_upload_frame, rxr_upload.hip).
// The fetch below is make_setup's (rxr_kernels.hip) for such a frame -- the same sections of the frame blob, indexed the same way --
// and the arithmetic is the one definition both sides share (rxr_tri_records, rxr_device.h).  Plain C++: tests/tri_records_main.cpp
// compiles it with a host compiler, also under AddressSanitizer.
#pragma once
#include <stddef.h>
#include <string.h>

#include "rxr_device.h"

// the sections of the staging blob a record is made from, and the frame-wide values
struct HostSetupSource {
    const float *pv;              // projected vertices, 4 floats each
    const float *uv;              // 2 floats each
    const float *nrm;             // 3 floats each (only read for batches with DB_HAS_NORMALS)
    const uint32_t *idx;          // 3 per triangle, batch-local
    const void *edges;            // rxr_edges per triangle, or (edgeless) one `visible` word per triangle
    bool edgeless;                // ABI 5: Edges::new of the projected vertices under the batch's cull mode (DevBatch.mode)
    const uint32_t *tri_info;     // (batch, vert_base) per triangle
    const DevBatch *batches;
    const DevTexDesc *tex;        // the frame's descriptor table
    const uint32_t *clip;         // x0, x1, y0, y1 per batch (RasterParams.batch_clip3d), or NULL
    uint32_t sample_mode, width, height;
};

// records of triangle t for the band [0, height); false: it can never produce a pixel.  A triangle whose Edges record is invisible or
// whose batch is skipped keeps the all-zero records it came with, as k_setup3d leaves them.
inline bool rxr_host_tri_records(const HostSetupSource &F, size_t t, TriSetup &S, TriShade &H) {
    const uint32_t bi = F.tri_info[2 * t], vbase = F.tri_info[2 * t + 1];
    const DevBatch &B = F.batches[bi];
    const size_t i[3] = {(size_t)F.idx[3 * t + 0] + vbase, (size_t)F.idx[3 * t + 1] + vbase, (size_t)F.idx[3 * t + 2] + vbase};
    TriRecordIn in{};
    if (F.edgeless)
        in.E = edges_from_xy(B.mode, ((const uint32_t *)F.edges)[t] != 0u, F.pv[4 * i[0]], F.pv[4 * i[0] + 1], F.pv[4 * i[1]], F.pv[4 * i[1] + 1],
                             F.pv[4 * i[2]], F.pv[4 * i[2] + 1]);
    else in.E = ((const rxr_edges *)F.edges)[t];
    if (!in.E.visible || (B.flags & DB_SKIP)) return false;
    for (int k = 0; k < 3; ++k) {
        memcpy(in.v[k], F.pv + 4 * i[k], 16);
        memcpy(in.uv[k], F.uv + 2 * i[k], 8);
        if (B.flags & DB_HAS_NORMALS) memcpy(in.n[k], F.nrm + 3 * i[k], 12);
    }
    in.batch = bi;
    in.bflags = B.flags;
    in.profile_id = B.profile_id;
    in.repeat_mode = B.repeat_mode;
    in.tex = B.tex;
    if (B.tex >= 0 && !(B.flags & DB_TERRAIN) && B.repeat_mode < 4u) in.desc = F.tex[B.tex];
    in.sample_mode = F.sample_mode;
    in.width = F.width;
    in.row0 = 0u;
    in.row1 = F.height;
    if (F.clip) {
        in.has_clip = 1u;
        for (int k = 0; k < 4; ++k) in.clip[k] = F.clip[4 * bi + k];
    }
    return rxr_tri_records(in, S, H);
}
