// rxr_query.h -- the host scaffold the device queries next to the renderer share (rxr_intersect.hip, rxr_bake.hip, rxr_terrain.hip,
// rxr_terrain_hit.hip, rxr_terrain_mesh.hip, rxr_terrain_gen.hip, rxr_terrain_excl.hip): the cross-stream ordering of a query's lane (rxr_ctx.h: QueryLane), the staging of a blocking form's host
// arrays, and the small helpers of their entry points.  A query's `_run` queues its launches between rxr_query_begin and
// rxr_query_end on whichever stream it is given; its blocking form stages through QueryIO on ctx->stream.
#pragma once
#include <algorithm>
#include <cstring>

#include "rxr_ctx.h"
#include "rxr_query_layout.h"

// orders `s` behind the lane's last call (its scratch, a fault report's host copy: whatever two calls of the query share)
inline int rxr_query_begin(rxr_ctx *ctx, QueryLane &q, hipStream_t s) {
    if (!q.ev) HIPCHK(ctx, hipEventCreateWithFlags(&q.ev, hipEventDisableTiming));
    if (q.pending) HIPCHK(ctx, hipStreamWaitEvent(s, q.ev, 0));
    return RXR_OK;
}
// behind the call's last launch or copy on `s`
inline int rxr_query_end(rxr_ctx *ctx, QueryLane &q, hipStream_t s) {
    HIPCHK(ctx, hipEventRecord(q.ev, s));
    q.pending = true;
    return RXR_OK;
}
// the blocking form has synchronised ctx->stream, and the lane's event lies behind on that very stream
inline void rxr_query_drained(QueryLane &q) { q.pending = false; }

// The blocking form's device copies of the caller's host arrays, in the lane's io buffer: in() / out() per array in the kernel's order,
// upload(), dev<T>(i) for the query's `_run`, download().
struct QueryIO {
    rxr_ctx *ctx;
    QueryLane &lane;
    QueryLayout L;
    const void *src[QueryLayout::MAX] = {};
    void *dst[QueryLayout::MAX] = {};
    unsigned in(const void *host, size_t bytes) {
        src[L.n] = host;
        return L.add(bytes);
    }
    unsigned out(void *host, size_t bytes) {   // host == NULL: an output the caller does not ask for
        dst[L.n] = host;
        return L.add(host ? bytes : 0);
    }
    unsigned inout(void *host, size_t bytes) {   // an output the kernel writes only parts of: the rest comes back as it went up
        dst[L.n] = host;
        return in(host, bytes);
    }
    template <class T>
    T *dev(unsigned i) const {   // (null for an absent output)
        return L.bytes[i] ? (T *)((uint8_t *)lane.io.p + L.off[i]) : nullptr;
    }
    int upload() {
        const int rc = rxr_ensure(ctx, lane.io, std::max<size_t>(L.total, 256));
        if (rc != RXR_OK) return rc;
        for (unsigned i = 0; i < L.n; ++i)
            if (src[i]) HIPCHK(ctx, hipMemcpyAsync(dev<void>(i), src[i], L.bytes[i], hipMemcpyHostToDevice, ctx->stream));
        return RXR_OK;
    }
    int download() {   // ... and waits for them
        for (unsigned i = 0; i < L.n; ++i)
            if (dst[i]) HIPCHK(ctx, hipMemcpyAsync(dst[i], dev<void>(i), L.bytes[i], hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        rxr_query_drained(lane);
        return RXR_OK;
    }
};

// a range of device memory on the context's device?
inline bool rxr_on_device(const rxr_ctx *ctx, const void *p, size_t bytes) {
    hipPointerAttribute_t a0{}, a1{};
    const hipError_t e0 = hipPointerGetAttributes(&a0, p), e1 = hipPointerGetAttributes(&a1, (const uint8_t *)p + bytes - 1);
    if (e0 != hipSuccess || e1 != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return a0.type == hipMemoryTypeDevice && a1.type == hipMemoryTypeDevice && a0.device == ctx->device && a1.device == ctx->device;
}

// a multi-device handle answers a blocking query as its member 0 does: call(member 0), its error carried up to the handle
template <class F>
int rxr_as_member0(rxr_ctx *ctx, F call) {
    rxr_ctx *m0 = rxr_member(ctx, 0);
    const int rc = call(m0);
    return rc == RXR_OK ? rc : rxr_fail(ctx, rc, rxr_last_error(m0));
}

// the rxr_check_* entry points' message out: `err`, cut to the caller's capacity
inline void rxr_copy_message(const std::string &err, char *message, uint32_t message_capacity) {
    if (!message || !message_capacity) return;
    const size_t n = std::min<size_t>(err.size(), message_capacity - 1);
    memcpy(message, err.data(), n);
    message[n] = 0;
}
