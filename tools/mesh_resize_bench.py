#!/usr/bin/env python3
"""A removed row of terrain cells' way from the resident heights to the registered meshes, timed both ways: one JSON line per case.

    python tools/mesh_resize_bench.py [--reps 10] [--warmup 2] [--only SUBSTRING] [--out FILE]

The scene of tools/mesh_update_bench.py: a 512 x 512-cell terrain in 1 024 chunks of 16 x 16 cells, every chunk's mesh registered with
rxr_set_meshes.  Per case, k "dirty" chunks lose one row of cells (their fourth) or get it back -- the heights are registered again
between the repetitions, alternately without and with those rows, OUTSIDE the timed part -- so that the counts of the k meshes really
change every time, and the k meshes are rebuilt from the resident heights and handed to the renderer

  resize_us      THIS path: rxr_terrain_meshes_to into device arrays + rxr_resize_meshes_to on the same stream.  Wall time, since the
                 call blocks.  Over PCIe: the k 40-byte check records down, the small tables (three prefix arrays, the mesh table, the
                 source words) up.
  reregister_us  the host route: rxr_terrain_meshes into host arrays + rxr_set_meshes of the WHOLE scene.  Wall time.
  repack_us      the stream time of k_mesh_repack alone (events around its launch), of the last repetition
  copy_us        one hipMemcpyAsync device-to-device of the bytes that kernel wrote (repack_bytes), in the same run, after a warm-up
                 copy: the yardstick of "memory-bound".  repack_over_copy is their ratio; nothing asserts it.

Both paths leave the context without a resident frame; the frame upload that follows is the same on both sides and is not timed.
Cases: chunk16_of_1024, chunks64_of_1024, chunks1024_of_1024 and chunk16_with_static_1m (chunk 16 alone, next to a static mesh of one
million triangles), and chunk16_registered_alone (that chunk the only mesh of the scene).  Before the timing, every word of the object pools and every box after this path is compared with a second
context that took the host route."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
F = np.float32
CS, CELLS = 16, 512
VS, TS = (CS + 1) ** 2, 2 * CS * CS
ROW = 3     # the row of cells (chunk-local y) a dirty chunk loses


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch

    import rusterix_amd
    from tests.pick_fuzz import IDENTITY, Mesh3D

    rxr = rusterix_amd.rxr_abi()
    ctx, ref = C.c_void_p(), C.c_void_p()
    assert rxr.rxr_create(C.byref(ctx), 0) == 0 and rxr.rxr_create(C.byref(ref), 0) == 0
    err = lambda c=None: (rxr.rxr_last_error(c or ctx) or b"").decode()
    stream = torch.cuda.Stream()
    sp = C.c_void_p(stream.cuda_stream)
    out = open(args.out, "a") if args.out else None

    ys, xs = np.mgrid[0:CELLS + 1, 0:CELLS + 1]
    rng = np.random.default_rng(1)
    h = (2.0 * np.sin(xs / 9.0) * np.cos(ys / 7.0) + 1.5 * np.sin((xs + ys) / 23.0) + rng.uniform(-0.2, 0.2, xs.shape)).astype(F)
    all_xy = np.stack([xs.ravel(), ys.ravel()], axis=1).astype(np.int32)
    all_h = h.ravel()
    scale = (C.c_float * 2)(1.0, 1.0)
    coords = np.ascontiguousarray(np.array([(x, y) for y in range(CELLS // CS) for x in range(CELLS // CS)], np.int32))
    n_all = len(coords)

    def set_heights(c, without_rows_of=()):
        """every cell listed, but for row ROW of the chunks `without_rows_of`"""
        dirty = np.zeros(n_all + 1, bool)      # (one more: the rim's cells belong to no chunk)
        dirty[list(without_rows_of)] = True
        side = CELLS // CS
        chunk = np.where((all_xy[:, 0] < CELLS) & (all_xy[:, 1] < CELLS), (all_xy[:, 1] // CS) * side + all_xy[:, 0] // CS, n_all)
        keep = ~(dirty[chunk] & (all_xy[:, 1] % CS == ROW))
        xy, hh = np.ascontiguousarray(all_xy[keep]), np.ascontiguousarray(all_h[keep])
        assert rxr.rxr_set_terrain_heights(c, scale, xy.ctypes.data, hh.ctypes.data, len(xy)) == 0, err(c)

    set_heights(ctx)
    host = [np.zeros((n_all, 2), np.uint32), np.zeros((n_all, VS, 4), F), np.zeros((n_all, TS, 3), np.uint32), np.zeros((n_all, VS, 3), F)]
    assert rxr.rxr_terrain_meshes(ctx, coords.ctypes.data, n_all, CS, *(a.ctypes.data for a in host)) == 0, err()
    full = [a.copy() for a in host]
    uvs = np.zeros((VS, 2), F)

    def static_mesh(side):
        gy, gx = np.mgrid[0:side + 1, 0:side + 1]
        v = np.ones(((side + 1) ** 2, 4), F)
        v[:, 0], v[:, 1], v[:, 2] = gx.ravel() * (CELLS / side), -5.0, gy.ravel() * (CELLS / side)
        i0 = (gy[:-1, :-1] * (side + 1) + gx[:-1, :-1]).ravel().astype(np.uint32)
        idx = np.stack([i0, i0 + side + 1, i0 + 1, i0 + 1, i0 + side + 1, i0 + side + 2], axis=1).reshape(-1, 3)
        nr = np.zeros((len(v), 3), F)
        nr[:, 1] = 1.0
        return v, np.ascontiguousarray(idx), np.zeros((len(v), 2), F), nr

    def scene(reg, extra):
        """the rxr_mesh3d array of the chunk meshes `reg` (+ `extra`), pointing into `host`"""
        arr = (Mesh3D * (len(reg) + len(extra)))()
        for m, i in enumerate(reg):
            a = arr[m]
            a.vertices, a.indices, a.uvs, a.normals = host[1][i].ctypes.data, host[2][i].ctypes.data, uvs.ctypes.data, host[3][i].ctypes.data
            a.n_vertices, a.n_triangles = int(host[0][i, 0]), int(host[0][i, 1])
            a.transform_3d, a.shader, a.list, a.chunk = IDENTITY, -1, 2, -1
            a.source.kind = 3
        for k, (v, idx, uv, nr) in enumerate(extra):
            a = arr[len(reg) + k]
            a.vertices, a.indices, a.uvs, a.normals = v.ctypes.data, idx.ctypes.data, uv.ctypes.data, nr.ctypes.data
            a.n_vertices, a.n_triangles = len(v), len(idx)
            a.transform_3d, a.shader, a.list, a.chunk = IDENTITY, -1, 3, -1
            a.source.kind = 3
        return arr

    def pools(c):
        totals = (C.c_uint64 * 2)()
        assert rxr.rxr_debug_object_pools(c, totals, None, None, None, None, 0, 0) == 0, err(c)
        nv, nt = int(totals[0]), int(totals[1])
        a = [np.zeros((nv, 4), F), np.zeros((nv, 2), F), np.zeros((nt, 3), np.uint32), np.zeros((nv, 3), F)]
        assert rxr.rxr_debug_object_pools(c, totals, *(x.ctypes.data for x in a), nv, nt) == 0, err(c)
        return a

    def case(name, chunk_ids, extra=(), reg=None):
        """chunk_ids: the dirty meshes, as positions in `reg`, the chunks registered (default: all)"""
        if args.only and args.only not in name:
            return
        reg = list(range(n_all)) if reg is None else list(reg)
        ids = np.ascontiguousarray(chunk_ids, np.uint32)
        k = len(ids)
        chunks = np.array(reg)[ids]
        cc = np.ascontiguousarray(coords[chunks])
        for a, b in zip(host, full):
            a[:] = b
        arr = scene(reg, extra)
        n_meshes = len(arr)
        set_heights(ctx)
        assert rxr.rxr_set_meshes(ctx, C.cast(arr, C.c_void_p), n_meshes) == 0, err()
        dev = [torch.zeros((k, 2), dtype=torch.int32, device="cuda"), torch.zeros((k, VS, 4), device="cuda"),
               torch.zeros((k, TS, 3), dtype=torch.int32, device="cuda"), torch.zeros((k, VS, 3), device="cuda")]
        torch.cuda.synchronize()
        state = dict(cut=False)

        def toggle():    # (untimed) the dirty chunks lose their row, or get it back
            state["cut"] = not state["cut"]
            set_heights(ctx, chunks if state["cut"] else ())

        def resize():
            rc = rxr.rxr_terrain_meshes_to(ctx, cc.ctypes.data, k, CS, *(d.data_ptr() for d in dev), sp)
            assert rc == 0, err()
            rc = rxr.rxr_resize_meshes_to(ctx, ids.ctypes.data, k, dev[0].data_ptr(), dev[1].data_ptr(), None, dev[2].data_ptr(), dev[3].data_ptr(), VS, TS, sp)
            assert rc == 0, err()

        sub = [np.zeros((k, 2), np.uint32), np.zeros((k, VS, 4), F), np.zeros((k, TS, 3), np.uint32), np.zeros((k, VS, 3), F)]

        def reregister(c=None):
            c = c or ctx
            rc = rxr.rxr_terrain_meshes(ctx, cc.ctypes.data, k, CS, *(a.ctypes.data for a in sub))
            assert rc == 0, err()
            for j, i in enumerate(ids):      # the caller's batches take the new arrays and counts
                for a in range(4):
                    host[a][chunks[j]] = sub[a][j]
                arr[int(i)].n_vertices, arr[int(i)].n_triangles = int(sub[0][j, 0]), int(sub[0][j, 1])
            rc = rxr.rxr_set_meshes(c, C.cast(arr, C.c_void_p), n_meshes)
            assert rc == 0, err(c)

        # every word first: this path on ctx against the host route on a second context
        toggle()
        resize()
        reregister(ref)
        assert int(sub[0][0, 1]) < TS, "the row of cells should have left the mesh"
        for got, want in zip(pools(ctx), pools(ref)):
            assert got.shape == want.shape and got.tobytes() == want.tobytes(), name
        lo, hi, lo2, hi2 = ((C.c_float * 3)() for _ in range(4))
        for m in range(n_meshes):
            assert rxr.rxr_mesh_bounds(ctx, m, lo, hi) == 0 and rxr.rxr_mesh_bounds(ref, m, lo2, hi2) == 0
            assert (np.array(lo[:]) == np.array(lo2[:])).all() and (np.array(hi[:]) == np.array(hi2[:])).all(), (name, m)
        assert rxr.rxr_set_meshes(ref, None, 0) == 0

        def timed(fn):
            for _ in range(args.warmup):
                toggle()
                fn()
            us = []
            for _ in range(args.reps):
                toggle()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                us.append((time.perf_counter() - t0) * 1e6)
            return us

        rs = timed(resize)
        us2, nbytes = (C.c_float * 2)(), C.c_uint64()
        assert rxr.rxr_debug_resize_repack(ctx, us2, C.byref(nbytes)) == 0, err()
        re = timed(reregister)
        nt = int(sum(a.n_triangles for a in arr))
        line = dict(case=name, chunks=k, registered_meshes=n_meshes, registered_triangles=nt, reps=args.reps,
                    resize_us_median=round(statistics.median(rs), 1), resize_us_min=round(min(rs), 1), resize_us_max=round(max(rs), 1),
                    reregister_us_median=round(statistics.median(re), 1), reregister_us_min=round(min(re), 1), reregister_us_max=round(max(re), 1),
                    speedup=round(statistics.median(re) / statistics.median(rs), 2),
                    repack_us=round(us2[0], 1), copy_us=round(us2[1], 1), repack_bytes=int(nbytes.value),
                    repack_over_copy=round(us2[0] / us2[1], 2) if us2[1] else None)
        print(json.dumps(line), flush=True)
        if out:
            out.write(json.dumps(line) + "\n")
            out.flush()

    case("chunk16_of_1024", [16])
    case("chunks64_of_1024", list(range(16, 16 + 64)))
    case("chunks1024_of_1024", list(range(n_all)))
    case("chunk16_with_static_1m", [16], extra=(static_mesh(708),))
    case("chunk16_registered_alone", [0], reg=[16])      # a lone small scene: the blocking call's fixed cost against a host route with little to do
    rxr.rxr_destroy(ctx)
    rxr.rxr_destroy(ref)


if __name__ == "__main__":
    main()
