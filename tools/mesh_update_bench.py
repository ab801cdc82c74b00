#!/usr/bin/env python3
"""A height stroke's way from the resident heights to the registered meshes, timed both ways: one JSON line per case.

    python tools/mesh_update_bench.py [--reps 10] [--warmup 2] [--only SUBSTRING]

A 512 x 512-cell terrain in 1 024 chunks of 16 x 16 cells, every chunk's mesh registered with rxr_set_meshes on a context of the
tool's own.  Per case, k of the chunks are rebuilt from the resident heights and handed to the renderer

  update_us    THIS path: rxr_terrain_meshes_to into device arrays + rxr_update_meshes_to on the same stream.  Wall time, since
               the call blocks.  Over PCIe: the k 32-byte check records coming back (and the kernel arguments).
  reregister_us  the path before rxr_update_meshes existed: rxr_terrain_meshes into host arrays + rxr_set_meshes of the WHOLE
               scene (host index loop, host box loop, staging copy, upload of every pool, the output pools zeroed, k_proj_static).
               Wall time.  Over PCIe: the three geometry arrays of the k chunks up and down (the blocking form's inout staging)
               and every object-space pool of the scene up.

Both leave the context without a resident frame; the frame upload that follows is the same on both sides and is not timed.
Cases: chunk16_of_1024 (chunk 16 alone), chunks64_of_1024, chunks1024_of_1024, and chunk16_with_static_1m (chunk 16 alone, with a
static mesh of one million triangles registered next to the chunks).  Before the timing, the box rxr_mesh_bounds reports after
this path is compared with the box of the vertices the device built (numpy fmin / fmax)."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="")
    args = ap.parse_args()

    import torch

    import rusterix_amd
    from tests.pick_fuzz import IDENTITY, Mesh3D

    rxr = rusterix_amd.rxr_abi()
    ctx = C.c_void_p()
    assert rxr.rxr_create(C.byref(ctx), 0) == 0
    err = lambda: (rxr.rxr_last_error(ctx) or b"").decode()
    stream = torch.cuda.Stream()
    sp = C.c_void_p(stream.cuda_stream)

    # the heights: every cell listed, and one more row and column for the last chunks' rim
    ys, xs = np.mgrid[0:CELLS + 1, 0:CELLS + 1]
    rng = np.random.default_rng(1)
    h = (2.0 * np.sin(xs / 9.0) * np.cos(ys / 7.0) + 1.5 * np.sin((xs + ys) / 23.0) + rng.uniform(-0.2, 0.2, xs.shape)).astype(F)
    xy = np.ascontiguousarray(np.stack([xs.ravel(), ys.ravel()], axis=1).astype(np.int32))
    scale = (C.c_float * 2)(1.0, 1.0)
    assert rxr.rxr_set_terrain_heights(ctx, scale, xy.ctypes.data, np.ascontiguousarray(h.ravel()).ctypes.data, len(xy)) == 0, err()

    coords = np.ascontiguousarray(np.array([(x, y) for y in range(CELLS // CS) for x in range(CELLS // CS)], np.int32))
    n_all = len(coords)
    host = [np.zeros((n_all, 2), np.uint32), np.zeros((n_all, VS, 4), F), np.zeros((n_all, TS, 3), np.uint32), np.zeros((n_all, VS, 3), F)]
    assert rxr.rxr_terrain_meshes(ctx, coords.ctypes.data, n_all, CS, *(a.ctypes.data for a in host)) == 0, err()
    uvs = np.zeros((VS, 2), F)

    def static_mesh(side):
        """a grid of side x side cells, two triangles each, below the terrain"""
        gy, gx = np.mgrid[0:side + 1, 0:side + 1]
        v = np.ones(((side + 1) ** 2, 4), F)
        v[:, 0], v[:, 1], v[:, 2] = gx.ravel() * (CELLS / side), -5.0, gy.ravel() * (CELLS / side)
        i0 = (gy[:-1, :-1] * (side + 1) + gx[:-1, :-1]).ravel().astype(np.uint32)
        idx = np.stack([i0, i0 + side + 1, i0 + 1, i0 + 1, i0 + side + 1, i0 + side + 2], axis=1).reshape(-1, 3)
        nr = np.zeros((len(v), 3), F)
        nr[:, 1] = 1.0
        return v, np.ascontiguousarray(idx), np.zeros((len(v), 2), F), nr

    def scene(extra):
        """the rxr_mesh3d array of the 1 024 chunk meshes (+ `extra`), pointing into `host`; (array, what it points into)"""
        arr = (Mesh3D * (n_all + len(extra)))()
        for i in range(n_all):
            a = arr[i]
            a.vertices, a.indices, a.uvs, a.normals = host[1][i].ctypes.data, host[2][i].ctypes.data, uvs.ctypes.data, host[3][i].ctypes.data
            a.n_vertices, a.n_triangles = int(host[0][i, 0]), int(host[0][i, 1])
            a.transform_3d, a.shader, a.list, a.chunk = IDENTITY, -1, 2, -1
            a.source.kind = 3
        for k, (v, idx, uv, nr) in enumerate(extra):
            a = arr[n_all + k]
            a.vertices, a.indices, a.uvs, a.normals = v.ctypes.data, idx.ctypes.data, uv.ctypes.data, nr.ctypes.data
            a.n_vertices, a.n_triangles = len(v), len(idx)
            a.transform_3d, a.shader, a.list, a.chunk = IDENTITY, -1, 3, -1
            a.source.kind = 3
        return arr

    def case(name, chunk_ids, extra=()):
        if args.only and args.only not in name:
            return
        ids = np.ascontiguousarray(chunk_ids, np.uint32)
        k = len(ids)
        cc = np.ascontiguousarray(coords[ids])
        arr = scene(extra)
        n_meshes = len(arr)
        assert rxr.rxr_set_meshes(ctx, C.cast(arr, C.c_void_p), n_meshes) == 0, err()
        dev = [torch.zeros((k, 2), dtype=torch.int32, device="cuda"), torch.zeros((k, VS, 4), device="cuda"),
               torch.zeros((k, TS, 3), dtype=torch.int32, device="cuda"), torch.zeros((k, VS, 3), device="cuda")]
        torch.cuda.synchronize()

        def update():
            rc = rxr.rxr_terrain_meshes_to(ctx, cc.ctypes.data, k, CS, *(d.data_ptr() for d in dev), sp)
            assert rc == 0, err()
            rc = rxr.rxr_update_meshes_to(ctx, ids.ctypes.data, k, *(d.data_ptr() for d in dev), VS, TS, sp)
            assert rc == 0, err()

        sub = [np.zeros((k, 2), np.uint32), np.zeros((k, VS, 4), F), np.zeros((k, TS, 3), np.uint32), np.zeros((k, VS, 3), F)]

        def reregister():
            rc = rxr.rxr_terrain_meshes(ctx, cc.ctypes.data, k, CS, *(a.ctypes.data for a in sub))
            assert rc == 0, err()
            for j, i in enumerate(ids):      # the caller's batches take the new arrays
                for a in range(1, 4):
                    host[a][i] = sub[a][j]
            rc = rxr.rxr_set_meshes(ctx, C.cast(arr, C.c_void_p), n_meshes)
            assert rc == 0, err()

        update()
        lo, hi = (C.c_float * 3)(), (C.c_float * 3)()
        for j in (0, k - 1):
            assert rxr.rxr_mesh_bounds(ctx, int(ids[j]), lo, hi) == 0, err()
            v = host[1][ids[j]][: host[0][ids[j], 0], :3]
            assert (np.array(lo[:], F) == np.fmin.reduce(v, axis=0)).all() and (np.array(hi[:], F) == np.fmax.reduce(v, axis=0)).all(), name

        def timed(fn):
            for _ in range(args.warmup):
                fn()
            us = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                fn()
                us.append((time.perf_counter() - t0) * 1e6)
            return us

        up, re = timed(update), timed(reregister)
        nv = int(sum(a.n_vertices for a in arr))
        nt = int(sum(a.n_triangles for a in arr))
        geometry = k * (VS * 16 + TS * 12 + VS * 12)
        line = dict(case=name, chunks=k, registered_meshes=n_meshes, registered_triangles=nt, reps=args.reps,
                    update_us_median=round(statistics.median(up), 1), update_us_min=round(min(up), 1), update_us_max=round(max(up), 1),
                    reregister_us_median=round(statistics.median(re), 1), reregister_us_min=round(min(re), 1), reregister_us_max=round(max(re), 1),
                    speedup=round(statistics.median(re) / statistics.median(up), 2),
                    update_pcie_bytes_down=k * 32, update_pcie_bytes_up=0,
                    reregister_pcie_bytes_down=geometry + k * 8,
                    reregister_pcie_bytes_up=geometry + nv * (16 + 8 + 12) + nt * 12 + 3 * 4 * (n_meshes + 1) + 96 * n_meshes)
        print(json.dumps(line), flush=True)

    case("chunk16_of_1024", [16])
    case("chunks64_of_1024", list(range(16, 16 + 64)))
    case("chunks1024_of_1024", list(range(n_all)))
    case("chunk16_with_static_1m", [16], extra=(static_mesh(708),))
    rxr.rxr_destroy(ctx)


if __name__ == "__main__":
    main()
