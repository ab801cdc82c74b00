#!/usr/bin/env python3
"""Vertex normals on the device against the host mirror's CPU form, both routes: one JSON line per case.

    python tools/vertex_normals_bench.py [--reps 20] [--warmup 3] [--only SUBSTRING] [--no-sweep]

Per case the meshes lie in device memory in the strided layout of rxr_vertex_normals_to (include/rxr.h) and

  small_us / general_us   STREAM time of one rxr_vertex_normals_to call (HIP events on a side stream around the call, median over
                          --reps; min and max next to it), with RXR_VERTEX_NORMALS_SMALL_MAX forcing the route.  null where the
                          route cannot take the case (a triangle stride above what one workgroup's LDS holds); the route that ran
                          is read back from rxr_debug_vertex_normals and recorded.
  default_route           what the library picks on its own
  cpu_pool_us             WALL time of the mirror's Scene::compute_static_normals over the worker pool, one batch a task
                          (RXR_HOST_THREADS, 16 unless the environment says otherwise), over the same meshes as host batches
  blocking_us             (one_box only) WALL time of the blocking rxr_vertex_normals: staging up, kernel, staging down

Before any timing every word of both routes' normals is compared with the mirror's CPU normals (a NaN against a NaN).
Cases: terrain_1024x16 (the 1 024 chunk meshes of 16 x 16 cells of a 512 x 512 terrain, vertices and indices from
rxr_terrain_meshes_to), terrain_1x64 (one chunk of 64 x 64), teapot (tests/golden/teapot_mesh.npz), box_grid_1m (289 meshes of
289 boxes: 1 002 252 triangles), one_box (12 triangles, blocking form).  The sweep (crossover_*) times one mesh and 64 meshes of
seeded random triangles at growing triangle strides through both routes: where the small route stops winning is what
NRM_SMALL_MAX in rxr_normals.hip is set from."""
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
os.environ.setdefault("RXR_HOST_THREADS", "16")
F = np.float32
SMALL, GENERAL = 1, 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="")
    ap.add_argument("--no-sweep", action="store_true")
    args = ap.parse_args()

    import torch

    import rusterix_amd
    from rusterix_amd import binding as B

    api = rusterix_amd.load()
    rxr = rusterix_amd.rxr_abi()
    ctx = C.c_void_p()
    assert rxr.rxr_create(C.byref(ctx), 0) == 0
    err = lambda: (rxr.rxr_last_error(ctx) or b"").decode()
    stream = torch.cuda.Stream()
    sp = C.c_void_p(stream.cuda_stream)
    consts = (C.c_uint32 * 3)()
    rxr.rxr_debug_vertex_normals_constants(consts)
    bound, cap = int(consts[0]), int(consts[1])

    def to_dev(a):
        return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()

    def same(got, want):
        nan = np.isnan(want)
        return bool((np.isnan(got) == nan).all() and (got.view(np.uint32)[~nan] == want.view(np.uint32)[~nan]).all())

    def cpu_side(counts, v, i):
        """the mirror's batches of the same meshes: (cpu_pool_us statistics, the CPU normals packed like the device's)"""
        scene = api.Scene.empty()
        n = len(counts)
        for k in range(n):
            nv, nt = int(counts[k, 0]), int(counts[k, 1])
            scene.add_d3_static(api.Batch3D.new(v[k, :nv], i[k, :nt], np.zeros((nv, 2), F)))
        us = []
        for r in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            scene.compute_static_normals(threads=True)
            if r >= args.warmup:
                us.append((time.perf_counter() - t0) * 1e6)
        want = np.zeros((n, v.shape[1], 3), F)
        for k in range(n):
            want[k, :int(counts[k, 0])] = scene.batch3d_normals(B.LIST_STATIC, k)
        return us, want

    def stream_us(call):
        for _ in range(args.warmup):
            call()
        us = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            call()
            e1.record(stream)
            e1.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3)
        return us

    def stats(prefix, us):
        return {prefix + "_us": round(statistics.median(us), 1), prefix + "_us_min": round(min(us), 1), prefix + "_us_max": round(max(us), 1)}

    def case(name, counts, v, i, dev=None, cpu=True, extra=None):
        """counts / v / i: host arrays; dev: the same on the device already (else they are copied up once, outside the timing)"""
        if args.only and args.only not in name:
            return
        n, vs, ts = len(counts), v.shape[1], i.shape[1]
        d_c, d_v, d_i = dev or (to_dev(counts), to_dev(v), to_dev(i))
        d_n = torch.zeros((n, vs, 3), device="cuda")
        d_r = torch.zeros((n,), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        line = dict(case=name, meshes=n, vertex_stride=vs, triangle_stride=ts, vertices=int(counts[:, 0].sum()), triangles=int(counts[:, 1].sum()),
                    reps=args.reps, small_bound=bound)
        cpu_us, want = cpu_side(counts, v, i) if cpu else (None, None)

        def call():
            rc = rxr.rxr_vertex_normals_to(ctx, n, d_c.data_ptr(), d_v.data_ptr() or None, d_i.data_ptr() or None, d_n.data_ptr() or None, d_r.data_ptr(), vs, ts, sp)
            assert rc == 0, err()

        launches = C.c_uint32()
        for route, env in (("default", None), ("small", "4000000000"), ("general", "0")):
            if env is None:
                os.environ.pop("RXR_VERTEX_NORMALS_SMALL_MAX", None)
            else:
                os.environ["RXR_VERTEX_NORMALS_SMALL_MAX"] = env
            d_n.zero_()
            torch.cuda.synchronize()
            call()
            torch.cuda.synchronize()
            ran = rxr.rxr_debug_vertex_normals(ctx, C.byref(launches))
            assert (d_r.cpu().numpy() == 0).all(), name
            if want is not None:
                assert same(d_n.cpu().numpy(), want), f"{name}: the {route} route's normals differ from the mirror's CPU normals"
                line["words_compared"] = int(want.size)
            if route == "default":
                line["default_route"] = "small" if ran == SMALL else "general"
                continue
            if ran != (SMALL if route == "small" else GENERAL):      # (an override is cut to what a workgroup holds)
                line[route + "_us"] = None
                continue
            line.update(stats(route, stream_us(call)))
            line[route + "_launches"] = int(launches.value)
        os.environ.pop("RXR_VERTEX_NORMALS_SMALL_MAX", None)
        if cpu_us is not None:
            line.update(stats("cpu_pool", cpu_us))
            line["cpu_threads"] = int(os.environ["RXR_HOST_THREADS"])
        if extra:
            line.update(extra(counts, v, i, want))
        print(json.dumps(line), flush=True)

    # ---- the terrain cases: vertices and indices from rxr_terrain_meshes_to -------------------------------------------------------------
    def terrain(name, cells, cs, coords):
        if args.only and args.only not in name:
            return
        ys, xs = np.mgrid[0:cells + 1, 0:cells + 1]
        rng = np.random.default_rng(1)
        h = (2.0 * np.sin(xs / 9.0) * np.cos(ys / 7.0) + 1.5 * np.sin((xs + ys) / 23.0) + rng.uniform(-0.2, 0.2, xs.shape)).astype(F)
        xy = np.ascontiguousarray(np.stack([xs.ravel(), ys.ravel()], axis=1).astype(np.int32))
        scale = (C.c_float * 2)(1.0, 1.0)
        assert rxr.rxr_set_terrain_heights(ctx, scale, xy.ctypes.data, np.ascontiguousarray(h.ravel()).ctypes.data, len(xy)) == 0, err()
        cc = np.ascontiguousarray(np.array(coords, np.int32))
        n, vs, ts = len(cc), (cs + 1) ** 2, 2 * cs * cs
        dev = [torch.zeros((n, 2), dtype=torch.int32, device="cuda"), torch.zeros((n, vs, 4), device="cuda"),
               torch.zeros((n, ts, 3), dtype=torch.int32, device="cuda"), torch.zeros((n, vs, 3), device="cuda")]
        torch.cuda.synchronize()
        assert rxr.rxr_terrain_meshes_to(ctx, cc.ctypes.data, n, cs, *(d.data_ptr() for d in dev), sp) == 0, err()
        torch.cuda.synchronize()
        counts = dev[0].cpu().numpy().view(np.uint32)
        v, i = dev[1].cpu().numpy(), dev[2].cpu().numpy().view(np.uint32)
        theirs = dev[3].cpu().numpy()

        def against_the_mesh_kernel(counts, v, i, want):
            return dict(equals_terrain_mesh_kernel=bool(same(theirs, want)))

        case(name, counts, v, i, dev=tuple(dev[:3]), extra=against_the_mesh_kernel)

    terrain("terrain_1024x16", 512, 16, [(x, y) for y in range(32) for x in range(32)])
    terrain("terrain_1x64", 64, 64, [(0, 0)])

    # ---- the teapot ------------------------------------------------------------------------------------------------------------------------
    z = np.load(os.path.join(ROOT, "tests", "golden", "teapot_mesh.npz"))
    tv = np.ones((1, len(z["positions"]), 4), F)
    tv[0, :, :3] = z["positions"]
    ti = np.ascontiguousarray(z["indices"].astype(np.uint32)[None])
    case("teapot", np.array([[tv.shape[1], ti.shape[1]]], np.uint32), tv, ti)

    # ---- the box grid: 289 meshes of 289 boxes (rusterix_amd/scenes.py box_grid_scene's geometry) ------------------------------------------
    if not args.only or args.only in "box_grid_1m one_box":
        bv, bi, _, _ = api.Batch3D.from_box(0.0, 0.0, 0.0, 0.16, 0.16, 0.16).geometry()
        nb = 289
        rng = np.random.default_rng(200)
        ys = rng.random((nb, nb)).astype(F) * F(0.4)
        gv = np.tile(bv[None, None], (nb, nb, 1, 1))
        gv[:, :, :, 0] += (np.arange(nb, dtype=F) * F(0.2))[None, :, None]
        gv[:, :, :, 1] += ys[:, :, None]
        gv[:, :, :, 2] += (np.arange(nb, dtype=F) * F(0.2))[:, None, None]
        gi = bi[None, None] + (np.arange(nb, dtype=np.uint32) * np.uint32(24))[None, :, None, None]
        gi = np.ascontiguousarray(np.broadcast_to(gi, (nb, nb, 12, 3)).reshape(nb, nb * 12, 3))
        case("box_grid_1m", np.tile(np.array([[nb * 24, nb * 12]], np.uint32), (nb, 1)), np.ascontiguousarray(gv.reshape(nb, nb * 24, 4)), gi)

        # ---- one box through the blocking form ---------------------------------------------------------------------------------------------
        def blocking(counts, v, i, want):
            out = np.zeros((1, 24, 3), F)
            us = []
            for r in range(args.warmup + args.reps):
                t0 = time.perf_counter()
                rc = rxr.rxr_vertex_normals(ctx, 1, counts.ctypes.data, v.ctypes.data, i.ctypes.data, out.ctypes.data, 24, 12)
                if r >= args.warmup:
                    us.append((time.perf_counter() - t0) * 1e6)
                assert rc == 0, err()
            assert same(out, want)
            return stats("blocking", us)

        case("one_box", np.array([[24, 12]], np.uint32), np.ascontiguousarray(bv[None]), np.ascontiguousarray(bi[None]), extra=blocking)

    # ---- the crossover: seeded random triangles, one mesh and 64 meshes, growing strides ---------------------------------------------------
    if not args.no_sweep:
        for n in (1, 64):
            for ts in (128, 256, 512, 1024, 1536, 2048, 2730, 3413, 4096, 5120, cap):
                rng = np.random.default_rng(ts)
                vs = ts // 2 + 2                                       # about as many vertices per triangle as a closed surface has
                v = np.ones((n, vs, 4), F)
                v[:, :, :3] = rng.random((n, vs, 3), dtype=F) * F(8.0) - F(4.0)
                a = rng.integers(0, vs, (n, ts, 1))
                i = np.ascontiguousarray(((a + np.concatenate([np.zeros((n, ts, 1), np.int64), rng.integers(1, vs // 2, (n, ts, 1)),
                                                                rng.integers(vs // 2, vs - 1, (n, ts, 1))], axis=2)) % vs).astype(np.uint32))
                case(f"crossover_n{n}_ts{ts}", np.tile(np.array([[vs, ts]], np.uint32), (n, 1)), v, i, cpu=(ts in (512, 3413)))
    rxr.rxr_destroy(ctx)


if __name__ == "__main__":
    main()
