#!/usr/bin/env python3
"""Timing of the generated terrain's per-tile chunk meshes on the device (rxr_generated_tile_meshes_to: grid, heights, apply_exclusions
and partition_by_tiles) against two baselines: one JSON line per case.

    python tools/terrain_tiles_bench.py [--reps 10] [--warmup 2] [--cpu-reps 1] [--only SUBSTRING] [--no-cpu]

--only runs the cases whose name contains SUBSTRING (for a profiler run of one case).

The map, the generator and the sectors are those of tools/terrain_exclusion_bench.py (a 512 x 512 map of 16 x 16 chunks of 32 x 32
cells, 16 control points, no powf: every word of the device's answer must equal the CPU's), at subdivisions 1 and 4, in three
configurations: one tile everywhere (t1_s0), four tiles in vertical stripes eight cells wide (t4_s0: four groups in every chunk),
and those stripes with 8 excluded squares (t4_s8: the unshared layout in the chunks a square touches):
  all_x256     the 256 chunks in ONE rxr_generated_tile_meshes_to call
  calls_x256   the same chunks as 256 calls of one box each, queued back to back on one stream
  chunk        one chunk (the one with the most active sectors); this case also times the blocking form with host arrays
  stroke_xK    K dirty chunks of a scene whose 256 x groups meshes are registered: the chain rxr_generated_tile_meshes_to ->
               rxr_vertex_normals_to -> rxr_update_meshes_to on one stream (wall time: the update blocks) against the host route it
               replaces, measured as rxr_generated_tile_meshes + rxr_vertex_normals into host arrays + rxr_set_meshes of the whole
               scene -- a LOWER bound of that route, whose partition would run on the host as well
us: events around the case's calls on a stream, outputs staying on the device; median, minimum and maximum over `reps`.
meshes_only_us: the same for rxr_generated_meshes_to alone over the same boxes -- the call this one extends; partition_factor is
their ratio.  CPU baseline: the mirror's generate_tile_meshes_cpu over its worker pool of CPU_THREADS = 16 threads (heights and keep
flags over the pool box by box, then the partition one box a task over the pool), every word compared first."""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
import terrain_exclusion_bench as EB  # noqa: E402  (the map, the generator and the sectors)

CPU_THREADS = EB.CPU_THREADS
F = np.float32


def stripes(n_tiles):
    """the whole map in vertical stripes eight cells wide, slots 0 .. n_tiles - 1 in turn: (cells [N][2], slots [N])"""
    if n_tiles == 1:
        return np.zeros((0, 2), np.int32), np.zeros(0, np.uint32)
    xs, zs = np.meshgrid(np.arange(int(EB.MAP), dtype=np.int32), np.arange(int(EB.MAP), dtype=np.int32), indexing="ij")
    slot = ((xs // 8) % n_tiles).astype(np.uint32)
    keep = slot > 0
    return np.column_stack([xs[keep], zs[keep]]).astype(np.int32), slot[keep]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cpu-reps", type=int, default=1)
    ap.add_argument("--only", default="")
    ap.add_argument("--no-cpu", action="store_true", help="skip the CPU baseline and the comparison (profiler runs)")
    args = ap.parse_args()

    os.environ["RXR_HOST_THREADS"] = str(CPU_THREADS)      # read once, when the mirror's worker pool starts

    import torch

    import rusterix_amd
    from tests.pick_fuzz import IDENTITY, Mesh3D
    from rusterix_amd import binding as B

    api = rusterix_amd.load()
    rxr = rusterix_amd.rxr_abi()
    ctx = C.c_void_p(api.lib.rxh_context())
    stream = torch.cuda.Stream()
    sp = C.c_void_p(stream.cuda_stream)
    err = lambda: (rxr.rxr_last_error(ctx) or b"").decode()

    def timed(calls):
        for _ in range(args.warmup):
            calls()
        stream.synchronize()
        us = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            calls()
            e1.record(stream)
            stream.synchronize()
            us.append(e0.elapsed_time(e1) * 1000.0)
        assert rxr.rxr_synchronize(ctx) == 0, err()
        return us

    def wall(call, reps):
        out = []
        for _ in range(reps):
            t0 = time.perf_counter()
            call()
            out.append((time.perf_counter() - t0) * 1e6)
        return statistics.median(out)

    def strides(sub, n_sectors):
        cells = (32 * sub) ** 2
        return (6 * cells if n_sectors else (32 * sub + 1) ** 2), 2 * cells

    def device_arrays(n, mg, vs, ts):
        m = n * mg
        z = lambda shape, dt=torch.int32: torch.zeros(shape, dtype=dt, device="cuda")
        return [z((n, 4)), z((m, 2)), z((m,)), z((m, vs, 4), torch.float32), z((m, vs, 2), torch.float32), z((m, ts, 3))]

    cpu_cache = {}

    def case(name, gen, sub, n_tiles, n_sectors, boxes, per_call):
        if args.only and args.only not in name:
            return
        b = np.ascontiguousarray(np.asarray(boxes, F).reshape(-1, 4))
        n, mg = len(b), n_tiles
        vs, ts = strides(sub, n_sectors)
        gen.generate_tile_meshes(b[:1], mg, vs, ts)   # registers the lists on the mirror's context
        dev = device_arrays(n, mg, vs, ts)
        torch.cuda.synchronize()
        off = [4, 2 * mg, mg, mg * vs * 4, mg * vs * 2, mg * ts * 3]   # words a box

        def calls():
            for b0 in range(0, n, per_call):
                p = [d.data_ptr() + 4 * b0 * o for d, o in zip(dev, off)]
                rc = rxr.rxr_generated_tile_meshes_to(ctx, b[b0:].ctypes.data, min(per_call, n - b0), sub, mg, vs, ts, *p, sp)
                assert rc == 0, err()

        us = timed(calls)
        n_calls = (n + per_call - 1) // per_call
        rounds = rxr.rxr_debug_terrain_tile_launches(ctx) * n_calls
        # the call this one extends, over the same boxes
        mstride = vs
        dc, dv = torch.zeros((n, 4), dtype=torch.int32, device="cuda"), torch.zeros((n, mstride, 4), device="cuda")
        torch.cuda.synchronize()

        def mesh_calls():
            for b0 in range(0, n, per_call):
                rc = rxr.rxr_generated_meshes_to(ctx, b[b0:].ctypes.data, min(per_call, n - b0), sub, mstride, dc[b0:].data_ptr(), dv[b0:].data_ptr(), sp)
                assert rc == 0, err()

        meshes_us = statistics.median(timed(mesh_calls))
        del dc, dv
        box_counts, counts = dev[0].cpu().numpy().view(np.uint32), dev[1].cpu().numpy().view(np.uint32).reshape(n, mg, 2)
        triangles = int(counts[:, :, 1].sum())
        med = statistics.median(us)
        line = dict(case=name, subdivisions=sub, tiles=n_tiles, sectors=n_sectors, boxes=n, calls=n_calls, rounds=rounds, max_groups=mg, vertex_stride=vs,
                    triangle_stride=ts, groups=int(box_counts[:, 3].sum()), triangles=triangles, vertices=int(counts[:, :, 0].sum()), us_median=round(med, 1),
                    us_min=round(min(us), 1), us_max=round(max(us), 1), reps=args.reps, ns_per_triangle=round(med * 1e3 / max(triangles, 1), 3),
                    meshes_only_us=round(meshes_us, 1), partition_factor=round(med / meshes_us, 2))
        if n == 1:
            line.update(blocking_us_median=round(wall(lambda: gen.generate_tile_meshes(b, mg, vs, ts), 3), 1))
        if not args.no_cpu:
            key = (name.split("_sub")[1], n)   # (all_x256 and calls_x256 of one configuration share the CPU's answer and time)
            if cpu_cache.get("key") != key:
                cpu_cache.clear()
                cpu_cache.update(key=key, out=gen.generate_tile_meshes_cpu(b, mg, vs, ts), us=wall(lambda: gen.generate_tile_meshes_cpu(b, mg, vs, ts), args.cpu_reps))
            cpu, cpu_us = cpu_cache["out"], cpu_cache["us"]
            got = [d.cpu().numpy() for d in dev]
            assert np.array_equal(cpu[0], box_counts) and np.array_equal(cpu[1], counts), f"{name}: the device's counts differ from the CPU mirror's"
            assert np.array_equal(cpu[2], got[2].view(np.uint32).reshape(n, mg)), f"{name}: group_tiles differ"
            v, uv, idx = got[3].reshape(n, mg, vs, 4), got[4].reshape(n, mg, vs, 2), got[5].view(np.uint32).reshape(n, mg, ts, 3)
            for i in range(n):
                for g in range(int(box_counts[i, 3])):
                    nv, nt = int(counts[i, g, 0]), int(counts[i, g, 1])
                    same = (np.array_equal(v[i, g, :nv].view(np.uint32), cpu[3][i, g, :nv].view(np.uint32)) and np.array_equal(uv[i, g, :nv].view(np.uint32), cpu[4][i, g, :nv].view(np.uint32))
                            and np.array_equal(idx[i, g, :nt], cpu[5][i, g, :nt]))
                    assert same, f"{name}: box {i} group {g} differs from the CPU mirror"
            line.update(cpu_us=round(cpu_us, 1), cpu_threads=CPU_THREADS, speedup_vs_cpu=round(cpu_us / med, 2), bit_equal=True)
            if n == 1:
                line.update(blocking_speedup_vs_cpu=round(cpu_us / line["blocking_us_median"], 2))
        print(json.dumps(line), flush=True)
        del dev

    def stroke(name, gen, sub, n_tiles, chunks, dirty):
        """`dirty` chunks of the registered scene: the chain on one stream against the host route's lower bound"""
        if args.only and args.only not in name:
            return
        b = np.ascontiguousarray(np.asarray(chunks, F).reshape(-1, 4))
        n, mg = len(b), n_tiles
        vs, ts = strides(sub, 0)
        m = n * mg
        host = gen.generate_tile_meshes(b, mg, vs, ts)   # (registers the lists too)
        box_counts, counts, group_tiles, v, uv, idx = (np.ascontiguousarray(a) for a in host)
        assert (box_counts[:, 3] == mg).all()
        nr = np.zeros((m, vs, 3), F)
        flat = lambda a: a.reshape((m,) + a.shape[2:])
        c2, v2, uv2, idx2 = flat(counts), flat(v), flat(uv), flat(idx)

        def normals():
            assert rxr.rxr_vertex_normals(ctx, m, c2.ctypes.data, v2.ctypes.data, idx2.ctypes.data, nr.ctypes.data, vs, ts) == 0, err()

        arr = (Mesh3D * m)()   # (the arrays are updated in place below: the records are filled once)
        for k, a in enumerate(arr):
            a.vertices, a.indices, a.uvs, a.normals = v2[k].ctypes.data, idx2[k].ctypes.data, uv2[k].ctypes.data, nr[k].ctypes.data
            a.n_vertices, a.n_triangles = int(c2[k, 0]), int(c2[k, 1])
            a.transform_3d = IDENTITY
            a.source.kind = B.SOURCE_PIXEL
            a.source.pixel = (C.c_uint8 * 4)(90, 160, 90, 255)
            a.shader, a.list, a.chunk = -1, 3, -1

        def register():
            assert rxr.rxr_set_meshes(ctx, C.cast(arr, C.c_void_p), m) == 0, err()

        normals()
        register()
        k = len(dirty)
        db = np.ascontiguousarray(b[dirty])
        named = np.ascontiguousarray(np.concatenate([np.arange(i * mg, (i + 1) * mg) for i in dirty]), np.uint32)
        dev = device_arrays(k, mg, vs, ts)
        dn = torch.zeros((k * mg, vs, 3), device="cuda")
        torch.cuda.synchronize()

        def chain():
            p = [d.data_ptr() for d in dev]
            assert rxr.rxr_generated_tile_meshes_to(ctx, db.ctypes.data, k, sub, mg, vs, ts, *p, sp) == 0, err()
            assert rxr.rxr_vertex_normals_to(ctx, k * mg, p[1], p[3], p[5], dn.data_ptr(), None, vs, ts, sp) == 0, err()
            assert rxr.rxr_update_meshes_to(ctx, named.ctypes.data, k * mg, p[1], p[3], p[5], dn.data_ptr(), vs, ts, sp) == 0, err()

        def host_route():
            out = gen.generate_tile_meshes(db, mg, vs, ts)
            for i, d in enumerate(dirty):   # the dirty chunks' new arrays into the scene's
                v[d], idx[d] = out[3][i], out[5][i]
            normals()
            register()

        for _ in range(args.warmup):
            chain()
        chain_us = wall(chain, args.reps)
        host_us = wall(host_route, max(args.cpu_reps, 3))
        print(json.dumps(dict(case=name, subdivisions=sub, tiles=n_tiles, sectors=0, scene_meshes=m, dirty_chunks=k, updated_meshes=k * mg, chain_wall_us_median=round(chain_us, 1),
                              host_route_wall_us_median=round(host_us, 1), host_route="rxr_generated_tile_meshes + rxr_vertex_normals (host arrays) + rxr_set_meshes of the scene: a lower bound",
                              speedup_vs_host_route=round(host_us / chain_us, 2), reps=args.reps)), flush=True)

    chunks = [(32.0 * x, 32.0 * y, 32.0 * x + 32.0, 32.0 * y + 32.0) for y in range(16) for x in range(16)]
    kw = EB.generator_lists()
    for sub in (1, 4):
        for n_tiles, n_sectors in ((1, 0), (4, 0), (4, 8)):
            gen = api.TerrainGenerator(**kw, subdivisions=sub)
            sb, off, vt = EB.sectors(n_sectors, 4)
            gen.set_exclusions(sb, off, vt)
            cells, slots = stripes(n_tiles)
            gen.set_tiles(cells, slots, n_tiles)
            active = [int(((sb[:, 0] <= c[2]) & (sb[:, 2] >= c[0]) & (sb[:, 1] <= c[3]) & (sb[:, 3] >= c[1])).sum()) for c in chunks] if n_sectors else [0] * len(chunks)
            busiest = int(np.argmax(active))
            tag = f"sub{sub}_t{n_tiles}_s{n_sectors}"
            case(f"all_x256_{tag}", gen, sub, n_tiles, n_sectors, chunks, len(chunks))
            case(f"calls_x256_{tag}", gen, sub, n_tiles, n_sectors, chunks, 1)
            case(f"chunk_{tag}", gen, sub, n_tiles, n_sectors, chunks[busiest:busiest + 1], 1)
        if sub == 1:
            gen = api.TerrainGenerator(**kw, subdivisions=sub)
            cells, slots = stripes(4)
            gen.set_tiles(cells, slots, 4)
            stroke("stroke_x1_sub1_t4_s0", gen, sub, 4, chunks, [100])
            stroke("stroke_x16_sub1_t4_s0", gen, sub, 4, chunks, list(range(96, 112)))


if __name__ == "__main__":
    main()
