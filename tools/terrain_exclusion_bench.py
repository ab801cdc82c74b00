#!/usr/bin/env python3
"""Timing of the generated terrain's chunk meshes on the device (rxr_generated_meshes_to and its blocking form: grid, heights and
apply_exclusions) against the host mirror's CPU generate_meshes_cpu (the same three steps): one JSON line per case.

    python tools/terrain_exclusion_bench.py [--reps 10] [--warmup 2] [--cpu-reps 1] [--only SUBSTRING] [--no-cpu]

--only runs the cases whose name contains SUBSTRING (for a profiler run of one case).

Cases, over a 512 x 512 map of 16 x 16 chunks with 16 control points (no powf: every word of the device's answer must equal the
CPU's), at subdivisions 1 (33 x 33 points a chunk) and 4 (129 x 129), with 0, 8 and 256 excluded sectors -- regular polygons of 4
or of 64 vertices, radius 6 to 14, both windings:
  all_x256     the 256 chunks in ONE rxr_generated_meshes_to call
  chunk        one chunk (the one with the most active sectors)
  calls_x256   the same chunks as 256 calls of one box each, queued back to back on one stream
Every case is first run on the device and on the CPU and compared word for word.  us: events around the case's calls on a stream,
outputs staying on the device; median, minimum and maximum over `reps` -- this includes the launches' fixed part.  blocking_us: wall
time of the blocking form with host arrays.  CPU baseline: the mirror's generate_meshes_cpu over its worker pool of CPU_THREADS = 16
threads, the CPUs a GPU job may use (RXR_HOST_THREADS is set to it before the pool starts; median of `cpu-reps`) -- never the code
under test."""
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
CPU_THREADS = 16
F = np.float32
MAP = 512.0


def generator_lists():
    rng = np.random.default_rng(16)
    cps = np.column_stack([rng.uniform(0, MAP, 16), rng.uniform(0, MAP, 16), rng.uniform(0.5, 8.0, 16), rng.uniform(1.0, 12.0, 16)])
    return dict(control_points=cps, map_box=(0.0, 0.0, MAP, MAP))


def sectors(n, n_vertices):
    """n regular polygons: (sector_boxes [n][4], vertex_offsets [n + 1], vertices [n * n_vertices][2])"""
    rng = np.random.default_rng([n, n_vertices])
    boxes, verts = [], []
    for s in range(n):
        cx, cy, r, phase = rng.uniform(16, MAP - 16), rng.uniform(16, MAP - 16), rng.uniform(6, 14), rng.uniform(0, 6.283)
        ang = phase + np.arange(n_vertices) * (2 * np.pi / n_vertices) * (1 if s % 2 else -1)
        p = np.column_stack([cx + r * np.cos(ang), cy + r * np.sin(ang)]).astype(F)
        verts.append(p)
        boxes.append((p[:, 0].min(), p[:, 1].min(), p[:, 0].max(), p[:, 1].max()))
    off = np.arange(n + 1, dtype=np.uint32) * n_vertices
    return np.array(boxes, F).reshape(-1, 4), off, (np.concatenate(verts) if n else np.zeros((0, 2), F))


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

    api = rusterix_amd.load()
    rxr = rusterix_amd.rxr_abi()
    ctx = C.c_void_p(api.lib.rxh_context())
    stream = torch.cuda.Stream()
    sp = C.c_void_p(stream.cuda_stream)

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
        assert rxr.rxr_synchronize(ctx) == 0, rxr.rxr_last_error(ctx)
        return us

    def wall(call, reps):
        out = []
        for _ in range(reps):
            t0 = time.perf_counter()
            call()
            out.append((time.perf_counter() - t0) * 1e6)
        return statistics.median(out)

    cpu_cache = {}

    def case(name, gen, sub, n_sectors, n_vertices, boxes, per_call):
        if args.only and args.only not in name:
            return
        b = np.ascontiguousarray(np.asarray(boxes, F).reshape(-1, 4))
        n, steps = len(b), 32 * sub + 1
        stride = 6 * (steps - 1) * (steps - 1)
        gen.generate_meshes(b[:1], stride)   # registers the lists on the mirror's context
        dc = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
        dv = torch.zeros((n, stride, 4), device="cuda")
        torch.cuda.synchronize()

        def calls():
            for b0 in range(0, n, per_call):
                rc = rxr.rxr_generated_meshes_to(ctx, b[b0:].ctypes.data, min(per_call, n - b0), sub, stride, dc[b0:].data_ptr(), dv[b0:].data_ptr(), sp)
                assert rc == 0, rxr.rxr_last_error(ctx)

        us = timed(calls)
        n_calls = (n + per_call - 1) // per_call
        rounds = rxr.rxr_debug_terrain_excl_launches(ctx) * n_calls
        counts = dc.cpu().numpy().view(np.uint32)
        assert (counts[:, :2] == steps).all()
        triangles = n * 2 * (steps - 1) * (steps - 1)
        unshared = counts[:, 2] > 0
        kept = int(counts[unshared, 3].sum() // 3) + int((~unshared).sum()) * 2 * (steps - 1) * (steps - 1)

        def blocking_call():
            for b0 in range(0, n, per_call):
                gen.generate_meshes(b[b0:b0 + per_call], stride)

        blocking = wall(blocking_call, 3)
        med = statistics.median(us)
        line = dict(case=name, subdivisions=sub, sectors=n_sectors, sector_vertices=n_vertices, boxes=n, calls=n_calls, rounds=rounds, points=n * steps * steps,
                    triangles=triangles, dropped=triangles - kept, most_active=int(counts[:, 2].max()), us_median=round(med, 1), us_min=round(min(us), 1),
                    us_max=round(max(us), 1), reps=args.reps, ns_per_triangle=round(med * 1e3 / triangles, 3), blocking_us_median=round(blocking, 1))
        if not args.no_cpu:
            key = (name.split("_sub")[1], n)   # (all_x256 and calls_x256 of one configuration share the CPU's answer and time)
            if cpu_cache.get("key") != key:
                cpu_cache.clear()
                cpu_cache.update(key=key, out=gen.generate_meshes_cpu(b, stride), us=wall(lambda: gen.generate_meshes_cpu(b, stride), args.cpu_reps))
            (ccounts, cv), cpu_us = cpu_cache["out"], cpu_cache["us"]
            assert np.array_equal(ccounts, counts), f"{name}: the device's counts differ from the CPU mirror's"
            v = dv.cpu().numpy()
            for i in range(n):
                k = int(counts[i, 3])
                assert np.array_equal(v[i, :k].view(np.uint32), cv[i, :k].view(np.uint32)), f"{name}: box {i} differs from the CPU mirror"
            line.update(cpu_us=round(cpu_us, 1), cpu_threads=CPU_THREADS, speedup_vs_cpu=round(cpu_us / med, 2), blocking_speedup_vs_cpu=round(cpu_us / blocking, 2),
                        bit_equal=True)
        print(json.dumps(line), flush=True)
        del dv

    chunks = [(32.0 * x, 32.0 * y, 32.0 * x + 32.0, 32.0 * y + 32.0) for y in range(16) for x in range(16)]
    kw = generator_lists()
    for sub in (1, 4):
        for n_sectors, n_vertices in ((0, 4), (8, 4), (8, 64), (256, 4), (256, 64)):
            gen = api.TerrainGenerator(**kw, subdivisions=sub)
            sb, off, vt = sectors(n_sectors, n_vertices)
            gen.set_exclusions(sb, off, vt)
            active = [int(((sb[:, 0] <= c[2]) & (sb[:, 2] >= c[0]) & (sb[:, 1] <= c[3]) & (sb[:, 3] >= c[1])).sum()) for c in chunks] if n_sectors else [0] * len(chunks)
            busiest = int(np.argmax(active))
            tag = f"sub{sub}_s{n_sectors}" + (f"_v{n_vertices}" if n_sectors else "")
            case(f"all_x256_{tag}", gen, sub, n_sectors, n_vertices, chunks, len(chunks))
            case(f"calls_x256_{tag}", gen, sub, n_sectors, n_vertices, chunks, 1)
            case(f"chunk_{tag}", gen, sub, n_sectors, n_vertices, chunks[busiest:busiest + 1], 1)


if __name__ == "__main__":
    main()
