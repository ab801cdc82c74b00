#!/usr/bin/env python3
"""Timing of the generated terrain's height field on the device (rxr_generated_heights_to, rxr_generated_grids_to and their blocking
forms) against the host mirror's CPU TerrainGenerator: one JSON line per case.

    python tools/terrain_gen_bench.py [--reps 20] [--warmup 3] [--cpu-reps 3] [--only SUBSTRING] [--no-cpu]

--only runs the cases whose name contains SUBSTRING (for a profiler run of one case).

Cases, over a 512 x 512 map, each with 16 and with 1 024 control points (c16 / c1024) and without and with 16 ridge squares (64
edges) and 64 linedefs (plain / rl):
  point          one point, the region server's query per entity move
  points4096     4 096 points in one call
  normals4096    the same with sample_normal_at: three samples a point in one launch
  grid33         the 33 x 33 grid of one 32 x 32 chunk
  grids_x256     the 256 chunks of the map in ONE rxr_generated_grids_to call (278 784 points)
  calls_x256     the same chunks as 256 calls of one box each, queued back to back on one stream
Every case is first run on the device and on the CPU and compared: where they differ (only behind a powf) the largest difference is
reported; more than 1e-3 ends the run.  us: events around the case's calls on a stream, outputs staying on the device; median,
minimum and maximum over `reps` -- this includes the launches' fixed part.  blocking_us: wall time of the blocking form with host
arrays.  CPU baseline: the mirror's sample_height_at over its worker pool of CPU_THREADS = 16 threads, the CPUs a GPU job may use
(RXR_HOST_THREADS is set to it before the pool starts; median of `cpu-reps`) -- never the code under test."""
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


def lists(n_control, features):
    rng = np.random.default_rng([n_control, int(features)])
    cps = np.column_stack([rng.uniform(0, MAP, n_control), rng.uniform(0, MAP, n_control), rng.uniform(0.5, 8.0, n_control), rng.uniform(1.0, 12.0, n_control)])
    ridges, offsets, edges, lines = [], [0], [], []
    if features:
        for _ in range(16):
            cx, cy, half = rng.uniform(32, MAP - 32), rng.uniform(32, MAP - 32), rng.uniform(4, 16)
            corners = [(cx - half, cy - half), (cx + half, cy - half), (cx + half, cy + half), (cx - half, cy + half)]
            edges += [(*corners[k], *corners[(k + 1) % 4]) for k in range(4)]
            offsets.append(len(edges))
            ridges.append((rng.uniform(0.5, 3.0), rng.uniform(0.0, 2.0), rng.uniform(8.0, 24.0), rng.uniform(0.5, 3.0)))
        for _ in range(64):
            x, y, a = rng.uniform(0, MAP), rng.uniform(0, MAP), rng.uniform(0, 6.283)
            ln = rng.uniform(16, 96)
            lines.append((x, y, x + ln * np.cos(a), y + ln * np.sin(a), rng.uniform(0, 2), rng.uniform(0, 2), rng.uniform(0.5, 2.0), rng.uniform(4.0, 12.0), rng.uniform(0.5, 3.0)))
    return dict(control_points=cps, ridges=ridges, ridge_edge_offsets=offsets, ridge_edges=edges, linedefs=lines, map_box=(0.0, 0.0, MAP, MAP))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu-reps", type=int, default=3)
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

    def report(name, gen, n_points, n_calls, launches, us, blocking_us, got, cpu_call, records):
        med = statistics.median(us)
        line = dict(case=name, points=n_points, records=records, calls=n_calls, launches=launches, us_median=round(med, 1), us_min=round(min(us), 1),
                    us_max=round(max(us), 1), reps=args.reps, ns_per_point=round(med * 1e3 / n_points, 2),
                    ps_per_point_record=round(med * 1e6 / n_points / max(records, 1), 2), blocking_us_median=round(blocking_us, 1))
        if not args.no_cpu:
            cpu = cpu_call()
            cpu_us = wall(cpu_call, args.cpu_reps)
            same = got.view(np.uint32) == cpu.view(np.uint32)
            diff = float(np.nanmax(np.abs(got.astype(np.float64) - cpu.astype(np.float64)))) if got.size else 0.0
            assert diff <= 1e-3, f"{name}: the device differs from the CPU mirror by {diff}"
            line.update(cpu_us=round(cpu_us, 1), cpu_threads=CPU_THREADS, speedup_vs_cpu=round(cpu_us / med, 2), blocking_speedup_vs_cpu=round(cpu_us / blocking_us, 2),
                        bit_equal_share=round(float(same.mean()), 4), max_abs_difference=diff)
        print(json.dumps(line), flush=True)

    def points_case(name, gen, records, pts, normals):
        if args.only and args.only not in name:
            return
        n = len(pts)
        gen.sample_heights(pts[:1])   # registers the lists on the mirror's context
        dp = torch.from_numpy(pts).cuda()
        dh, dn = torch.zeros(n, device="cuda"), torch.zeros((n, 3), device="cuda")
        torch.cuda.synchronize()

        def calls():
            rc = rxr.rxr_generated_heights_to(ctx, dp.data_ptr(), n, dh.data_ptr(), dn.data_ptr() if normals else None, sp)
            assert rc == 0, rxr.rxr_last_error(ctx)

        us = timed(calls)
        launches = rxr.rxr_debug_terrain_gen_launches(ctx)
        blocking = wall((lambda: gen.sample_normals(pts)) if normals else (lambda: gen.sample_heights(pts)), max(args.reps // 4, 3))
        report(name, gen, n, 1, launches, us, blocking, dh.cpu().numpy(), lambda: (gen.sample_normals_cpu(pts)[0] if normals else gen.sample_heights_cpu(pts)), records)

    def grids_case(name, gen, records, boxes, per_call):
        if args.only and args.only not in name:
            return
        b = np.ascontiguousarray(np.asarray(boxes, F).reshape(-1, 4))
        n, stride = len(b), 33 * 33
        gen.sample_heights(np.zeros((1, 2), F))
        dc = torch.zeros((n, 2), dtype=torch.int32, device="cuda")
        dh = torch.zeros((n, stride), device="cuda")
        torch.cuda.synchronize()

        def calls():
            for b0 in range(0, n, per_call):
                rc = rxr.rxr_generated_grids_to(ctx, b[b0:].ctypes.data, min(per_call, n - b0), 1, stride, dc[b0:].data_ptr(), dh[b0:].data_ptr(), sp)
                assert rc == 0, rxr.rxr_last_error(ctx)

        us = timed(calls)
        n_calls = (n + per_call - 1) // per_call
        launches = rxr.rxr_debug_terrain_gen_launches(ctx) * n_calls
        assert (dc.cpu().numpy() == 33).all()

        def blocking_call():
            for b0 in range(0, n, per_call):
                gen.grid_heights(b[b0:b0 + per_call], stride)

        blocking = wall(blocking_call, max(args.reps // 4, 3))
        report(name, gen, n * stride, n_calls, launches, us, blocking, dh.cpu().numpy(), lambda: gen.grid_heights_cpu(b, stride)[1], records)

    rng = np.random.default_rng(3)
    pts = rng.uniform(0, MAP, (4096, 2)).astype(F)
    chunks = [(32.0 * x, 32.0 * y, 32.0 * x + 32.0, 32.0 * y + 32.0) for y in range(16) for x in range(16)]
    for n_control in (16, 1024):
        for features in (False, True):
            kw = lists(n_control, features)
            gen = api.TerrainGenerator(**kw)
            records = n_control + (64 + 64 if features else 0)
            tag = f"c{n_control}_{'rl' if features else 'plain'}"
            points_case(f"point_{tag}", gen, records, pts[:1], False)
            points_case(f"points4096_{tag}", gen, records, pts, False)
            points_case(f"normals4096_{tag}", gen, 3 * records, pts, True)
            grids_case(f"grid33_{tag}", gen, records, chunks[37:38], 1)
            grids_case(f"grids_x256_{tag}", gen, records, chunks, len(chunks))
            grids_case(f"calls_x256_{tag}", gen, records, chunks, 1)


if __name__ == "__main__":
    main()
