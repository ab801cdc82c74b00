#!/usr/bin/env python3
"""Timing of the terrain chunk meshes on the device (rxr_terrain_meshes_to, rxr_terrain_meshes) against the host mirror's CPU
Terrain::build_mesh: one JSON line per case.

    python tools/terrain_mesh_bench.py [--reps 20] [--warmup 3] [--cpu-reps 3] [--only SUBSTRING] [--no-cpu]

--only runs the cases whose name contains SUBSTRING (for a profiler run of one case).

Cases, over a rolling height field in which every cell is listed:
  chunk16          one chunk of 16 x 16 cells, the editor's unit after a brush stroke
  chunks16_x1024   the 1 024 chunks of a 512 x 512-cell terrain in ONE call (four launches of 256 workgroups)
  calls16_x1024    the same chunks as 1 024 calls of one chunk each, queued back to back on one stream
  chunk64          one chunk of 64 x 64 cells, the bound
Every case is first run on the device and on the CPU and the meshes compared bit for bit; a difference ends the run.  us: events
around the case's calls on a stream, outputs staying on the device (rxr_terrain_meshes_to); median, minimum and maximum over `reps`
-- this includes the launches' fixed part.  blocking_us: wall time of rxr_terrain_meshes with host arrays (the three geometry
arrays go up and come down).  CPU baseline: the mirror's build_mesh per chunk over its worker pool of CPU_THREADS = 16 threads,
the CPUs a GPU job may use (RXR_HOST_THREADS is set to it before the pool starts; median of `cpu-reps`) -- never the code under
test; it includes making the Batch3D objects, which the device path's caller does as well."""
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

    def field(cells, cs):
        """cells x cells listed cells, and one more row and column so that the last chunks' rim reads heights too"""
        t = api.Terrain((1.0, 1.0), cs)
        rng = np.random.default_rng(1)
        ys, xs = np.mgrid[0:cells + 1, 0:cells + 1]
        h = (2.0 * np.sin(xs / 9.0) * np.cos(ys / 7.0) + 1.5 * np.sin((xs + ys) / 23.0) + rng.uniform(-0.2, 0.2, xs.shape)).astype(F)
        for y in range(cells + 1):
            for x in range(cells + 1):
                t.set_height(x, y, float(h[y, x]))
        return t

    def case(name, terrain, coords, per_call):
        if args.only and args.only not in name:
            return
        cs = terrain.chunk_size
        cc = np.ascontiguousarray(np.asarray(coords, np.int32).reshape(-1, 2))
        n = len(cc)
        vs, ts = (cs + 1) ** 2, 2 * cs * cs
        terrain.build_meshes([coords[0]])                   # registers the terrain's heights on the mirror's context
        counts = torch.zeros((n, 2), dtype=torch.int32, device="cuda")
        vertices, normals = torch.zeros((n, vs, 4), device="cuda"), torch.zeros((n, vs, 3), device="cuda")
        indices = torch.zeros((n, ts, 3), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()

        def calls():
            for c0 in range(0, n, per_call):
                rc = rxr.rxr_terrain_meshes_to(ctx, cc[c0:].ctypes.data, min(per_call, n - c0), cs, counts[c0:].data_ptr(), vertices[c0:].data_ptr(),
                                               indices[c0:].data_ptr(), normals[c0:].data_ptr(), sp)
                assert rc == 0, rxr.rxr_last_error(ctx)

        for _ in range(args.warmup):
            calls()
        stream.synchronize()
        launches = rxr.rxr_debug_terrain_mesh_launches(ctx) * ((n + per_call - 1) // per_call)
        got = [a.cpu().numpy() for a in (counts, vertices, indices, normals)]
        cpu_s = []
        if not args.no_cpu:
            for _ in range(args.cpu_reps):
                t0 = time.perf_counter()
                cpu = terrain.build_meshes_cpu(cc)
                cpu_s.append(time.perf_counter() - t0)
            for i, b in enumerate(cpu):
                v, idx, _, nrm = b.geometry()
                assert got[0][i].tolist() == [len(v), len(idx)], f"{name}: chunk {i}: counts differ from the CPU mirror's"
                for a, w in ((got[1][i][: len(v)], v), (got[2][i][: len(idx)], idx), (got[3][i][: len(v)], nrm)):
                    assert np.array_equal(np.ascontiguousarray(a).view(np.uint32), w.view(np.uint32)), f"{name}: chunk {i} differs from the CPU mirror's"
        us = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            calls()
            e1.record(stream)
            stream.synchronize()
            us.append(e0.elapsed_time(e1) * 1000.0)
        assert rxr.rxr_synchronize(ctx) == 0, rxr.rxr_last_error(ctx)
        # the blocking form with host arrays, as the mirror's build_meshes calls it
        host = [np.zeros((n, 2), np.uint32), np.zeros((n, vs, 4), F), np.zeros((n, ts, 3), np.uint32), np.zeros((n, vs, 3), F)]
        blocking = []
        for _ in range(max(args.reps // 4, 3)):
            t0 = time.perf_counter()
            for c0 in range(0, n, per_call):
                rc = rxr.rxr_terrain_meshes(ctx, cc[c0:].ctypes.data, min(per_call, n - c0), cs, *(a[c0:].ctypes.data for a in host))
                assert rc == 0, rxr.rxr_last_error(ctx)
            blocking.append((time.perf_counter() - t0) * 1e6)
        med = statistics.median(us)
        out_bytes = int(got[0][:, 0].sum()) * 28 + int(got[0][:, 1].sum()) * 12
        line = dict(case=name, chunks=n, chunk_size=cs, calls=(n + per_call - 1) // per_call, launches=launches, us_median=round(med, 1), us_min=round(min(us), 1),
                    us_max=round(max(us), 1), reps=args.reps, us_per_chunk=round(med / n, 3), triangles=int(got[0][:, 1].sum()),
                    output_gb_per_s=round(out_bytes / med / 1e3, 2), blocking_us_median=round(statistics.median(blocking), 1))
        if cpu_s:
            cpu_us = statistics.median(cpu_s) * 1e6
            line.update(cpu_us=round(cpu_us, 1), cpu_threads=CPU_THREADS, speedup_vs_cpu=round(cpu_us / med, 2),
                        blocking_speedup_vs_cpu=round(cpu_us / statistics.median(blocking), 2), bit_identical=True)
        print(json.dumps(line), flush=True)

    t16 = field(512, 16)
    all16 = [(x, y) for y in range(32) for x in range(32)]
    case("chunk16", t16, [(7, 5)], 1)
    case("chunks16_x1024", t16, all16, len(all16))
    case("calls16_x1024", t16, all16, 1)
    case("chunk64", field(64, 64), [(0, 0)], 1)


if __name__ == "__main__":
    main()
