#!/usr/bin/env python3
"""Timing of the flattened terrain heights on the device (rxr_flatten_terrain_to, rxr_flatten_terrain) against the host mirror's CPU
Terrain::process_heights_cpu, and of a height stroke's way to the chunk meshes: one JSON line per case.

    python tools/terrain_flatten_bench.py [--reps 20] [--warmup 3] [--cpu-reps 3] [--only SUBSTRING] [--no-cpu] [--no-stroke]

--only runs the cases whose name contains SUBSTRING (for a profiler run of one case).

The terrain is 512 x 512 listed cells in 1 024 chunks of 16 x 16.  Op lists:
  ops0          none: the cells are copied
  squares8      8 squares of side 24 spread over the terrain, bevel 2
  polygons256   256 polygons of 64 edges and radius 12 on a 16 x 16 lattice, bevel 1.5
  ..._roads64   the same with one group of 64 road segments across the terrain on top, bevel 2
Per op list:
  all           the 1 024 chunks in ONE call (four launches of 256 workgroups)
  one           one chunk
  calls         the same chunks as 1 024 calls of one chunk each, queued back to back on one stream
Every case is first run on the device and on the CPU and every height word and presence byte compared (a NaN needs a NaN); a
difference ends the run.  us: events around the case's calls on a stream, outputs staying on the device (rxr_flatten_terrain_to);
median, minimum and maximum over `reps` -- this includes the launches' fixed part.  blocking_us: wall time of rxr_flatten_terrain
with host arrays.  CPU baseline: the mirror's dictionary transcription, a chunk a task over its worker pool of CPU_THREADS = 16
threads, the CPUs a GPU job may use (RXR_HOST_THREADS is set to it before the pool starts; median of `cpu-reps`) -- never the code
under test.

stroke_*: wall time from changed heights to built chunk meshes in device memory, d dirty chunks of the 1 024, both routes through the
C ABI on one stream and ended by rxr_synchronize (the rxr_update_meshes_to that follows is the same call in both and is left out):
  device   rxr_set_terrain_heights(chunk.heights) -> rxr_flatten_terrain_to(all 1 024 chunks: a registration resets the processed
           grid) -> rxr_terrain_meshes_to(d chunks) under RXR_TERRAIN_HEIGHTS_PROCESSED
  host     process_heights_cpu(all 1 024 chunks, 16 threads) -> rxr_set_terrain_heights(processed_heights) -> rxr_terrain_meshes_to(d)
Both register every cell, so both send the same bytes over PCIe (pcie_bytes: 12 a listed cell); the op list crosses once, when it
changes (op_bytes), not per stroke."""
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
CELLS, CS = 512, 16


def op_lists():
    from tests import terrain_flatten_ref as R

    def squares8(sc):
        for k in range(8):
            x0, y0 = 30.0 + 60.0 * k, 40.0 + 55.0 * ((k * 3) % 8)
            sc.sector(R.square(x0, y0, x0 + 24.0, y0 + 24.0), bevel=2.0, floor_height=F(0.5 * k - 1.0))

    def polygons256(sc):
        for k in range(256):
            sc.sector(R.polygon(16.0 + 32.0 * (k % 16), 16.0 + 32.0 * (k // 16), 12.0, 64, 0.01 * k), bevel=1.5, floor_height=F(0.01 * k - 1.0))

    def roads64(sc):
        xs = np.linspace(4.0, 508.0, 65).astype(F)
        sc.linedefs([(xs[k], F(200.0 + 90.0 * np.sin(k / 5.0)), xs[k + 1], F(200.0 + 90.0 * np.sin((k + 1) / 5.0)), F(1.0 + 0.02 * k), F(1.0 + 0.02 * (k + 1))) for k in range(64)], bevel=2.0)

    out = {}
    for name, makers in (("ops0", ()), ("squares8", (squares8,)), ("polygons256", (polygons256,)), ("squares8_roads64", (squares8, roads64)),
                         ("polygons256_roads64", (polygons256, roads64)), ("ops0_roads64", (roads64,))):
        sc = R.FlattenScene((1.0, 1.0), CS)
        for m in makers:
            m(sc)
        out[name] = sc
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu-reps", type=int, default=3)
    ap.add_argument("--only", default="")
    ap.add_argument("--no-cpu", action="store_true", help="skip the CPU baseline and the comparison (profiler runs)")
    ap.add_argument("--no-stroke", action="store_true")
    args = ap.parse_args()

    os.environ["RXR_HOST_THREADS"] = str(CPU_THREADS)      # read once, when the mirror's worker pool starts

    import torch

    import rusterix_amd
    from rusterix_amd import abi
    from tests import terrain_flatten_ref as R

    api = rusterix_amd.load()
    rxr = rusterix_amd.rxr_abi()
    ctx = C.c_void_p(api.lib.rxh_context())
    stream = torch.cuda.Stream()
    sp = C.c_void_p(stream.cuda_stream)

    rng = np.random.default_rng(1)
    ys, xs = np.mgrid[0:CELLS, 0:CELLS]
    field = (2.0 * np.sin(xs / 9.0) * np.cos(ys / 7.0) + 1.5 * np.sin((xs + ys) / 23.0) + rng.uniform(-0.2, 0.2, xs.shape)).astype(F)
    xy = np.ascontiguousarray(np.stack([xs.ravel(), ys.ravel()], axis=1).astype(np.int32))
    hh = np.ascontiguousarray(field.ravel())
    scale = np.array([1.0, 1.0], F)
    all_chunks = np.ascontiguousarray(np.array([(x, y) for y in range(CELLS // CS) for x in range(CELLS // CS)], np.int32))
    per = CS * CS

    def register(heights):
        assert rxr.rxr_set_terrain_heights(ctx, scale.ctypes.data, xy.ctypes.data, heights.ctypes.data, len(heights)) == 0, rxr.rxr_last_error(ctx)

    def mirror_of(sc):
        t = api.Terrain((1.0, 1.0), CS)
        for i in range(len(hh)):
            t.set_height(int(xy[i, 0]), int(xy[i, 1]), float(hh[i]))
        keep, _ = sc.arrays()
        return t.set_flatten_ops(keep["kinds"], keep["params"], keep["ranges"], keep["records"])

    terrain = None
    for ops_name, sc in op_lists().items():
        if args.only and args.only not in ops_name and not any(args.only in f"{ops_name}_{k}" for k in ("all", "one", "calls", "stroke")):
            continue
        keep, op_args = sc.arrays()
        op_bytes = sum(a.nbytes for a in keep.values())
        register(hh)
        assert rxr.rxr_set_terrain_flatten(ctx, *op_args) == 0, rxr.rxr_last_error(ctx)
        if not args.no_cpu:
            if terrain is None:
                terrain = mirror_of(sc)
            else:
                terrain.set_flatten_ops(keep["kinds"], keep["params"], keep["ranges"], keep["records"])
        cpu_all = None
        for shape, coords, per_call in (("all", all_chunks, len(all_chunks)), ("one", all_chunks[5 * 32 + 7: 5 * 32 + 8], 1), ("calls", all_chunks, 1)):
            name = f"{ops_name}_{shape}"
            if args.only and args.only not in name:
                continue
            n = len(coords)
            dh = torch.zeros((n, per), dtype=torch.float32, device="cuda")
            dp = torch.zeros((n, per), dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()

            def calls():
                for c0 in range(0, n, per_call):
                    rc = rxr.rxr_flatten_terrain_to(ctx, coords[c0:].ctypes.data, min(per_call, n - c0), CS, dh[c0:].data_ptr(), dp[c0:].data_ptr(), sp)
                    assert rc == 0, rxr.rxr_last_error(ctx)

            for _ in range(args.warmup):
                calls()
            stream.synchronize()
            launches = rxr.rxr_debug_terrain_flatten_launches(ctx) * ((n + per_call - 1) // per_call)
            got_h, got_p = dh.cpu().numpy(), dp.cpu().numpy()
            cpu_s = []
            if not args.no_cpu:
                for _ in range(args.cpu_reps):
                    t0 = time.perf_counter()
                    want_h, want_p = terrain.process_heights_cpu(coords)
                    cpu_s.append(time.perf_counter() - t0)
                d = R.first_difference(got_h, got_p, want_h, want_p)
                assert not d, f"{name}: the device differs from the CPU mirror: {d}"
                if shape == "all":
                    cpu_all = statistics.median(cpu_s)
            us = []
            for _ in range(args.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                calls()
                e1.record(stream)
                stream.synchronize()
                us.append(e0.elapsed_time(e1) * 1000.0)
            assert rxr.rxr_synchronize(ctx) == 0
            host_h, host_p = np.zeros((n, per), F), np.zeros((n, per), np.uint8)
            blocking = []
            if shape != "calls":
                for _ in range(max(args.reps // 4, 3)):
                    t0 = time.perf_counter()
                    assert rxr.rxr_flatten_terrain(ctx, coords.ctypes.data, n, CS, host_h.ctypes.data, host_p.ctypes.data) == 0, rxr.rxr_last_error(ctx)
                    blocking.append((time.perf_counter() - t0) * 1e6)
            med = statistics.median(us)
            changed = int((got_h.view(np.uint32) != field.reshape(32, CS, 32, CS).transpose(0, 2, 1, 3).reshape(-1, per)[: len(got_h)].view(np.uint32)).sum()) if shape != "one" else None
            line = dict(case=name, ops=len(sc.ops), records=int(len(keep["records"])), chunks=n, calls=(n + per_call - 1) // per_call, launches=launches,
                        us_median=round(med, 1), us_min=round(min(us), 1), us_max=round(max(us), 1), reps=args.reps, us_per_chunk=round(med / n, 3), cells_changed=changed)
            if blocking:
                line.update(blocking_us_median=round(statistics.median(blocking), 1))
            if cpu_s:
                cpu_us = statistics.median(cpu_s) * 1e6
                line.update(cpu_us=round(cpu_us, 1), cpu_threads=CPU_THREADS, speedup_vs_cpu=round(cpu_us / med, 2), bit_identical=True)
                if blocking:
                    line.update(blocking_speedup_vs_cpu=round(cpu_us / statistics.median(blocking), 2))
            print(json.dumps(line), flush=True)

        # ---- a height stroke until the dirty chunks' meshes are built ----
        if args.no_stroke or args.no_cpu or (args.only and args.only not in f"{ops_name}_stroke"):
            continue
        vs, ts = (CS + 1) ** 2, 2 * CS * CS
        for dirty in (1, 64, 1024):
            dc = np.ascontiguousarray(all_chunks[:dirty])
            counts = torch.zeros((dirty, 2), dtype=torch.int32, device="cuda")
            vertices, normals = torch.zeros((dirty, vs, 4), device="cuda"), torch.zeros((dirty, vs, 3), device="cuda")
            indices = torch.zeros((dirty, ts, 3), dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()

            def meshes():
                rc = rxr.rxr_terrain_meshes_to(ctx, dc.ctypes.data, dirty, CS, counts.data_ptr(), vertices.data_ptr(), indices.data_ptr(), normals.data_ptr(), None)
                assert rc == 0, rxr.rxr_last_error(ctx)
                assert rxr.rxr_synchronize(ctx) == 0

            def device_route():
                register(hh)
                assert rxr.rxr_set_terrain_height_source(ctx, abi.RXR_TERRAIN_HEIGHTS_PROCESSED) == 0
                assert rxr.rxr_flatten_terrain_to(ctx, all_chunks.ctypes.data, len(all_chunks), CS, None, None, None) == 0, rxr.rxr_last_error(ctx)
                meshes()
                assert rxr.rxr_set_terrain_height_source(ctx, abi.RXR_TERRAIN_HEIGHTS_REGISTERED) == 0

            def host_route():
                ph, pp = terrain.process_heights_cpu(all_chunks)
                assert pp.all()                                           # (every cell is listed: the processed map has the same keys)
                flat = np.ascontiguousarray(ph.reshape(32, 32, CS, CS).transpose(0, 2, 1, 3).reshape(-1))
                register(flat)
                meshes()

            results = {}
            for route, fn in (("device", device_route), ("host", host_route)):
                fn()
                got = [a.cpu().numpy().copy() for a in (counts, vertices, indices, normals)]
                t = []
                for _ in range(max(args.cpu_reps, 3)):
                    t0 = time.perf_counter()
                    fn()
                    t.append((time.perf_counter() - t0) * 1e6)
                results[route] = (statistics.median(t), got)
            for a, b in zip(results["device"][1], results["host"][1]):
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"{ops_name}_stroke_{dirty}: the two routes built different meshes"
            print(json.dumps(dict(case=f"{ops_name}_stroke_{dirty}", dirty_chunks=dirty, device_route_us=round(results["device"][0], 1), host_route_us=round(results["host"][0], 1),
                                  speedup=round(results["host"][0] / results["device"][0], 2), pcie_bytes_device_route=int(len(hh) * 12), pcie_bytes_host_route=int(len(hh) * 12),
                                  op_bytes_once=int(op_bytes), cpu_threads=CPU_THREADS, meshes_identical=True)), flush=True)
        register(hh)
    assert rxr.rxr_set_terrain_flatten(ctx, None, None, None, 0, None, 0) == 0


if __name__ == "__main__":
    main()
