#!/usr/bin/env python3
"""Timing of the terrain bake on the device (rxr_bake_terrain_to) against the host mirror's CPU Terrain::bake_chunk: one JSON line
per case.

    python tools/terrain_bench.py [--reps 10] [--warmup 2] [--cpu-reps 3] [--only SUBSTRING]

--only runs the cases whose name contains SUBSTRING (for a profiler run of one case).

Cases: one chunk of 16 x 16 tiles at 64 px per tile (1024 x 1024 texels) with every cell None, Blend(2) (81 taps a texel) and Blend(8)
(1 089 taps); 64 chunks at 16 px per tile with Blend(2) in one call, and the same 64 chunks as 64 calls.  Every case is first baked once
on the device and once on the CPU and the two compared byte for byte; a difference ends the run.  stream_us: events around `reps`
calls on a stream after warm-up, outputs staying on the device, median over three such rounds -- the time a caller's stream is busy per
call set, which INCLUDES launch and host issue overhead (it dominates the None case and the 64-call case); the kernel's own time
comes from a `rocprofv3 --kernel-trace --stats` run of this tool (profiles/terrain/README.md).  CPU baseline: the mirror's bake_chunk
over its worker pool of CPU_THREADS = 16 threads, the CPUs a GPU job may use (RXR_HOST_THREADS is set to it before the pool
starts; median of `cpu-reps`) -- never the code under test.  Each case is then timed
again with RXR_TERRAIN_NAIVE=1, the kernel's plain per-lane loop with every tap's own divisions: the A-B of the separable set-up."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cpu-reps", type=int, default=3)
    ap.add_argument("--only", default="")
    args = ap.parse_args()

    os.environ["RXR_HOST_THREADS"] = str(CPU_THREADS)      # read once, when the mirror's worker pool starts

    import torch

    import rusterix_amd
    from tests import terrain_ref as R

    api = rusterix_amd.load()
    rxr = rusterix_amd.rxr_abi()
    ctx = C.c_void_p(api.lib.rxh_context())
    stream = torch.cuda.Stream()
    sp = C.c_void_p(stream.cuda_stream)

    def case(name, spec, coords, ppt, calls):
        if args.only and args.only not in name:
            return
        terrain = spec.product(api)
        cc = np.ascontiguousarray(np.asarray(coords, np.int32).reshape(-1, 2))
        n, side = len(cc), spec.chunk_size * ppt
        steps = max([int(np.ceil(b[1] / (min(spec.scale) * 0.5))) for b in spec.blends.values()] or [0])
        taps_per_texel = (2 * steps + 1) ** 2 if spec.blends else 1
        # the baseline, and the comparison that licenses the timing
        cpu_s, cpu = [], None
        for _ in range(args.cpu_reps):
            t0 = time.perf_counter()
            cpu = [np.asarray(terrain.bake_chunk(tuple(c), ppt).data).reshape(side, side, 4) for c in cc]
            cpu_s.append(time.perf_counter() - t0)
        got = terrain.bake_chunks(cc, ppt)           # (registers the terrain: rxr_set_terrain)
        for i in range(n):
            assert np.array_equal(got[i], cpu[i]), f"{name}: chunk {i}: {R.first_difference(got[i], cpu[i])}"
        dev = torch.empty((n, side, side, 4), dtype=torch.uint8, device="cuda")
        per = n // calls

        def run():
            for i in range(calls):
                rc = rxr.rxr_bake_terrain_to(ctx, cc[i * per:].ctypes.data, per, ppt, dev.data_ptr() + i * per * side * side * 4, sp)
                assert rc == 0, rxr.rxr_last_error(ctx)

        def timed():
            for _ in range(args.warmup):
                run()
            stream.synchronize()
            rounds = []
            for _ in range(3):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(args.reps):
                    run()
                e1.record(stream)
                stream.synchronize()
                rounds.append(e0.elapsed_time(e1) * 1000.0 / args.reps)
            assert rxr.rxr_synchronize(ctx) == 0, rxr.rxr_last_error(ctx)
            return statistics.median(rounds)

        us = timed()
        launches = rxr.rxr_debug_terrain_launches(ctx)
        assert np.array_equal(dev.cpu().numpy(), got), name
        os.environ["RXR_TERRAIN_NAIVE"] = "1"
        naive_us = timed()
        assert np.array_equal(dev.cpu().numpy(), got), name + " (plain loop)"
        del os.environ["RXR_TERRAIN_NAIVE"]
        texels = n * side * side
        print(json.dumps(dict(case=name, chunks=n, side=side, calls=calls, taps_per_texel=taps_per_texel, launches_last_call=launches,
                              stream_us=round(us, 1), ps_per_tap=round(us * 1e6 / (texels * taps_per_texel), 3),
                              plain_loop_us=round(naive_us, 1), separable_speedup=round(naive_us / us, 2),
                              cpu_ms=round(statistics.median(cpu_s) * 1e3, 2), cpu_threads=CPU_THREADS,
                              speedup_vs_cpu=round(statistics.median(cpu_s) * 1e6 / us, 1), byte_identical=True)), flush=True)

    case("1x1024x1024_none", R.uniform_scene(R.NONE, 0, 16), [(0, 0)], 64, 1)
    case("1x1024x1024_blend2", R.uniform_scene(R.RADIUS, 2, 16), [(0, 0)], 64, 1)
    case("1x1024x1024_blend8", R.uniform_scene(R.RADIUS, 8, 16), [(0, 0)], 64, 1)
    grid = [(x, y) for y in range(8) for x in range(8)]
    many = R.uniform_scene(R.RADIUS, 2, 16, chunks=8)
    case("64x256x256_blend2_one_call", many, grid, 16, 1)
    case("64x256x256_blend2_64_calls", many, grid, 16, 64)


if __name__ == "__main__":
    main()
