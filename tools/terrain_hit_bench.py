#!/usr/bin/env python3
"""Timing of the terrain pick on the device (rxr_terrain_hits_to) against the host mirror's CPU Terrain::ray_terrain_hit: one JSON
line per case and route.

    python tools/terrain_hit_bench.py [--reps 20] [--warmup 3] [--cpu-reps 3] [--only SUBSTRING] [--no-cpu]

--only runs the cases whose name contains SUBSTRING (for a profiler run of one case).

Cases:
  miss_N     N = 1, 64, 256, 1 024, 4 096, 16 384, 65 536, 262 144 and 1 048 576 rays that run all 1500 steps: they fly level over
             the EMPTY terrain with max_distance = NaN (no height is loaded: every cell lies outside the grid).  The largest fill
             the chip: the time per ray-step the launch bound is derived from.
  field_N    the same rays over a 256 x 256-cell height field they never touch: every step loads a height.
  screen     1920 x 1080 screen rays (rxr_screen_rays_to) from an orbit camera over that field, max_distance 100: the user's size.
Every case is first run on both routes and on the CPU and the arrays compared bit for bit; a difference ends the run.  us: events
around ONE call on a stream, outputs staying on the device, the two routes ALTERNATED call by call in one process after warm-up;
median, minimum and maximum over `reps` -- this includes the launch's fixed part, which the kernel trace of
profiles/terrain_hit/README.md separates.  CPU baseline: the mirror's ray_terrain_hit over its worker pool of CPU_THREADS = 16
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
STEPS = 1500
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
    few = rxr.rxr_debug_terrain_hit_few_rays()

    def field():
        t = api.Terrain((1.0, 1.0), 16)
        rng = np.random.default_rng(1)
        ys, xs = np.mgrid[0:256, 0:256]
        h = (2.0 * np.sin(xs / 9.0) * np.cos(ys / 7.0) + 1.5 * np.sin((xs + ys) / 23.0) + rng.uniform(-0.2, 0.2, xs.shape)).astype(F)
        for y in range(256):
            for x in range(256):
                t.set_height(x, y, float(h[y, x]))
        return t

    terrains = {"miss": api.Terrain((1.0, 1.0), 16), "field": field()}

    def register(terrain):
        # one ray through the mirror registers the terrain's heights (rxr_set_terrain_heights) on the mirror's context
        terrain.ray_terrain_hits(np.zeros((1, 3), F), np.array([[0, 1, 0]], F), 0.0)

    def level_rays(n):
        """rays at y = 50 crossing the field's square, 150 units long at most: no step comes near a height"""
        rng = np.random.default_rng(n)
        o = np.stack([rng.uniform(0, 255, n), np.full(n, 50.0), rng.uniform(0, 255, n)], axis=1).astype(F)
        a = rng.uniform(0, 2 * np.pi, n)
        d = np.stack([np.cos(a), np.zeros(n), np.sin(a)], axis=1).astype(F)
        return o, d

    def case(name, terrain, do, dd, md, routes):
        if args.only and args.only not in name:
            return
        n = do.shape[0]
        register(terrain)
        outs = {}
        for r in routes:
            outs[r] = (torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, device="cuda"), torch.zeros((n, 3), device="cuda"),
                       torch.zeros((n, 2), dtype=torch.int32, device="cuda"))
        torch.cuda.synchronize()

        def call(r):
            os.environ["RXR_TERRAIN_HIT_ROUTE"] = r
            hit, t, wp, gp = outs[r]
            rc = rxr.rxr_terrain_hits_to(ctx, do.data_ptr(), dd.data_ptr(), n, md, hit.data_ptr(), t.data_ptr(), wp.data_ptr(), gp.data_ptr(), sp)
            assert rc == 0, rxr.rxr_last_error(ctx)

        for _ in range(args.warmup):
            for r in routes:
                call(r)
        stream.synchronize()
        launches = {}
        for r in routes:
            call(r)
            n_launch = C.c_uint32(0)
            kernel = rxr.rxr_debug_terrain_hit_kernel(ctx, C.byref(n_launch)).decode()
            assert kernel == "k_terrain_hit_" + r, kernel
            launches[r] = n_launch.value
        stream.synchronize()
        got = {r: tuple(a.cpu().numpy() for a in outs[r]) for r in routes}
        for r in routes[1:]:
            for a, b in zip(got[r], got[routes[0]]):
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"{name}: {r} differs from {routes[0]}"
        cpu_s = []
        if not args.no_cpu:
            o, d = do.cpu().numpy(), dd.cpu().numpy()
            for _ in range(args.cpu_reps):
                t0 = time.perf_counter()
                cpu = terrain.ray_terrain_hits_cpu(o, d, md)
                cpu_s.append(time.perf_counter() - t0)
            for a, key in zip(got[routes[0]], ("hit", "t", "world_pos", "grid_pos")):
                assert np.array_equal(a.view(np.uint32), cpu[key].view(np.uint32)), f"{name}: device {key} differs from the CPU mirror's"
        us = {r: [] for r in routes}
        for _ in range(args.reps):
            for r in routes:                      # alternated: drift of the box hits both alike
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                call(r)
                e1.record(stream)
                stream.synchronize()
                us[r].append(e0.elapsed_time(e1) * 1000.0)
        assert rxr.rxr_synchronize(ctx) == 0, rxr.rxr_last_error(ctx)
        hit_share = float((got[routes[0]][0] != 0).mean())
        steps = n * STEPS if name != "screen" else None
        for r in routes:
            med = statistics.median(us[r])
            line = dict(case=name, rays=n, route=r, launches=launches[r], us_median=round(med, 1), us_min=round(min(us[r]), 1), us_max=round(max(us[r]), 1),
                        reps=args.reps, hit_share=round(hit_share, 3), default_route="wave" if n <= few else "lane")
            if steps:
                line["ps_per_ray_step"] = round(med * 1e6 / steps, 3)
            if cpu_s:
                line.update(cpu_ms=round(statistics.median(cpu_s) * 1e3, 2), cpu_threads=CPU_THREADS, speedup_vs_cpu=round(statistics.median(cpu_s) * 1e6 / med, 1),
                            bit_identical=True)
            print(json.dumps(line), flush=True)
        os.environ.pop("RXR_TERRAIN_HIT_ROUTE", None)

    for kind in ("miss", "field"):
        for n in (1, 64, 256, 1024, 4096, 16384, 65536, 262144, 1048576):
            o, d = level_rays(n)
            case(f"{kind}_{n}", terrains[kind], torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda(), float("nan"), ["lane", "wave"])

    # the user's size: a 1920 x 1080 picking buffer from an editor-like camera over the field
    if not args.only or args.only in "screen":
        w, h = 1920, 1080
        cam = api.D3OrbitCamera.new()
        cam.set_parameter_f32("distance", 60.0)
        cam.center = (128.0, 0.0, 128.0)
        cam.azimuth, cam.elevation = 0.9, 0.7
        view, proj = cam.matrices(float(w), float(h))
        iv, ip, _ = api.Rasterizer.setup(None, view, proj).derived()
        do, dd = torch.zeros((w * h, 3), device="cuda"), torch.zeros((w * h, 3), device="cuda")
        torch.cuda.synchronize()
        rc = rxr.rxr_screen_rays_to(ctx, iv.ctypes.data, ip.ctypes.data, float(w), float(h), 0, 0, w, h, do.data_ptr(), dd.data_ptr(), sp)
        assert rc == 0, rxr.rxr_last_error(ctx)
        stream.synchronize()
        case("screen", terrains["field"], do, dd, 100.0, ["lane", "wave"])


if __name__ == "__main__":
    main()
