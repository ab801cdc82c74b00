#!/usr/bin/env python3
"""Timing of ray picking on the device (rxr_intersect_to, rxr_screen_rays_to): one JSON line per case.

    python tools/intersect_bench.py [--reps 20] [--warmup 3] [--cpu-rays 4]

Cases: 1 ray and 4096 rays x the 1 M-triangle box grid, 1920x1080 screen rays x the teapot and x the map scene.  Per case: device
time per call from events after warm-up (the intersect alone, rays already on the device), rays/s, ray-triangle tests/s, the larger
of two lower bounds -- VALU (an estimate: ~110 fp32 lane-operations per test, the correctly rounded divisions and square root of
the normalisation included, against a 157.3 T lane-ops/s peak) and HBM (36 B of triangle record per pass over the triangles, 8 TB/s)
-- with the one that binds, and a CPU baseline: tests/intersect_ref.py (numpy, one host thread) timed on a few rays and scaled,
labelled as such."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VALU_PEAK = 157.3e12      # fp32 lane-operations per second (MI355X: 256 CUs, 2.4 GHz, 256 fp32 lane-ops per CU and clock)
HBM_PEAK = 8.0e12         # bytes per second
OPS_PER_TEST = 110.0      # VALU lane-operations of one test through to t (division + normalisation share amortised)
BYTES_PER_TRI = 36.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu-rays", type=int, default=4)
    args = ap.parse_args()

    import torch

    import rusterix_amd
    from rusterix_amd import scenes
    from tests import intersect_ref as R

    api = rusterix_amd.load()
    rxr = rusterix_amd.rxr_abi()

    def case(name, builder, rays):
        with R.recording(api) as meshes_of:
            cfg = builder(api)
        meshes = meshes_of(cfg.scene)
        ntri = sum(len(m["indices"]) for m in meshes)
        cfg.scene.intersect(np.zeros((1, 3), np.float32), np.ones((1, 3), np.float32))  # registers the meshes
        ctx = api.lib.rxh_context()
        o, d = rays(cfg, ctx)
        n = o.shape[0]
        stream = torch.cuda.Stream()
        sp = stream.cuda_stream
        t = torch.empty(n, dtype=torch.float32, device="cuda")
        m = torch.empty(n, dtype=torch.int32, device="cuda")
        k = torch.empty_like(m)
        hp = torch.empty((n, 3), dtype=torch.float32, device="cuda")

        def call():
            rc = rxr.rxr_intersect_to(ctx, o.data_ptr(), d.data_ptr(), n, 0, t.data_ptr(), m.data_ptr(), k.data_ptr(), hp.data_ptr(), None, None, sp)
            assert rc == 0, rxr.rxr_last_error(ctx)

        for _ in range(args.warmup):
            call()
        stream.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record(stream)
            for _ in range(args.reps):
                call()
            e1.record(stream)
        stream.synchronize()
        us = e0.elapsed_time(e1) * 1000.0 / args.reps
        tests = float(n) * ntri
        valu_us = tests * OPS_PER_TEST / VALU_PEAK * 1e6
        hbm_us = (ntri * BYTES_PER_TRI * (1 if n <= 64 else max(1, n // 4096)) + n * 40) / HBM_PEAK * 1e6
        # CPU baseline: the numpy restatement on a few of the rays, scaled to all of them
        ho, hd = o.cpu().numpy(), d.cpu().numpy()
        sel = np.linspace(0, n - 1, min(n, args.cpu_rays)).astype(np.int64)
        recs = [R.tri_records(x) for x in meshes]
        c0 = time.perf_counter()
        R.intersect(meshes, ho[sel], hd[sel], records=recs)
        cpu_s = (time.perf_counter() - c0) / len(sel) * n
        hits = int((m.cpu().numpy() != -1).sum())
        print(json.dumps(dict(case=name, rays=n, triangles=ntri, hits=hits, device_us=round(us, 2), rays_per_s=n / (us * 1e-6),
                              tests_per_s=tests / (us * 1e-6), bound_us=round(max(valu_us, hbm_us), 2),
                              bound="VALU" if valu_us >= hbm_us else "HBM", bound_fraction=round(max(valu_us, hbm_us) / us, 3),
                              cpu_numpy_baseline_s=round(cpu_s, 3), cpu_baseline="tests/intersect_ref.py, numpy on one host thread, "
                              f"timed on {len(sel)} rays and scaled")), flush=True)

    def grid_rays(k):
        def rays(cfg, ctx):
            rng = np.random.default_rng(7)
            eye = np.array([28.9, 20.0, 60.0], np.float32)
            target = np.stack([rng.uniform(0, 57.8, k), rng.uniform(0, 0.5, k), rng.uniform(0, 57.8, k)], axis=1).astype(np.float32)
            o = torch.tensor(np.repeat(eye[None], k, axis=0), device="cuda")
            return o, torch.tensor(target - eye[None], device="cuda")
        return rays

    def screen(cfg, ctx):
        r = cfg.setup()
        r.rasterize(cfg.scene, np.zeros(cfg.width * cfg.height * 4, np.uint8), cfg.width, cfg.height, cfg.tile_size, cfg.assets)
        iv, ip, _ = r.derived()
        n = cfg.width * cfg.height
        o = torch.empty((n, 3), dtype=torch.float32, device="cuda")
        d = torch.empty_like(o)
        assert rxr.rxr_screen_rays_to(ctx, iv.ctypes.data, ip.ctypes.data, float(cfg.width), float(cfg.height), 0, 0, cfg.width, cfg.height,
                                      o.data_ptr(), d.data_ptr(), None) == 0
        torch.cuda.synchronize()
        return o, d

    grid = lambda api: scenes.box_grid_scene(api, width=320, height=200)
    case("grid_1ray", grid, grid_rays(1))
    case("grid_4096rays", grid, grid_rays(4096))
    case("teapot_1080p", lambda api: scenes.teapot_scene(api, 1920, 1080, 60, logo_size=64), screen)
    case("map_1080p", lambda api: scenes.map_scene(api, 1920, 1080, 40, logo_size=64), screen)


if __name__ == "__main__":
    main()
