#!/usr/bin/env python3
"""Timing of the path tracer on the device (rxr_trace_to, include/rxr.h): one JSON line per case.

    python tools/trace_bench.py [--samples 4] [--warmup 1] [--out profiles/trace/trace_bench.jsonl]

Cases: the teapot at 1920x1080, a reduced box grid (n = 32: 12 288 triangles) at 960x540 and the tests' small room at 1920x1080, all
matte with one point light, eight bounces.  Per case: stream time per sample (one frame of one sample per pixel) from events after
warm-up, the accumulation buffer already on the device; paths and ray-triangle tests per second counting EVERY slot of every round --
dead paths stay in their slots (rxr_trace.hip), so a round always tests width x height rays against every triangle; the share of the
time a round takes (the same call with 0, 1, 2, 4 and 8 bounces: the differences are the rounds' cost, the 0 the rays and the average);
and the
baseline: the host mirror's CPU path of the same loop (Scene.trace(cpu=True), rusterix_host.cpp) on 16 threads of the same machine, one
sample of the same frame, with the largest difference between the two images (the CPU's cos and sin are the host's)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cpu-threads", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    import rusterix_amd
    from rusterix_amd import scenes
    from rusterix_amd import trace as T
    from tests import intersect_ref as R
    from tests import trace_scenes as S

    api = rusterix_amd.load()
    out = open(args.out, "w") if args.out else None

    def product_scene(builder):
        """the 3D batches of a product scene as matte grey meshes under one light, seen from outside their box"""
        with R.recording(api) as meshes_of:
            cfg = builder(api)
        meshes = [T.mesh(m["vertices"], m["indices"], m["uvs"], m["normals"], list=m["list"], chunk=m.get("chunk", -1), source=S.PIXEL(200, 190, 170),
                         material=(T.MATTE, T.MOD_NONE, 0.7)) for m in meshes_of(cfg.scene) if len(m["indices"])]
        v = np.concatenate([m["vertices"][:, :3] for m in meshes])
        lo, hi = v.min(axis=0), v.max(axis=0)
        centre, size = (lo + hi) / 2, float((hi - lo).max())
        eye = centre + np.array([0.4, 0.5, 1.0], np.float32) * size
        light = S.point_light(tuple(centre + np.array([-0.5, 1.0, 0.6]) * size), intensity=2.0, start=size, end=4 * size)
        scene = dict(meshes=meshes, static_tiles=[], dynamic_tiles=[], lights=[light], sample_mode=0, animation_frame=1)
        return scene, lambda w, h: T.camera_firstp(eye, centre, 60.0, w, h)

    def case(name, scene, camera_of, w, h):
        ntri = sum(len(m["indices"]) for m in scene["meshes"])
        with T.Tracer() as tr:
            S.load(tr, scene)
            kind, consts = camera_of(w, h)
            acc = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            stream = torch.cuda.Stream()

            def timed(bounces):
                def call(first, n):
                    rc = tr.rxr.rxr_trace_to(tr.ctx, kind, consts.ctypes.data, w, h, first, n, 1, bounces, acc.data_ptr(), stream.cuda_stream)
                    assert rc == 0, tr.error()
                call(0, args.warmup)
                stream.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                call(args.warmup, args.samples)
                e1.record(stream)
                stream.synchronize()
                return e0.elapsed_time(e1) * 1000.0 / args.samples

            by_bounces = {b: timed(b) for b in (0, 1, 2, 4, 8)}
            us = by_bounces[8]
            image = acc.cpu().numpy()
        sc, assets = S.mirror_scene(api, S.ordered(scene))
        cpu_acc = api.AccumBuffer(w, h)
        c0 = time.perf_counter()
        sc.trace(camera_of(w, h), cpu_acc, assets, n_frames=1, seed=1, bounces=8, cpu=True, threads=args.cpu_threads)
        cpu_s = time.perf_counter() - c0
        with T.Tracer() as tr:   # (one device sample of the same frame, for the comparison of the images)
            S.load(tr, scene)
            one = T.AccumBuffer(w, h)
            tr.trace(camera_of(w, h), one, n_frames=1, seed=1, bounces=8)
        image_diff = float(np.abs(one.pixels - cpu_acc.pixels).max())
        rec = dict(case=name, width=w, height=h, triangles=ntri, bounces=8, samples=args.samples, device_us_per_sample=round(us, 1),
                   device_us_by_bounces={str(b): round(t, 1) for b, t in by_bounces.items()},
                   round_us=round((by_bounces[8] - by_bounces[4]) / 4, 1), rays_and_accumulate_us=round(by_bounces[0], 1),
                   path_slots_per_s=w * h / (us * 1e-6), tests_per_s=8.0 * w * h * ntri / ((us - by_bounces[0]) * 1e-6),
                   image_mean=[round(float(x), 4) for x in image[..., :3].mean(axis=(0, 1))],
                   cpu_mirror_s_per_sample=round(cpu_s, 3), cpu_threads=args.cpu_threads, cpu_over_device=round(cpu_s / (us * 1e-6), 1),
                   largest_difference_device_cpu=image_diff, cpu_baseline="the host mirror's CPU path (Scene.trace(cpu=True)), one sample of the same frame")
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")

    teapot, teapot_cam = product_scene(lambda a: scenes.teapot_scene(a, 160, 120, 40, logo_size=64))
    case("teapot_1080p", teapot, teapot_cam, 1920, 1080)
    grid, grid_cam = product_scene(lambda a: scenes.box_grid_scene(a, n=32, width=160, height=120))
    case("box_grid_n32_540p", grid, grid_cam, 960, 540)
    room = S.diffuse_room()
    case("room_1080p", room, lambda w, h: S.cameras(w, h)["firstp"], 1920, 1080)
    case("room_64x36", room, lambda w, h: S.cameras(w, h)["firstp"], 64, 36)      # (a thumbnail: launch cost against a CPU's milliseconds)


if __name__ == "__main__":
    main()
