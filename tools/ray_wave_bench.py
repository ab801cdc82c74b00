#!/usr/bin/env python3
"""Timing of the wave walk of the ray box tree (rxr_set_ray_wave, include/rxr.h) against the two existing routes in the same session:
one JSON line per cell, stream time from device events after a warm-up of every shape, arrays already on the device (the method of
tools/ray_accel_bench.py).

    python tools/ray_wave_bench.py [--reps 7] [--scenes teapot,grid_n32,grid_1m,terrain] [--rays 1,8,...] [--skip-trace] [--tag TEXT]
                                   [--out profiles/ray_wave/ray_wave_bench.jsonl]

Cells   pinhole rays (1, 8, 64, 256, 1 024, 4 096, 16 384, 65 536 and 1920 x 1080) against the teapot, the 12 288-triangle box grid,
        the 1 M-triangle box grid and a 524 288-triangle terrain of 1 024 chunk meshes.
Routes  brute   both switches off: a thread per triangle up to 64 rays, a thread per ray over triangle slices above
        thread  the tree on, a thread per ray (more than 64 rays only: below, the tree on changes nothing)
        wave    the tree on and RXR_RAY_WAVE_FORCE: a wave per ray
        Within a repetition the routes alternate; a cell's figures are the median, the minimum and the maximum over the repetitions
        of one call's stream time (short calls: the mean of several back-to-back calls a repetition).  Every output word of every
        route is compared with the first route's before a time is recorded.  Brute force is not run where rays x triangles is above
        --brute-cap.
Trace   one sample with eight bounces of the 12 288-triangle grid at 64 x 36 and 960 x 540: tree off, tree on, tree on with
        RXR_RAY_WAVE_ON (the shipped rule).
--tag   copied into every line (the leaf-box A-B runs a second build of the library through RXR_DEVICE_SO).
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
F = np.float32
RAY_SHAPES = {1: (1, 1), 8: (4, 2), 64: (8, 8), 256: (16, 16), 1024: (32, 32), 4096: (64, 64), 16384: (128, 128), 65536: (256, 256),
              1920 * 1080: (1920, 1080)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--scenes", default="teapot,grid_n32,grid_1m,terrain")
    ap.add_argument("--rays", default=",".join(str(n) for n in RAY_SHAPES))
    ap.add_argument("--brute-cap", type=float, default=7e10, help="brute force is skipped above this many ray-triangle tests a call")
    ap.add_argument("--skip-trace", action="store_true")
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.reps >= 5, "at least five repetitions a cell"

    import torch

    import rusterix_amd
    from rusterix_amd import scenes
    from rusterix_amd import trace as T
    from tests import intersect_ref as R
    from tests import trace_scenes as S

    api = rusterix_amd.load()
    out = open(args.out, "a") if args.out else None

    def emit(**rec):
        if args.tag:
            rec["tag"] = args.tag
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    def tmesh(v, idx, uv, nr, lst=T.LIST_STATIC, chunk=-1):
        return T.mesh(v, idx, uv, nr, list=lst, chunk=chunk, source=S.PIXEL(200, 190, 170), material=(T.MATTE, T.MOD_NONE, 0.7))

    def product_scene(builder):
        with R.recording(api) as meshes_of:
            cfg = builder(api)
        return [tmesh(m["vertices"], m["indices"], m["uvs"], m["normals"], m["list"], m.get("chunk", -1)) for m in meshes_of(cfg.scene) if len(m["indices"])]

    def terrain(side=32, chunk=16):
        """side x side chunk meshes of chunk x chunk cells (two triangles a cell) over a smooth height field: tools/ray_refresh_bench.py's"""
        out = []
        i0 = (np.arange(chunk)[:, None] * (chunk + 1) + np.arange(chunk)[None, :]).ravel()
        idx = np.stack([np.stack([i0, i0 + 1, i0 + chunk + 2], 1), np.stack([i0, i0 + chunk + 2, i0 + chunk + 1], 1)], 1).reshape(-1, 3).astype(np.uint32)
        for k in range(side * side):
            xs, zs = np.meshgrid(np.arange(chunk + 1, dtype=F) + (k % side) * chunk, np.arange(chunk + 1, dtype=F) + (k // side) * chunk)
            hgt = (np.sin(xs * 0.05) * np.cos(zs * 0.07) * 6.0 + np.sin(xs * 0.31 + zs * 0.17) * 0.8).astype(F)
            v = np.stack([xs.ravel(), hgt.ravel(), zs.ravel(), np.ones(xs.size, F)], axis=1).astype(F)
            out.append(tmesh(v, idx, v[:, :2].copy(), np.tile(np.array([0, 1, 0], F), (len(v), 1))))
        return out

    def view(meshes):
        v = np.concatenate([m["vertices"][:, :3] for m in meshes])
        lo, hi = v.min(axis=0), v.max(axis=0)
        centre, size = (lo + hi) / 2, float((hi - lo).max())
        return (centre + np.array([0.4, 0.5, 1.0], F) * size).astype(F), centre.astype(F), size

    def pinhole(eye, centre, w, h, fov=60.0):
        """w x h rays of a pinhole camera at `eye` looking at `centre`, row-major"""
        fwd = (centre - eye) / np.linalg.norm(centre - eye)
        right = np.cross(fwd, np.array([0, 1, 0], np.float64))
        right /= np.linalg.norm(right)
        up = np.cross(right, fwd)
        th = np.tan(np.radians(fov) / 2)
        xs = ((np.arange(w) + 0.5) / w * 2 - 1) * th * max(w / h, 1.0)
        ys = (1 - (np.arange(h) + 0.5) / h * 2) * th
        d = fwd[None, None, :] + xs[None, :, None] * right[None, None, :] + ys[:, None, None] * up[None, None, :]
        return np.tile(eye.astype(F), (w * h, 1)), d.reshape(-1, 3).astype(F)

    ROUTES = dict(brute=(T.RAY_ACCEL_OFF, T.RAY_WAVE_OFF), thread=(T.RAY_ACCEL_ON, T.RAY_WAVE_OFF), wave=(T.RAY_ACCEL_ON, T.RAY_WAVE_FORCE))

    class Pick:
        def __init__(self, tr, o, d):
            self.tr, self.n = tr, len(o)
            self.o, self.d = torch.tensor(o, device="cuda"), torch.tensor(d, device="cuda")
            self.t = torch.empty(self.n, dtype=torch.float32, device="cuda")
            self.m = torch.empty(self.n, dtype=torch.int32, device="cuda")
            self.k = torch.empty_like(self.m)
            self.stream = torch.cuda.Stream()
            torch.cuda.synchronize()

        def route(self, name):
            self.tr.ray_accel, self.tr.ray_wave = ROUTES[name]

        def call(self):
            rc = self.tr.rxr.rxr_intersect_to(self.tr.ctx, self.o.data_ptr(), self.d.data_ptr(), self.n, 0, self.t.data_ptr(), self.m.data_ptr(), self.k.data_ptr(),
                                              None, None, None, self.stream.cuda_stream)
            assert rc == 0, self.tr.error()

        def words(self):
            self.stream.synchronize()
            return (self.t.cpu().numpy().view(np.uint32).copy(), self.m.cpu().numpy().copy(), self.k.cpu().numpy().copy())

        def timed(self, calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(self.stream)
            for _ in range(calls):
                self.call()
            e1.record(self.stream)
            self.stream.synchronize()
            return e0.elapsed_time(e1) * 1000.0 / calls

    def stats(xs):
        med, lo, hi = statistics.median(xs), min(xs), max(xs)
        return dict(us=round(med, 1), min_us=round(lo, 1), max_us=round(hi, 1), spread=round((hi - lo) / med, 3))

    def pick_cells(name, meshes, counts):
        ntri = sum(len(m["indices"]) for m in meshes)
        eye, centre, _ = view(meshes)
        with T.Tracer() as tr:
            tr.set_meshes(meshes)
            for n in counts:
                w, h = RAY_SHAPES[n]
                o, d = pinhole(eye, centre, w, h)
                p = Pick(tr, o, d)
                routes = [r for r in ("brute", "thread", "wave") if not (r == "brute" and float(n) * ntri > args.brute_cap) and not (r == "thread" and n <= 64)]
                rec = dict(case=f"pick_{name}_{n}", scene=name, rays=n, triangles=ntri, reps=args.reps)
                ref, calls = None, {}
                for r in routes:      # warm-up of this shape on every route, the comparison of every word, the calls a repetition
                    p.route(r)
                    p.call()
                    got = p.words()
                    if ref is None:
                        ref = got
                    rec[f"{r}_same_words"] = bool(all(np.array_equal(a, b) for a, b in zip(ref, got)))
                    assert rec[f"{r}_same_words"], (name, n, r)
                    calls[r] = int(min(50, max(1, 1500.0 / max(p.timed(1), 1.0))))
                times = {r: [] for r in routes}
                for _ in range(args.reps):
                    for r in routes:
                        p.route(r)
                        times[r].append(p.timed(calls[r]))
                for r in routes:
                    rec[r] = dict(stats(times[r]), calls=calls[r])
                rec["hits"] = int((ref[1] != -1).sum())
                for r in ("thread", "wave"):
                    if r in routes:
                        tr.ray_accel, tr.ray_wave = T.RAY_ACCEL_COUNT, ROUTES[r][1]
                        p.call()
                        p.stream.synchronize()
                        rec[f"{r}_tests_per_ray"] = round(tr.ray_accel_info()["tests"] / n, 1)
                existing = [r for r in ("brute", "thread") if r in routes]
                if existing:      # ahead: by more than twice the larger min-to-max spread of the two
                    best = min(existing, key=lambda r: rec[r]["us"])
                    margin = 2 * max(rec[best]["max_us"] - rec[best]["min_us"], rec["wave"]["max_us"] - rec["wave"]["min_us"])
                    rec["best_existing"] = best
                    rec["wave_over_best"] = round(rec["wave"]["us"] / rec[best]["us"], 3)
                    rec["wave_ahead"] = bool(rec[best]["us"] - rec["wave"]["us"] > margin)
                rec["rule_takes"] = bool(tr.rxr.rxr_ray_wave_takes(n, ntri))
                emit(**rec)
                del p
            tr.ray_accel, tr.ray_wave = T.RAY_ACCEL_OFF, T.RAY_WAVE_OFF

    def trace_cell(name, meshes, w, h, samples=2):
        ntri = sum(len(m["indices"]) for m in meshes)
        eye, centre, size = view(meshes)
        light = S.point_light(tuple(centre + np.array([-0.5, 1.0, 0.6]) * size), intensity=2.0, start=size, end=4 * size)
        scene = dict(meshes=meshes, static_tiles=[], dynamic_tiles=[], lights=[light], sample_mode=0, animation_frame=1)
        modes = dict(tree_off=(T.RAY_ACCEL_OFF, T.RAY_WAVE_OFF), tree_on=(T.RAY_ACCEL_ON, T.RAY_WAVE_OFF), tree_on_wave_on=(T.RAY_ACCEL_ON, T.RAY_WAVE_ON))
        with T.Tracer() as tr:
            S.load(tr, scene)
            kind, consts = T.camera_firstp(eye, centre, 60.0, w, h)
            acc = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            stream = torch.cuda.Stream()

            def run(first, n):
                rc = tr.rxr.rxr_trace_to(tr.ctx, kind, consts.ctypes.data, w, h, first, n, 1, 8, acc.data_ptr(), stream.cuda_stream)
                assert rc == 0, tr.error()

            def timed():
                run(0, 1)
                stream.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                run(1, samples)
                e1.record(stream)
                stream.synchronize()
                return e0.elapsed_time(e1) * 1000.0 / samples

            rec = dict(case=f"trace_{name}_{w}x{h}", triangles=ntri, width=w, height=h, bounces=8, samples=samples, reps=args.reps)
            images, times = {}, {k: [] for k in modes}
            for k, (accel, wave) in modes.items():
                tr.ray_accel, tr.ray_wave = accel, wave
                timed()
                images[k] = acc.cpu().numpy().view(np.uint32).copy()
            rec["same_floats"] = bool(all(np.array_equal(images["tree_off"], x) for x in images.values()))
            assert rec["same_floats"], name
            for _ in range(args.reps):
                for k, (accel, wave) in modes.items():
                    tr.ray_accel, tr.ray_wave = accel, wave
                    times[k].append(timed())
            for k in modes:
                rec[k] = stats(times[k])
            tr.ray_accel, tr.ray_wave = T.RAY_ACCEL_ON, T.RAY_WAVE_ON
            b0 = tr.ray_wave_info()["batches"]
            timed()
            rec["wave_batches_a_call"] = tr.ray_wave_info()["batches"] - b0
            rec["rule_takes_first_round"] = bool(tr.rxr.rxr_ray_wave_takes(w * h, ntri))
            emit(**rec)

    wanted = args.scenes.split(",")
    counts = [int(x) for x in args.rays.split(",") if x]
    builders = dict(teapot=lambda: product_scene(lambda a: scenes.teapot_scene(a, 160, 120, 40, logo_size=64)),
                    grid_n32=lambda: product_scene(lambda a: scenes.box_grid_scene(a, n=32, width=160, height=120)),
                    grid_1m=lambda: product_scene(lambda a: scenes.box_grid_scene(a, width=320, height=200)),
                    terrain=terrain)
    for name in wanted:
        meshes = builders[name]()
        pick_cells(name, meshes, counts)
        if name == "grid_n32" and not args.skip_trace:
            trace_cell(name, meshes, 64, 36)
            trace_cell(name, meshes, 960, 540)
        del meshes


if __name__ == "__main__":
    main()
