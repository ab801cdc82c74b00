#!/usr/bin/env python3
"""Timing of the ray box tree (rxr_set_ray_accel, include/rxr.h) against the brute-force kernels in the same session: one JSON line per
case, stream time from events after warm-up, arrays already on the device (the method of tools/intersect_bench.py and
tools/trace_bench.py).

    python tools/ray_accel_bench.py [--reps 5] [--samples 2] [--skip-large] [--out profiles/ray_accel/ray_accel_bench.jsonl]

Cases
  build_*        the tree's build for the teapot, the 12 288-triangle box grid and the 1 M-triangle box grid: a 65-ray query right after
                 rxr_set_meshes with the mode on, minus the same query once the tree stands (the records of the picking path are built
                 in both modes; their share is the same query with the mode off, right after rxr_set_meshes, minus its steady time)
  pick_*         pinhole screen rays against the teapot (1920x1080), 65 536 rays and 1920x1080 rays against the 1 M grid (the full
                 buffer with the mode on only), mode off and on, with the tests a ray under RXR_RAY_ACCEL_COUNT
  trace_*        one sample with eight bounces for the four cases of profiles/trace/README.md, mode off and on
  trace_teapot_by_bounces   the same call with 0, 1, 2, 4 and 8 bounces in both modes
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
F = np.float32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--samples", type=int, default=2)
    ap.add_argument("--skip-large", action="store_true", help="without the 1 M-triangle grid")
    ap.add_argument("--skip-trace", action="store_true")
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

    def emit(**rec):
        rec["leaf"], rec["node_width"] = leaf_width
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")

    def product_scene(builder):
        with R.recording(api) as meshes_of:
            cfg = builder(api)
        meshes = [T.mesh(m["vertices"], m["indices"], m["uvs"], m["normals"], list=m["list"], chunk=m.get("chunk", -1), source=S.PIXEL(200, 190, 170),
                         material=(T.MATTE, T.MOD_NONE, 0.7)) for m in meshes_of(cfg.scene) if len(m["indices"])]
        v = np.concatenate([m["vertices"][:, :3] for m in meshes])
        lo, hi = v.min(axis=0), v.max(axis=0)
        centre, size = (lo + hi) / 2, float((hi - lo).max())
        eye = centre + np.array([0.4, 0.5, 1.0], F) * size
        light = S.point_light(tuple(centre + np.array([-0.5, 1.0, 0.6]) * size), intensity=2.0, start=size, end=4 * size)
        scene = dict(meshes=meshes, static_tiles=[], dynamic_tiles=[], lights=[light], sample_mode=0, animation_frame=1)
        return scene, eye.astype(F), centre.astype(F)

    def pinhole(eye, centre, w, h, fov=60.0):
        """w x h rays of a pinhole camera at `eye` looking at `centre`, row-major"""
        fwd = (centre - eye) / np.linalg.norm(centre - eye)
        right = np.cross(fwd, np.array([0, 1, 0], np.float64))
        right /= np.linalg.norm(right)
        up = np.cross(right, fwd)
        th = np.tan(np.radians(fov) / 2)
        xs = ((np.arange(w) + 0.5) / w * 2 - 1) * th * w / h
        ys = (1 - (np.arange(h) + 0.5) / h * 2) * th
        d = fwd[None, None, :] + xs[None, :, None] * right[None, None, :] + ys[:, None, None] * up[None, None, :]
        return np.tile(eye.astype(F), (w * h, 1)), d.reshape(-1, 3).astype(F)

    def info(tr):
        return tr.ray_accel_info()

    class Pick:
        def __init__(self, tr, o, d):
            self.tr, self.n = tr, len(o)
            self.o, self.d = torch.tensor(o, device="cuda"), torch.tensor(d, device="cuda")
            n = self.n
            self.t = torch.empty(n, dtype=torch.float32, device="cuda")
            self.m = torch.empty(n, dtype=torch.int32, device="cuda")
            self.k = torch.empty_like(self.m)
            self.stream = torch.cuda.Stream()
            torch.cuda.synchronize()

        def call(self, n=None):
            n = n or self.n
            rc = self.tr.rxr.rxr_intersect_to(self.tr.ctx, self.o.data_ptr(), self.d.data_ptr(), n, 0, self.t.data_ptr(), self.m.data_ptr(), self.k.data_ptr(),
                                              None, None, None, self.stream.cuda_stream)
            assert rc == 0, self.tr.error()

        def timed(self, reps, n=None, warmup=1):
            for _ in range(warmup):
                self.call(n)
            self.stream.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(self.stream)
            for _ in range(reps):
                self.call(n)
            e1.record(self.stream)
            self.stream.synchronize()
            return e0.elapsed_time(e1) * 1000.0 / reps

    def pick_cases(name, scene, eye, centre, ray_sets):
        """ray_sets: [(label, w, h, with_off)]"""
        ntri = sum(len(m["indices"]) for m in scene["meshes"])
        with T.Tracer() as tr:
            tr.set_meshes(scene["meshes"])
            # build: the first 65-ray query after rxr_set_meshes, minus the steady one, in both modes
            o, d = pinhole(eye, centre, 13, 5)
            p = Pick(tr, o, d)
            first = {}
            for mode in (T.RAY_ACCEL_OFF, T.RAY_ACCEL_ON):
                tr.ray_accel = mode
                p.call()
                p.stream.synchronize()      # (every buffer exists from here on)
                firsts = []
                for _ in range(3):
                    tr.set_meshes(scene["meshes"])
                    firsts.append(p.timed(1, warmup=0))
                first[mode] = (min(firsts), p.timed(args.reps))
            i = info(tr)
            records_us = first[T.RAY_ACCEL_OFF][0] - first[T.RAY_ACCEL_OFF][1]
            emit(case=f"build_{name}", triangles=ntri, nodes=i["nodes"], levels=i["levels"], wild=i["wild"],
                 first_query_off_us=round(first[T.RAY_ACCEL_OFF][0], 1), steady_query_off_us=round(first[T.RAY_ACCEL_OFF][1], 1),
                 first_query_on_us=round(first[T.RAY_ACCEL_ON][0], 1), steady_query_on_us=round(first[T.RAY_ACCEL_ON][1], 1),
                 records_us=round(records_us, 1), tree_build_us=round(first[T.RAY_ACCEL_ON][0] - first[T.RAY_ACCEL_ON][1] - records_us, 1))
            for label, w, h, with_off in ray_sets:
                o, d = pinhole(eye, centre, w, h)
                p = Pick(tr, o, d)
                rec = dict(case=f"pick_{name}_{label}", rays=w * h, triangles=ntri)
                ref = None
                for mode, key in ((T.RAY_ACCEL_OFF, "off"), (T.RAY_ACCEL_ON, "on")):
                    if mode == T.RAY_ACCEL_OFF and not with_off:
                        continue
                    tr.ray_accel = mode
                    rec[f"{key}_us"] = round(p.timed(args.reps if mode else max(1, args.reps // 2)), 1)
                    got = (p.t.cpu().numpy().view(np.uint32).copy(), p.m.cpu().numpy().copy(), p.k.cpu().numpy().copy())
                    if ref is not None:
                        rec["same_words"] = bool(all(np.array_equal(a, b) for a, b in zip(ref, got)))
                    ref = got
                rec["hits"] = int((ref[1] != -1).sum())
                tr.ray_accel = T.RAY_ACCEL_COUNT
                p.call()
                rec["tests_per_ray"] = round(info(tr)["tests"] / (w * h), 2)
                if "off_us" in rec:
                    rec["speedup"] = round(rec["off_us"] / rec["on_us"], 2)
                emit(**rec)

    def trace_case(name, scene, camera_of, w, h, by_bounces=False):
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
                call(0, 1)
                stream.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                call(1, args.samples)
                e1.record(stream)
                stream.synchronize()
                return e0.elapsed_time(e1) * 1000.0 / args.samples

            rec = dict(case=f"trace_{name}", width=w, height=h, triangles=ntri, bounces=8, samples=args.samples)
            images = {}
            for mode, key in ((T.RAY_ACCEL_OFF, "off"), (T.RAY_ACCEL_ON, "on")):
                tr.ray_accel = mode
                bb = {b: timed(b) for b in ((0, 1, 2, 4, 8) if by_bounces else (8,))}
                rec[f"{key}_us_per_sample"] = round(bb[8], 1)
                if by_bounces:
                    rec[f"{key}_us_by_bounces"] = {str(b): round(t, 1) for b, t in bb.items()}
                images[key] = acc.cpu().numpy().view(np.uint32).copy()
            rec["same_floats"] = bool(np.array_equal(images["off"], images["on"]))
            tr.ray_accel = T.RAY_ACCEL_COUNT
            timed(8)
            rec["tests_per_path_slot_and_round"] = round(info(tr)["tests"] / (args.samples * 8.0 * w * h), 2)
            rec["speedup"] = round(rec["off_us_per_sample"] / rec["on_us_per_sample"], 2)
            emit(**rec)

    from tests import ray_accel_ref as A
    leaf_width = (os.environ.get("RXR_BENCH_LEAF_WIDTH") or f"{A.LEAF}x{A.WIDTH}").split("x")
    leaf_width = (int(leaf_width[0]), int(leaf_width[1]))

    teapot, t_eye, t_centre = product_scene(lambda a: scenes.teapot_scene(a, 160, 120, 40, logo_size=64))
    grid32, g_eye, g_centre = product_scene(lambda a: scenes.box_grid_scene(a, n=32, width=160, height=120))
    pick_cases("teapot", teapot, t_eye, t_centre, [("1080p", 1920, 1080, True), ("4096", 64, 64, True)])
    pick_cases("grid_n32", grid32, g_eye, g_centre, [("540p", 960, 540, True), ("4096", 64, 64, True)])
    if not args.skip_large:
        big, b_eye, b_centre = product_scene(lambda a: scenes.box_grid_scene(a, width=320, height=200))
        pick_cases("grid_1m", big, b_eye, b_centre, [("4096", 64, 64, True), ("65536", 256, 256, True), ("1080p", 1920, 1080, False)])
        del big
    if not args.skip_trace:
        trace_case("teapot_1080p", teapot, lambda w, h: T.camera_firstp(t_eye, t_centre, 60.0, w, h), 1920, 1080, by_bounces=True)
        trace_case("box_grid_n32_540p", grid32, lambda w, h: T.camera_firstp(g_eye, g_centre, 60.0, w, h), 960, 540)
        room = S.diffuse_room()
        trace_case("room_1080p", room, lambda w, h: S.cameras(w, h)["firstp"], 1920, 1080)
        trace_case("room_64x36", room, lambda w, h: S.cameras(w, h)["firstp"], 64, 36)


if __name__ == "__main__":
    main()
