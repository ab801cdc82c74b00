#!/usr/bin/env python3
"""Cost of the first many-ray query after rxr_update_meshes under RXR_RAY_REFRESH_RANGED against RXR_RAY_REFRESH_FULL, in the same
session and build (rxr_set_ray_refresh, include/rxr.h).  One JSON line per case.

    python tools/ray_refresh_bench.py [--reps 10] [--cases terrain,static,teapot,chain,sweep,drift] [--out profiles/ray_refresh/ray_refresh_bench.jsonl]

Method: two contexts hold the same meshes with the box tree on, one in each mode.  Per repetition both take the same update (device
arrays, rxr_update_meshes_to; the geometry alternates between two states so that every update changes something), then one
65-ray rxr_intersect_to (the smallest query on the many-ray path) between two events on its stream.  The refresh's cost is that time minus the median of the same query
with nothing pending; the medians over --reps repetitions are reported.  Before any time is taken every output word of a
4 096-ray query on both contexts is compared after an update.

Cases
  terrain_*   1 024 chunk meshes of 16 x 16 cells (512 triangles each) of a 512 x 512 terrain; 1, 16, 64 and all chunks dirty
              (_tree_off: the box tree off in both contexts, so only the pick records are at stake)
  static_1m   one such chunk next to a static mesh of about a million triangles
  teapot      the teapot scene, every mesh dirty
  chain       wall time of rxr_update_meshes_to for one dirty chunk followed by one trace sample (64 x 36, 4 bounces), host clock around
              both, synchronised; the mesh generation and the normals ahead of it are in profiles/terrain_tiles and
              profiles/vertex_normals and are not repeated here
  sweep       1 to 64 dirty chunks (64 leaves each) through both refit routes: RXR_RAY_REFIT_SMALL_MAX=0 in the environment of a child
              process forces the launch per level; above the shipped bound only that route exists
  drift       1, 10 and 100 strokes that raise or sink a bump of a chunk's own extent (16) in a random chunk, a refit after each; then the ray-triangle tests a ray
              and the trace-sample time, against the same geometry registered fresh on a second context (what rxr_ray_accel_invalidate and a build give)
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
F = np.float32
CHUNK = 16
TIMED_RAYS = 65      # the smallest query that takes the many-ray path: the refresh is timed against a small, steady base


def chunk_mesh(cx, cz, lift=0.0, bump=None):
    """(vertices [289][4], indices [512][3], normals [289][3]) of chunk (cx, cz): heights of a smooth field plus `lift`, plus a bump
    (amplitude, x, z in cells of the chunk) four cells wide"""
    xs, zs = np.meshgrid(np.arange(CHUNK + 1, dtype=F) + cx * CHUNK, np.arange(CHUNK + 1, dtype=F) + cz * CHUNK)
    h = (np.sin(xs * 0.05) * np.cos(zs * 0.07) * 6.0 + np.sin(xs * 0.31 + zs * 0.17) * 0.8 + lift).astype(F)
    if bump is not None:
        r2 = (xs - (cx * CHUNK + bump[1])) ** 2 + (zs - (cz * CHUNK + bump[2])) ** 2
        h = (h + bump[0] * np.exp(-r2 / 32.0)).astype(F)
    v = np.stack([xs.ravel(), h.ravel(), zs.ravel(), np.ones(xs.size, F)], axis=1).astype(F)
    i0 = (np.arange(CHUNK)[:, None] * (CHUNK + 1) + np.arange(CHUNK)[None, :]).ravel()
    idx = np.stack([np.stack([i0, i0 + 1, i0 + CHUNK + 2], 1), np.stack([i0, i0 + CHUNK + 2, i0 + CHUNK + 1], 1)], 1).reshape(-1, 3).astype(np.uint32)
    nr = np.tile(np.array([0, 1, 0], F), (len(v), 1))
    return v, idx, nr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--cases", default="terrain,static,teapot,chain,sweep,drift")
    ap.add_argument("--sweep-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    cases = set(args.cases.split(","))

    import torch

    import rusterix_amd
    from rusterix_amd import scenes
    from rusterix_amd import trace as T
    from tests import intersect_ref as R
    from tests import trace_scenes as S

    out = open(args.out, "a") if args.out else None

    def emit(**rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    def tmesh(v, idx, nr, lst=T.LIST_STATIC):
        return T.mesh(v, idx, v[:, :2].copy(), nr, list=lst, source=S.PIXEL(200, 190, 170), material=(T.MATTE, T.MOD_NONE, 0.7))

    def rays_down(lo, hi, n_side=64, y=60.0):
        xs, zs = np.meshgrid(np.linspace(lo[0], hi[0], n_side, dtype=F), np.linspace(lo[1], hi[1], n_side, dtype=F))
        o = np.stack([xs.ravel(), np.full(xs.size, y, F), zs.ravel()], axis=1).astype(F)
        d = np.tile(np.array([0.05, -1.0, 0.03], F), (len(o), 1))
        return o, d

    class Ctx:
        """a context with the tree on, in one refresh mode, with device arrays for rays, outputs and updates"""

        def __init__(self, meshes, mode, o, d, accel=None):
            self.tr = T.Tracer()
            self.tr.set_textures([], [])
            self.tr.set_chunk_textures([])
            self.tr.set_meshes(meshes)
            self.tr.set_scene([S.point_light((256.0, 80.0, 256.0), intensity=3.0, start=50.0, end=600.0)], 0, 1)
            self.tr.ray_accel, self.tr.ray_refresh = (T.RAY_ACCEL_ON if accel is None else accel), mode
            self.n = len(o)
            self.o, self.d = torch.tensor(o, device="cuda"), torch.tensor(d, device="cuda")
            self.t = torch.empty(self.n, dtype=torch.float32, device="cuda")
            self.m = torch.empty(self.n, dtype=torch.int32, device="cuda")
            self.k = torch.empty_like(self.m)
            self.stream = torch.cuda.Stream()
            torch.cuda.synchronize()
            self.query()
            self.stream.synchronize()

        def close(self):
            self.tr.close()

        def query(self, n=None):
            rc = self.tr.rxr.rxr_intersect_to(self.tr.ctx, self.o.data_ptr(), self.d.data_ptr(), n or self.n, 0, self.t.data_ptr(), self.m.data_ptr(), self.k.data_ptr(),
                                              None, None, None, self.stream.cuda_stream)
            assert rc == 0, self.tr.error()

        def timed_query(self):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(self.stream)
            self.query(TIMED_RAYS)
            e1.record(self.stream)
            self.stream.synchronize()
            return e0.elapsed_time(e1) * 1000.0

        def words(self):
            self.stream.synchronize()
            return self.t.cpu().numpy().view(np.uint32).copy(), self.m.cpu().numpy().copy(), self.k.cpu().numpy().copy()

        def update(self, upd):
            named, counts, v, idx, nr = upd
            rc = self.tr.rxr.rxr_update_meshes_to(self.tr.ctx, named.ctypes.data, len(named), counts.data_ptr(), v.data_ptr(), idx.data_ptr(), nr.data_ptr(),
                                                  v.shape[1], idx.shape[1], self.stream.cuda_stream)
            assert rc == 0, self.tr.error()

    def device_update(named, geoms):
        """the device arrays of one update: geoms[i] = (vertices, indices, normals) of mesh named[i]"""
        vs, ts = max(len(g[0]) for g in geoms), max(len(g[1]) for g in geoms)
        n = len(geoms)
        counts = np.array([(len(g[0]), len(g[1])) for g in geoms], np.uint32)
        v, idx, nr = np.zeros((n, vs, 4), F), np.zeros((n, ts, 3), np.uint32), np.zeros((n, vs, 3), F)
        for i, g in enumerate(geoms):
            v[i, :len(g[0])], idx[i, :len(g[1])], nr[i, :len(g[0])] = g
        dev = [torch.tensor(a.view(np.int32) if a.dtype == np.uint32 else a, device="cuda") for a in (counts, v, idx, nr)]
        torch.cuda.synchronize()
        return (np.asarray(named, np.uint32), *dev)

    def compare_modes(name, meshes, o, d, states, extra=None, reps=None, accel=None):
        """states: two updates of the same named meshes (A and B).  Emits the case's line; returns it"""
        reps = reps or args.reps
        both = {key: Ctx(meshes, mode, o, d, accel) for key, mode in (("full", T.RAY_REFRESH_FULL), ("ranged", T.RAY_REFRESH_RANGED))}
        try:
            same = True
            for upd in states:      # every output word, before any time is taken
                got = {}
                for key, c in both.items():
                    c.update(upd)
                    c.query()
                    got[key] = c.words()
                same = same and all(np.array_equal(a, b) for a, b in zip(got["full"], got["ranged"]))
            rec = dict(case=name, triangles=sum(len(m["indices"]) for m in meshes), meshes=len(meshes), dirty_meshes=len(states[0][0]), rays_compared=len(o), rays_timed=TIMED_RAYS,
                       same_words=bool(same), hits=int((got["ranged"][1] != -1).sum()), reps=reps)
            for key, c in both.items():
                steady = float(np.median([c.timed_query() for _ in range(reps)]))
                first = []
                for r in range(reps):
                    c.update(states[r % 2])
                    first.append(c.timed_query())
                rec[f"{key}_first_query_us"] = round(float(np.median(first)), 1)
                rec[f"{key}_steady_query_us"] = round(steady, 1)
                rec[f"{key}_refresh_us"] = round(float(np.median(first)) - steady, 1)
            i = both["ranged"].tr.ray_refresh_info()
            rec.update(dirty_triangles=i["triangles"], dirty_leaves=i["leaves"], dirty_nodes=i["nodes"], route=i["route"],
                       builds_full=both["full"].tr.ray_accel_info()["builds"], builds_ranged=both["ranged"].tr.ray_accel_info()["builds"])
            v = both["ranged"].tr.ray_refresh_verify()
            rec["verify"] = [v["pick_words"], v["sorted_words"], v["nodes"]]
            rec["full_over_ranged"] = round(rec["full_refresh_us"] / max(rec["ranged_refresh_us"], 0.1), 2)
            if extra:
                rec.update(extra)
            emit(**rec)
            return rec
        finally:
            for c in both.values():
                c.close()

    def terrain(side=32):
        return [tmesh(*chunk_mesh(k % side, k // side)) for k in range(side * side)]

    def chunk_states(named, side=32, lift=3.0):
        return [device_update(named, [chunk_mesh(k % side, k // side, lift=l) for k in named]) for l in (lift, 0.0)]

    if args.sweep_child:      # (the parent set RXR_RAY_REFIT_SMALL_MAX=0: every refit takes a launch per level)
        meshes = terrain()
        o, d = rays_down((0, 0), (512, 512))
        for n in (1, 2, 4, 8):
            compare_modes(f"sweep_general_{n * 64}_leaves", meshes, o, d, chunk_states(list(range(100, 100 + n))), extra=dict(forced_general=True))
        return

    if "terrain" in cases or "sweep" in cases:
        meshes = terrain()
        o, d = rays_down((0, 0), (512, 512))
    if "terrain" in cases:
        rng = np.random.default_rng(1)
        for n in (1, 16, 64, 1024):
            named = sorted(rng.choice(1024, n, replace=False).tolist()) if n < 1024 else list(range(1024))
            compare_modes(f"terrain_{n}_of_1024_chunks_dirty", meshes, o, d, chunk_states(named))
            if n in (1, 1024):      # the pick records alone: no tree in either mode
                compare_modes(f"terrain_{n}_of_1024_chunks_dirty_tree_off", meshes, o, d, chunk_states(named), accel=T.RAY_ACCEL_OFF)
    if "sweep" in cases:
        for n in (1, 2, 4, 8, 16, 32, 64):
            compare_modes(f"sweep_{n * 64}_leaves", meshes, o, d, chunk_states(list(range(100, 100 + n))))
        if out:
            out.close()
            out = None
        env = dict(os.environ, RXR_RAY_REFIT_SMALL_MAX="0")
        cmd = [sys.executable, os.path.abspath(__file__), "--sweep-child", "--reps", str(args.reps)] + (["--out", args.out] if args.out else [])
        subprocess.run(cmd, check=True, env=env, timeout=600)      # (a fresh process: the bound is read once)
        out = open(args.out, "a") if args.out else None
    if "static" in cases:
        n = 708
        xs, zs = np.meshgrid(np.arange(n + 1, dtype=F) * F(0.7), np.arange(n + 1, dtype=F) * F(0.7))
        v = np.stack([xs.ravel(), np.sin(xs.ravel() * 0.1) * 2 - 30.0, zs.ravel(), np.ones(xs.size, F)], axis=1).astype(F)
        i0 = (np.arange(n)[:, None] * (n + 1) + np.arange(n)[None, :]).ravel()
        idx = np.stack([np.stack([i0, i0 + 1, i0 + n + 2], 1), np.stack([i0, i0 + n + 2, i0 + n + 1], 1)], 1).reshape(-1, 3).astype(np.uint32)
        big = [tmesh(v, idx, np.tile(np.array([0, 1, 0], F), (len(v), 1))), tmesh(*chunk_mesh(10, 10), lst=T.LIST_DYNAMIC)]
        o, d = rays_down((100, 100), (260, 260))
        compare_modes("static_1m_plus_one_chunk_dirty", big, o, d, [device_update([1], [chunk_mesh(10, 10, lift=l)]) for l in (3.0, 0.0)])
        del big, v, idx
    if "teapot" in cases:
        api = rusterix_amd.load()
        with R.recording(api) as meshes_of:
            cfg = scenes.teapot_scene(api, 160, 120, 40, logo_size=64)
        tp = [tmesh(m["vertices"], m["indices"], m["normals"], lst=m["list"]) for m in meshes_of(cfg.scene) if len(m["indices"])]
        allv = np.concatenate([m["vertices"][:, :3] for m in tp])
        lo, hi = allv.min(axis=0), allv.max(axis=0)
        o, d = rays_down((lo[0], lo[2]), (hi[0], hi[2]), y=float(hi[1] + 1.0))
        states = []
        for s in (1.01, 1.0):
            geoms = []
            for m in tp:
                v = m["vertices"].copy()
                v[:, :3] *= F(s)
                geoms.append((v, m["indices"], m["normals"]))
            states.append(device_update(list(range(len(tp))), geoms))
        compare_modes("teapot_wholly_dirty", tp, o, d, states)
    if "chain" in cases:
        meshes = terrain()
        w, h = 64, 36
        cam_kind, cam = T.camera_firstp((256.0, 40.0, 200.0), (256.0, 0.0, 256.0), 70.0, w, h)
        o, d = rays_down((0, 0), (512, 512))
        rec = dict(case="chain_update_to_then_trace_sample", triangles=len(meshes) * 512, width=w, height=h, bounces=4, reps=args.reps)
        states = chunk_states([500])
        for key, mode in (("full", T.RAY_REFRESH_FULL), ("ranged", T.RAY_REFRESH_RANGED)):
            c = Ctx(meshes, mode, o, d)
            acc = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()

            def sample(frame):
                rc = c.tr.rxr.rxr_trace_to(c.tr.ctx, cam_kind, cam.ctypes.data, w, h, frame, 1, 1, 4, acc.data_ptr(), c.stream.cuda_stream)
                assert rc == 0, c.tr.error()
                c.stream.synchronize()

            sample(0)
            walls, alone = [], []
            for r in range(args.reps):
                t0 = time.perf_counter()
                c.update(states[r % 2])
                sample(r + 1)
                walls.append((time.perf_counter() - t0) * 1e6)
                t0 = time.perf_counter()
                sample(r + 1)
                alone.append((time.perf_counter() - t0) * 1e6)
            rec[f"{key}_update_and_sample_wall_us"] = round(float(np.median(walls)), 1)
            rec[f"{key}_sample_alone_wall_us"] = round(float(np.median(alone)), 1)
            c.close()
        emit(**rec)
    if "drift" in cases:
        side = 32
        meshes = terrain(side)
        o, d = rays_down((0, 0), (512, 512), n_side=256, y=300.0)
        w, h = 256, 144
        cam_kind, cam = T.camera_firstp((256.0, 40.0, 200.0), (256.0, 0.0, 256.0), 70.0, w, h)
        c = Ctx(meshes, T.RAY_REFRESH_RANGED, o, d)
        acc = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()

        def measure(c):
            c.tr.ray_accel = T.RAY_ACCEL_COUNT
            c.query()
            c.stream.synchronize()
            tests = c.tr.ray_accel_info()["tests"] / len(o)
            c.tr.ray_accel = T.RAY_ACCEL_ON
            q = float(np.median([c.timed_query() for _ in range(args.reps)]))
            ts = []
            for r in range(args.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(c.stream)
                rc = c.tr.rxr.rxr_trace_to(c.tr.ctx, cam_kind, cam.ctypes.data, w, h, r, 1, 1, 8, acc.data_ptr(), c.stream.cuda_stream)
                assert rc == 0, c.tr.error()
                e1.record(c.stream)
                c.stream.synchronize()
                ts.append(e0.elapsed_time(e1) * 1000.0)
            return round(tests, 2), round(q, 1), round(float(np.median(ts)), 1), c.words()

        rng = np.random.default_rng(2)
        bumps = {}      # per chunk (amplitude, x, z): a stroke adds the chunk's own extent to the amplitude, up or down, and moves the centre
        geom = lambda k: chunk_mesh(k % side, k // side, bump=bumps.get(k))
        done = 0
        for strokes in (1, 10, 100):
            while done < strokes:
                k = int(rng.integers(side * side))
                bumps[k] = (bumps.get(k, (0.0,))[0] + CHUNK * (1 if rng.random() < 0.5 else -1), float(rng.uniform(2, 14)), float(rng.uniform(2, 14)))
                c.update(device_update([k], [geom(k)]))
                c.query()      # (a refit per stroke; the tree keeps the order of its one build)
                done += 1
            i = c.tr.ray_accel_info()
            refit = measure(c)
            # the same geometry registered fresh on a context of its own: a tree in this geometry's own order
            f = Ctx([tmesh(*geom(k)) for k in range(side * side)], T.RAY_REFRESH_FULL, o, d)
            fresh = measure(f)
            f.close()
            emit(case=f"drift_after_{strokes}_strokes", triangles=side * side * 512, rays=len(o), builds=i["builds"], refits=c.tr.ray_refresh_info()["refits"],
                 refit_tests_per_ray=refit[0], fresh_tests_per_ray=fresh[0], refit_query_us=refit[1], fresh_query_us=fresh[1],
                 refit_trace_sample_us=refit[2], fresh_trace_sample_us=fresh[2], trace=f"{w}x{h}, 8 bounces",
                 same_words=bool(all(np.array_equal(a, b) for a, b in zip(refit[3], fresh[3]))))
        c.close()


if __name__ == "__main__":
    main()
