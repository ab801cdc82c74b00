#!/usr/bin/env python3
"""What chunk textures cost per frame when the frame carries them, and what they cost resident: one JSON line per row.

    python tools/chunk_texture_bench.py [--reps 20] [--warmup 3] [--only SUBSTRING] [--out profiles/chunk_textures/chunk_texture_bench.jsonl]

Three groups of rows, all on one GPU, all through code paths that exist side by side in one build:

  upload/<case>/<carried|resident>   the reduced box grid (scenes.box_grid_scene, 96 boxes, 1920 x 1080, device projection, so that the
        frame is matrices and headers only) plus chunks that hold `case`'s terrain textures.  upload_us: wall time of the mirror's
        Rasterizer::upload, whose device work is rxr_upload_frame.  frame_us: upload + rxr_render_rows + rxr_synchronize, wall.
        carried: the textures cross the ABI in every frame (alpha scan, memcpy into the staging blob, host-to-device copy); resident:
        Scene.resident_chunk_textures, registered before the timing.  Cases: none, 64 chunks x 256 x 256, 1 chunk x 1024 x 1024.
  stroke/<k>/<host|device>   a texture stroke on k chunks of 256 x 256 until the frame is uploaded again, wall.  host: Terrain.bake_chunks
        (rxr_bake_terrain, the bytes come down), the chunks' textures assigned, upload (the bytes go up again, all 64 chunks').
        device: Terrain.rebuild_chunk_textures (rxr_bake_terrain_to + rxr_update_chunk_textures_to), upload.  k = 1, 8, 64 of 64.
  commit/<shape>   rxr_update_chunk_textures_to alone from a device tensor, on a context of the tool's own: call_us is the wall time of
        the blocking call (rxr_quiesce, the flag fill, the k_chunk_tex_commit launches, the copy-back of the flag words, one
        synchronise).  The kernel's own duration on the stream, and the bandwidth it implies, come from a
        `rocprofv3 --kernel-trace --stats` run of `--only commit/<shape>` per shape (profiles/chunk_textures/README.md): a host clock
        around a blocking call cannot separate it from the call's fixed cost.

Every figure is the median [min..max] of --reps after --warmup rounds."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

os.environ.setdefault("RXR_SHADER_JIT", "0")  # (measurements name their mode: interpreted unless asked otherwise)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def texture(B, tag, side):
    rng = np.random.default_rng([0x43544258, tag])
    img = rng.integers(0, 256, size=(side * side, 4), dtype=np.uint8)
    img[:, 3] = 255
    return B.Texture(img.reshape(-1), side, side)


def stats(us):
    return dict(median=round(statistics.median(us), 1), min=round(min(us), 1), max=round(max(us), 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch

    import rusterix_amd
    from rusterix_amd import binding as B
    from rusterix_amd import scenes

    prod = rusterix_amd.load()
    host = prod.lib
    rxr = rusterix_amd.rxr_abi()
    out = open(args.out, "w") if args.out else None

    def emit(line):
        text = json.dumps(line)
        print(text, flush=True)
        if out:
            out.write(text + "\n")
            out.flush()

    def timed(fn, prepare=None):
        us = []
        for i in range(args.warmup + args.reps):
            if prepare:
                prepare()
            t0 = time.perf_counter()
            fn()
            if i >= args.warmup:
                us.append((time.perf_counter() - t0) * 1e6)
        return us

    host.rxh_set_device_projection(1)
    W, H = 1920, 1080

    def grid_with_chunks(textures, resident):
        cfg = scenes.box_grid_scene(prod, n=96, width=W, height=H)
        chunks = []
        for k, t in enumerate(textures):
            c = cfg.scene.add_chunk()
            c.terrain(t, origin=(16 * k, 0), size=16)
            chunks.append(c)
        cfg.scene.resident_chunk_textures = resident
        return cfg, chunks

    def upload(cfg, r):
        rc = host.rxh_rasterizer_upload(r._h, cfg.scene._h, W, H, cfg.tile_size, cfg.assets._h)
        assert rc == 0, host.rxh_last_error()

    def frame(cfg, r):
        upload(cfg, r)
        ctx = host.rxh_context()
        assert rxr.rxr_render_rows(ctx, 0, H) == 0 and rxr.rxr_synchronize(ctx) == 0, rxr.rxr_last_error(ctx)

    # ---- upload/<case>/<carried|resident> ----
    cases = (("none", []), ("64x256x256", [(k, 256) for k in range(64)]), ("1x1024x1024", [(100, 1024)]))
    for name, spec in cases:
        textures = [texture(B, tag, side) for tag, side in spec]
        for mode in ("carried", "resident"):
            row = f"upload/{name}/{mode}"
            if args.only and args.only not in row:
                continue
            cfg, _ = grid_with_chunks(textures, mode == "resident")
            r = cfg.setup()
            frame(cfg, r)   # registers what there is to register
            n0 = prod.chunk_texture_registrations()
            up, fr = timed(lambda: upload(cfg, r)), timed(lambda: frame(cfg, r))
            assert prod.chunk_texture_registrations() == n0, "the timed uploads must not register"
            emit(dict(row=row, chunk_textures=len(spec), texture_bytes=sum(s * s * 4 for _, s in spec), reps=args.reps, upload_us=stats(up), frame_us=stats(fr)))

    # ---- stroke/<k>/<host|device> ----
    CS, PPT, NX = 16, 16, 8     # 64 chunks of 16 x 16 cells at 16 pixels per tile: 256 x 256 texels each
    coords_all = np.array([(x, y) for y in range(NX) for x in range(NX)], np.int32)

    def stroke_scene(resident):
        terrain = prod.Terrain((1.0, 1.0), CS)
        a, b = texture(B, 201, 32), texture(B, 202, 48)
        for x in range(CS * NX):
            for y in range(CS * NX):
                terrain.set_source(x, y, a if (x // 3 + y // 5) % 2 else b)
        baked = terrain.bake_chunks(coords_all, PPT)
        cfg, chunks = grid_with_chunks([B.Texture(baked[k].reshape(-1), CS * PPT, CS * PPT) for k in range(len(coords_all))], resident)
        return terrain, cfg, chunks

    for k in (1, 8, 64):
        for mode in ("host", "device"):
            row = f"stroke/{k}/{mode}"
            if args.only and args.only not in row:
                continue
            terrain, cfg, chunks = stroke_scene(mode == "device")
            r = cfg.setup()
            frame(cfg, r)
            ids = list(range(k))
            cc = coords_all[ids]
            paint = [texture(B, 300 + i, 32) for i in range(2)]
            turn = [0]

            def prepare():   # the stroke itself (one cell per named chunk changes its source): not timed, the same on both sides
                turn[0] += 1
                for (cx, cy) in cc:
                    terrain.set_source(int(cx) * CS + 3, int(cy) * CS + 3, paint[turn[0] % 2])

            def host_path():
                baked = terrain.bake_chunks(cc, PPT)
                for j, i in enumerate(ids):
                    chunks[i].terrain(B.Texture(baked[j].reshape(-1), CS * PPT, CS * PPT), origin=(16 * i, 0), size=16)
                upload(cfg, r)

            def device_path():
                assert terrain.rebuild_chunk_textures(cfg.scene, cc, ids, PPT) == 0
                upload(cfg, r)

            us = timed(host_path if mode == "host" else device_path, prepare)
            emit(dict(row=row, chunks=k, of_chunks=len(coords_all), texture_bytes=k * (CS * PPT) ** 2 * 4, reps=args.reps, stroke_to_upload_us=stats(us)))
    host.rxh_set_device_projection(0)

    # ---- commit/<k> ----
    from rusterix_amd.abi import rxr_texture as Tex

    for k, side in ((1, 256), (8, 256), (64, 256), (1, 1024)):
        row = f"commit/{k}x{side}x{side}"
        if args.only and args.only not in row:
            continue
        ctx = C.c_void_p()
        assert rxr.rxr_create(C.byref(ctx), 0) == 0
        tex = (Tex * k)()
        for t in tex:
            t.rgba, t.width, t.height = None, side, side
        terrain_map, first = np.zeros(1, np.int32), np.zeros(2, np.uint32)
        assert rxr.rxr_set_chunk_textures(ctx, C.cast(tex, C.c_void_p), k, terrain_map.ctypes.data, first.ctypes.data, None, 1) == 0, rxr.rxr_last_error(ctx)
        stream = torch.cuda.Stream()
        src = torch.randint(0, 256, (k * side * side * 4,), dtype=torch.uint8, device="cuda")
        slots = np.arange(k, dtype=np.uint32)
        torch.cuda.synchronize()
        wall = []
        for i in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            rc = rxr.rxr_update_chunk_textures_to(ctx, slots.ctypes.data, k, src.data_ptr(), stream.cuda_stream)
            t1 = time.perf_counter()
            assert rc == 0, rxr.rxr_last_error(ctx)
            if i >= args.warmup:
                wall.append((t1 - t0) * 1e6)
        emit(dict(row=row, slots=k, bytes_copied=k * side * side * 4, launches=int(rxr.rxr_debug_chunk_tex_launches(ctx)), reps=args.reps, call_us=stats(wall)))
        rxr.rxr_destroy(ctx)
    if out:
        out.close()


if __name__ == "__main__":
    main()
