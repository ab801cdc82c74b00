#!/usr/bin/env python3
"""Timing of the shader-texture bake on the device (rxr_bake_shaders_to): one JSON line per case.

    python tools/bake_bench.py [--reps 20] [--warmup 3] [--cpu-texels 2048]

Cases: 256 programs x 64 x 64 in one call (a chunk set's bakes: 4096 workgroups in one launch), the same 256 bakes as 256 calls of one
program each (what a bake per Chunk::add_shader costs: launch-bound), and one program at 2048 x 2048 (Rusteria::shade as the rsia
tool runs it).  Per case: device time per call from events around `reps` calls after warm-up (the bake alone, outputs staying on
the device), texels/s, and the bytes written over the HBM peak as the floor the hardware sets -- the kernel is an interpreter, not a
copy, so the share is small and is reported as what it is.  CPU baseline: the same work done texel by texel through the oracle's
orc_vm_shade from Python, timed on a few texels and scaled -- it INCLUDES the ctypes call overhead of one call per texel, and is
labelled so."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12         # bytes per second
BYTES_PER_TEXEL = 20.0    # one float4 and one packed RGBA8 store


def programs(n):
    """n distinct programs of a texture-like kind: arithmetic on uv, a branch, a short loop (no libm: the interpreter itself is timed)"""
    from rusterix_amd.binding import Program

    out = []
    for k in range(n):
        a, b = 2.0 + (k % 7), 0.1 + 0.003 * k
        out.append(Program([[("Push", 0.0), ("StoreLocal", 0),
                             ("For", [("Push", 0.0), ("StoreLocal", 1)], [("LoadLocal", 1), ("Push", 4.0), "Lt"],
                              [("LoadLocal", 1), ("Push", 1.0), "Add", ("StoreLocal", 1)],
                              ["UV", ("Push", a), "Mul", ("LoadLocal", 1), "Add", "Fract", ("LoadLocal", 0), "Add", ("StoreLocal", 0)]),
                             ("LoadLocal", 0), ("Push", 0.25), "Mul", "UV", ("GetComponents", [0]), ("Push", 0.5), "Lt",
                             ("If", [("Push", b), "Add"], [("Push", 0.9, 0.8, 0.7), "Mul"]), "SetColor"]], shade_locals=2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu-texels", type=int, default=2048)
    args = ap.parse_args()

    import torch

    import rusterix_amd
    from tests import bake_ref as R
    from tests.oracle_api import load_oracle

    api = rusterix_amd.load()
    rxr = rusterix_amd.rxr_abi()
    progs = programs(256)
    scene = api.Scene.empty()
    for p in progs:
        scene.add_program(p)
    first = scene.bake_shaders([0], 64, 64)       # makes the set resident
    ctx = api.lib.rxh_context()
    ref = R.Reference(load_oracle(), progs)
    want = ref.pixels(0, 64, 64)
    assert np.array_equal(first["pixels"][0].view(np.uint32), want.view(np.uint32)), "the device's bake differs from the oracle's"
    # CPU baseline: orc_vm_shade per texel from Python
    k = max(1, min(args.cpu_texels, 4096))
    c0 = time.perf_counter()
    ref.pixels(0, k, 1)
    cpu_s_per_texel = (time.perf_counter() - c0) / k

    stream = torch.cuda.Stream()
    sp = stream.cuda_stream

    def case(name, order, w, h, calls):
        n = len(order) // calls
        texels = len(order) * w * h
        px = torch.empty((len(order), h, w, 4), dtype=torch.float32, device="cuda")
        by = torch.empty((len(order), h, w, 4), dtype=torch.uint8, device="cuda")
        lists = [np.ascontiguousarray(order[i * n:(i + 1) * n], np.uint32) for i in range(calls)]

        def run():
            for i, l in enumerate(lists):
                off = i * n * w * h
                rc = rxr.rxr_bake_shaders_to(ctx, l.ctypes.data, n, w, h, px.data_ptr() + off * 16, by.data_ptr() + off * 4, sp)
                assert rc == 0, rxr.rxr_last_error(ctx)

        for _ in range(args.warmup):
            run()
        stream.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record(stream)
            for _ in range(args.reps):
                run()
            e1.record(stream)
        stream.synchronize()
        assert rxr.rxr_synchronize(ctx) == 0, rxr.rxr_last_error(ctx)
        us = e0.elapsed_time(e1) * 1000.0 / args.reps
        floor_us = texels * BYTES_PER_TEXEL / HBM_PEAK * 1e6
        print(json.dumps(dict(case=name, bakes=len(order), width=w, height=h, calls=calls, device_us=round(us, 2), texels_per_s=texels / (us * 1e-6),
                              hbm_write_floor_us=round(floor_us, 3), floor_fraction=round(floor_us / us, 4),
                              cpu_python_baseline_s=round(cpu_s_per_texel * texels, 3),
                              cpu_baseline=f"orc_vm_shade per texel from Python, ctypes call overhead included, timed on {k} texels of program 0 and scaled")),
              flush=True)

    order = np.arange(256, dtype=np.uint32)
    case("256x64x64_one_call", order, 64, 64, 1)
    case("256x64x64_256_calls", order, 64, 64, 256)
    case("1x2048x2048", np.zeros(1, np.uint32), 2048, 2048, 1)


if __name__ == "__main__":
    main()
