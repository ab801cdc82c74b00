#!/usr/bin/env python3
"""Wide sweep of the seeded ray-picking scenes (tests/pick_fuzz.py): the device against tests/intersect_ref.py::intersect_many, bit
for bit, on many more seeds than tests/test_gpu_intersect_fuzz.py runs -- per seed 1, 8, 9, 64, 65, 256, 257 and `rays` rays, plain
and full, and the two kernels against each other.  One process, one context; it stops at the first error of the library (a fault
is not run past), mismatching seeds are listed.  usage: python tools/intersect_fuzz_sweep.py [first_seed] [n_seeds] [--rays N]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rusterix_amd  # noqa: E402
from tests import pick_fuzz as P  # noqa: E402

argv = [a for a in sys.argv[1:]]
rays = 3000
if "--rays" in argv:
    i = argv.index("--rays")
    rays = int(argv[i + 1])
    del argv[i:i + 2]
first = int(argv[0]) if len(argv) > 0 else 1000
n = int(argv[1]) if len(argv) > 1 else 100
lib = rusterix_amd.lib_paths()["rxr"]
print(f"library {os.path.relpath(lib, ROOT)}, {os.path.getsize(lib)} bytes, built {time.strftime('%Y-%m-%d %H:%M:%S', time.gmtime(os.path.getmtime(lib)))} UTC", flush=True)
bad = []
t0 = time.time()
with P.PickContext() as ctx:
    for s in range(first, first + n):
        if s in P.SEEDS:
            continue    # (the suite's own)
        msg = P.check_seed(s, ctx, rays)
        if msg:
            bad.append((s, msg))
        if (s - first) % 100 == 99:
            print(f"... {s - first + 1} seeds, {len(bad)} mismatching so far, {time.time() - t0:.0f} s", flush=True)
print(f"seeds {first} .. {first + n - 1}, {rays} rays each: mismatching seeds: {len(bad)}; {time.time() - t0:.0f} s")
for s, msg in bad[:20]:
    print("  ", s, msg)
sys.exit(1 if bad else 0)
