"""Flattened terrain heights without a GPU: the host mirror's Terrain::process_heights_cpu against the dictionary transcription of
tests/terrain_flatten_ref.py on every case of the GPU suite -- every height word and presence byte, a NaN where the reference has
one --; the per-cell predicate form the device kernel takes, restated here in numpy over a chunk's cells at once, held to the loop
form on the same cases (the fuzz scenes among them); what rxr_check_terrain_flatten refuses; and the registration arithmetic under
AddressSanitizer and UBSan in a stand-alone program."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import rusterix_amd
from rusterix_amd.abi import RXR_ERR_INVALID, RXR_ERR_UNSUPPORTED, RXR_OK
from tests import terrain_flatten_ref as R
from tests.terrain_flatten_ref import F
from tests.terrain_ref import as_i32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def api():
    return rusterix_amd.load()


# ---- the mirror ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_the_mirror_equals_the_transcription(api, name):
    sc, coords, want = R.case(name)
    heights, present = sc.product(api).process_heights_cpu(coords)
    for i, c in enumerate(coords):
        d = R.first_difference(heights[i], present[i], *want[i])
        assert not d, f"{name} chunk {c}: {d}"


def test_the_cases_hold_what_their_names_say():
    """the properties the cases were built for, read off the transcription's answers"""
    def cell(name, chunk, x, y):
        sc, coords, want = R.case(name)
        cs = sc.spec.chunk_size
        i = coords.index(chunk)
        lx, ly = x - chunk[0] * cs, y - chunk[1] * cs
        return want[i][0][ly * cs + lx], want[i][1][ly * cs + lx], sc.spec.heights.get((x, y))

    # last wins: the overlap's cell (4, 3) lies deep inside both squares and takes the later op's floor
    assert cell("overlap_first_order", (0, 0), 4, 3)[0] == F(-2.0) and cell("overlap_other_order", (0, 0), 4, 3)[0] == F(2.0)
    # an absent cell inside a sector is present at floor_height; one under the road alone at the segment's height
    h, p, was = cell("road_over_sector", (0, 0), 3, 2)
    assert was is None and p == 1 and h == F(1.0)
    h, p, was = cell("road_over_sector", (1, 0), 13, 4)
    assert was is None and p == 1 and F(3.0) < h < F(4.0)
    # the linedef op wins over the sector under it
    assert cell("road_over_sector", (0, 0), 5, 4)[0] > F(3.0)
    # a chunk no op reaches is the registered cells
    sc, coords, want = R.case("untouched_chunk")
    h, p = want[1]
    for ly in range(8):
        for lx in range(8):
            was = sc.spec.heights.get((32 + lx, 32 + ly))
            assert p[ly * 8 + lx] == (was is not None) and h[ly * 8 + lx].view(np.uint32) == F(0.0 if was is None else was).view(np.uint32)
    # the +-1 filter: chunk (0, 0) is the registered cells although bevel * 4 reaches it; chunk (1, 0) is flattened
    sc, coords, want = R.case("filter_margin")
    assert all(want[0][0][ly * 8 + lx] == sc.spec.heights[(lx, ly)] for ly in range(8) for lx in range(8))
    assert cell("filter_margin", (1, 0), 10, 3)[0] == F(3.0)
    # the per-chunk segment filter: (7, 4) takes the long segment's height 1.0 although the short one (height 5.0) is nearer
    h, _, was = cell("neighbour_segments", (0, 0), 7, 4)
    assert min(F(1.0), was) <= h <= max(F(1.0), was) and cell("neighbour_segments", (1, 0), 9, 4)[0] > F(3.0)
    # bevel == 0: NaN on the road's tile centres, the last row and column untouched
    sc, coords, want = R.case("zero_bevel")
    assert np.isnan(want[0][0][5 * 8: 5 * 8 + 7]).all() and want[0][0][5 * 8 + 7] == sc.spec.heights[(7, 5)]
    assert all(want[0][0][ly * 8 + 7] == sc.spec.heights[(7, ly)] for ly in range(8))
    assert cell("zero_bevel", (0, 0), 2, 2)[0] == F(2.0)
    # a degenerate first segment is never displaced: every cell of the loop's range is a NaN; in second place it changes nothing
    assert np.isnan(R.case("degenerate_first_segment")[2][0][0][:7 * 8].reshape(7, 8)[:, :7]).all()
    assert not np.isnan(R.case("degenerate_second_segment")[2][0][0]).any()
    # a negative bevel: the road writes nothing
    sc, coords, want = R.case("negative_bevel")
    assert want[0][0][8 * 16 + 0] == sc.spec.heights[(0, 8)]


# ---- the per-cell form -----------------------------------------------------------------------------------------------------------------
def per_cell(sc, coord):
    """processed heights and presence of a chunk's own cells as a function of the cell: the last op in list order that writes it.  The
    device kernel's form (rusterix_amd/csrc/rxr_terrain_flatten.hip), in numpy float32 over all cells of the chunk at once."""
    cs = sc.spec.chunk_size
    ox, oy = coord[0] * cs, coord[1] * cs
    bbox = sc.bounds(coord)
    ys, xs = np.meshgrid(np.arange(oy, oy + cs), np.arange(ox, ox + cs), indexing="ij")
    xs, ys = xs.ravel(), ys.ravel()
    px, py = xs.astype(F), ys.astype(F)
    was = np.array([(int(x), int(y)) in sc.spec.heights for x, y in zip(xs, ys)])
    unprocessed = np.array([sc.spec.heights.get((int(x), int(y)), F(0.0)) for x, y in zip(xs, ys)], F)
    in_chunk_box = (px >= bbox.min[0]) & (px <= bbox.max[0]) & (py >= bbox.min[1]) & (py <= bbox.max[1])
    value, written = unprocessed.copy(), np.zeros(len(xs), bool)

    def clamp01(t):
        return np.where(t < F(0.0), F(0.0), np.where(t > F(1.0), F(1.0), t)).astype(F)

    def smoothstep(bevel, x):
        t = clamp01((x - F(0.0)) / (bevel - F(0.0)))
        return (t * t) * (F(3.0) - F(2.0) * t)

    def distance(qx, qy, r):
        ex, ey = F(r[2] - r[0]), F(r[3] - r[1])
        t = clamp01(((qx - r[0]) * ex + (qy - r[1]) * ey) / F(ex * ex + ey * ey))
        cx, cy = r[0] + ex * t, r[1] + ey * t
        return np.sqrt((qx - cx) * (qx - cx) + (qy - cy) * (qy - cy)), t

    with np.errstate(all="ignore"):
        for op in sc.ops:
            bevel = op.bevel
            if op.kind == R.SECTOR:
                if not bbox.intersects(op.box.expanded(2.0)):
                    continue
                rb, eb = op.box.expanded(bevel), bbox.expanded(bevel)
                lo_x, hi_x = int(as_i32(np.floor(rb.min[0]))), int(as_i32(np.ceil(rb.max[0])))
                lo_y, hi_y = int(as_i32(np.floor(rb.min[1]))), int(as_i32(np.ceil(rb.max[1])))
                reached = (xs >= lo_x) & (xs <= hi_x) & (ys >= lo_y) & (ys <= hi_y) & (px >= eb.min[0]) & (px <= eb.max[0]) & (py >= eb.min[1]) & (py <= eb.max[1])
                min_dist = np.full(len(xs), R.F32_MAX, F)
                inside = np.zeros(len(xs), bool)
                n = len(op.records)
                for i, r in enumerate(op.records):
                    min_dist = np.fmin(min_dist, distance(px, py, r)[0])
                    if n >= 3:
                        j = op.records[i - 1]
                        cross = (r[1] > py) != (j[1] > py)
                        inside ^= cross & (px < F(j[0] - r[0]) * (py - r[1]) / F(j[1] - r[1]) + r[0])
                sd = np.where(inside, -min_dist, min_dist)
                s = smoothstep(bevel, bevel - sd)
                original = np.where(was, unprocessed, op.floor_height)
                writes = reached & in_chunk_box & (sd < F(bevel * F(4.0)))
                new = original * (F(1.0) - s) + op.floor_height * s
            else:
                segments = [r for r in op.records if bbox.intersects(R.BBox(*r[6:10]).expanded(2.0))]
                if not segments:
                    continue
                sx, sy = sc.spec.scale
                lo_x = int(as_i32(np.floor(F(F(bbox.min[0] - F(bevel * sx)) / sx))))
                lo_y = int(as_i32(np.floor(F(F(bbox.min[1] - F(bevel * sy)) / sy))))
                hi_x = int(as_i32(np.ceil(F(F(bbox.max[0] + F(bevel * sx)) / sx))))
                hi_y = int(as_i32(np.ceil(F(F(bbox.max[1] + F(bevel * sy)) / sy))))
                cx, cy = (px + F(0.5)) * sx, (py + F(0.5)) * sy
                best = best_t = h0 = h1 = None
                for k, r in enumerate(segments):
                    dist, t = distance(cx, cy, r)
                    take = np.ones(len(xs), bool) if k == 0 else dist < best
                    best = dist if k == 0 else np.where(take, dist, best)
                    best_t = t if k == 0 else np.where(take, t, best_t)
                    h0 = np.where(take, r[4], F(0.0) if k == 0 else h0).astype(F)
                    h1 = np.where(take, r[5], F(0.0) if k == 0 else h1).astype(F)
                height = h0 * (F(1.0) - best_t) + h1 * best_t
                blend = smoothstep(bevel, bevel - best)
                original = np.where(was, unprocessed, height)
                writes = (xs >= lo_x) & (xs < hi_x) & (ys >= lo_y) & (ys < hi_y) & in_chunk_box & ~(best > bevel)
                new = original * (F(1.0) - blend) + height * blend
            value = np.where(writes, new, value).astype(F)
            written |= writes
    return value, (was | written).astype(np.uint8)


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_the_per_cell_form_equals_the_loop_form(name):
    sc, coords, want = R.case(name)
    for i, c in enumerate(coords):
        d = R.first_difference(*per_cell(sc, c), *want[i])
        assert not d, f"{name} chunk {c}: {d}"


@pytest.mark.parametrize("seed", range(3, 23))
def test_the_per_cell_form_on_more_fuzz_scenes(api, seed):
    sc, coords = R.fuzz_scene(seed)
    heights, present = sc.product(api).process_heights_cpu(coords)
    for i, c in enumerate(coords):
        want = sc.dense(c)
        assert not R.first_difference(*per_cell(sc, c), *want), f"seed {seed} chunk {c}"
        assert not R.first_difference(heights[i], present[i], *want), f"seed {seed} chunk {c}: the mirror"


# ---- rxr_check_terrain_flatten ---------------------------------------------------------------------------------------------------------
def check(kinds, params, ranges, records, n_ops=None, n_records=None, null=()):
    rxr = rusterix_amd.rxr_abi()
    k, p = np.array(kinds, np.uint32), np.array(params, np.float32).reshape(-1, 6)
    g, r = np.array(ranges, np.uint32).reshape(-1, 2), np.array(records, np.float32).reshape(-1, 10)
    msg = C.create_string_buffer(256)
    ptr = lambda name, a: None if name in null or not a.size else a.ctypes.data
    rc = rxr.rxr_check_terrain_flatten(ptr("kinds", k), ptr("params", p), ptr("ranges", g), len(k) if n_ops is None else n_ops, ptr("records", r),
                                       len(r) if n_records is None else n_records, msg, 256)
    return rc, msg.value.decode()


def test_what_the_check_refuses():
    op, rec = [0.5, 0.0, 0, 0, 1, 1], [0.0] * 10
    assert check([], [], [], []) == (RXR_OK, "")
    assert check([0, 1], [op, op], [[0, 2], [1, 1]], [rec, rec])[0] == RXR_OK              # overlapping ranges are legal
    assert check([0], [op], [[2, 0]], [rec, rec])[0] == RXR_OK                             # an empty range at the pool's end
    rc, msg = check([2], [op], [[0, 1]], [rec])
    assert rc == RXR_ERR_INVALID and "kind 2" in msg
    for bad in ([0, 3], [2, 1], [3, 0], [0xFFFFFFFF, 2], [1, 0xFFFFFFFF]):
        rc, msg = check([0, 1], [op, op], [[0, 1], bad], [rec, rec])
        assert rc == RXR_ERR_INVALID and "op 1" in msg and "range" in msg, bad
    for name in ("kinds", "params", "ranges", "records"):
        assert check([0], [op], [[0, 1]], [rec], null=(name,))[0] == RXR_ERR_INVALID, name
    many = rusterix_amd.abi.RXR_TERRAIN_FLATTEN_MAX_OPS + 1
    rc, msg = check([0] * many, [op] * many, [[0, 0]] * many, [rec])
    assert rc == RXR_ERR_UNSUPPORTED and "RXR_TERRAIN_FLATTEN_MAX_OPS" in msg
    assert check([0] * (many - 1), [op] * (many - 1), [[0, 0]] * (many - 1), [rec])[0] == RXR_OK
    cap = rusterix_amd.abi.RXR_TERRAIN_FLATTEN_MAX_RECORDS
    rc, msg = check([0], [op], [[0, 1]], [rec] * (cap + 1))
    assert rc == RXR_ERR_UNSUPPORTED and "RXR_TERRAIN_FLATTEN_MAX_RECORDS" in msg
    assert check([0], [op], [[0, cap]], [rec] * cap)[0] == RXR_OK
    rc, msg = check([0, 1], [op, op], [[0, cap], [0, 1]], [rec] * cap)                     # the ranges' sum counts, not the pool alone
    assert rc == RXR_ERR_UNSUPPORTED and "in all" in msg and "RXR_TERRAIN_FLATTEN_MAX_RECORDS" in msg
    segs = rusterix_amd.abi.RXR_TERRAIN_FLATTEN_MAX_SEGMENTS                                # the linedef ops' share has a bound of its own
    assert check([1, 0], [op, op], [[0, segs], [0, segs]], [rec] * segs)[0] == RXR_OK
    rc, msg = check([1, 1], [op, op], [[0, segs], [5, 1]], [rec] * segs)
    assert rc == RXR_ERR_UNSUPPORTED and "RXR_TERRAIN_FLATTEN_MAX_SEGMENTS" in msg
    # a message cut to its capacity stays terminated
    rxr = rusterix_amd.rxr_abi()
    small = C.create_string_buffer(b"\xff" * 8, 8)
    k = np.array([7], np.uint32)
    assert rxr.rxr_check_terrain_flatten(k.ctypes.data, np.zeros(6, np.float32).ctypes.data, np.zeros(2, np.uint32).ctypes.data, 1, None, 0, small, 8) == RXR_ERR_INVALID
    assert small.raw[7] == 0 and len(small.value) == 7


def test_a_refused_list_leaves_the_mirrors_ops_as_they_were(api):
    sc, coords, want = R.case("overlap_first_order")
    t = sc.product(api)
    with pytest.raises(Exception):
        t.set_flatten_ops([5], [[0.5, 0, 0, 0, 1, 1]], [[0, 0]], [])
    heights, present = t.process_heights_cpu(coords)
    assert not R.first_difference(heights[0], present[0], *want[0])
    t.set_flatten_ops([], [], [], [])                                                         # no ops: the registered cells
    heights, present = t.process_heights_cpu(coords)
    assert all(heights[0][ly * 8 + lx] == sc.spec.heights[(lx, ly)] for ly in range(8) for lx in range(8)) and present.all()


def test_the_generated_ffi_is_what_the_header_implies():
    pr = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_ffi.py"), "--check"], capture_output=True, text=True)
    assert pr.returncode == 0, pr.stdout + pr.stderr
    ffi = open(os.path.join(ROOT, "shim", "rusterix-hip-shim", "src", "ffi.rs")).read()
    for name in ("rxr_check_terrain_flatten", "rxr_set_terrain_flatten", "rxr_flatten_terrain", "rxr_flatten_terrain_to", "rxr_set_terrain_height_source",
                 "RXR_TERRAIN_FLATTEN_MAX_OPS", "RXR_TERRAIN_FLATTEN_MAX_RECORDS", "RXR_TERRAIN_HEIGHTS_PROCESSED"):
        assert name in ffi, name


# ---- sanitizers, on a stand-alone program ----------------------------------------------------------------------------------------------
def test_validation_and_registration_are_clean_under_asan_and_ubsan(tmp_path):
    # the static runtimes are looked for BEFORE anything is built: once they are there, a failed build is a failure
    for lib in ("libasan.a", "libubsan.a"):
        found = subprocess.run(["g++", "-print-file-name=" + lib], capture_output=True, text=True).stdout.strip()
        if not os.path.isabs(found) or not os.path.exists(found):
            pytest.skip(f"this g++ has no static {lib}")
    exe = str(tmp_path / "terrain_flatten_asan")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-o", exe, os.path.join(ROOT, "tests", "terrain_flatten_asan_main.cpp")]
    pr = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert pr.returncode == 0, pr.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    pr = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert pr.returncode == 0 and "terrain flatten records under sanitizers: clean" in pr.stdout, (pr.stdout + pr.stderr)[-4000:]
