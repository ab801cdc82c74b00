"""The generated terrain's partition by tiles without a GPU (reference src/chunkbuilder/terrain_generator.rs: partition_by_tiles
:954-1034; src/chunkbuilder/surface_mesh_builder.rs: fix_winding :201-239): the host mirror's CPU partition against the transcription
(tests/terrain_tiles_ref.py) word for word on the shared fuzz scenes, the first-use closed form the device uses against the
reference's dictionary walk, the claim that fix_winding never swaps a generated group -- whatever the heights are --, the refusals of
rxr_check_terrain_tiles, the generated ffi, and the mirror's CPU functions under AddressSanitizer and UBSan in a stand-alone
program."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import rusterix_amd
from rusterix_amd.abi import RXR_ERR_INVALID, RXR_ERR_UNSUPPORTED, RXR_OK
from tests import terrain_exclusion_ref as X
from tests import terrain_gen_ref as G
from tests import terrain_tiles_ref as T
from tests.terrain_exclusion_ref import Exclusions
from tests.terrain_gen_ref import F, Generator
from tests.terrain_tiles_ref import Tiles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")
SENTINEL = F(-12345.75)
SEEDS = [1, 2, 3]
NONE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def api():
    return rusterix_amd.load()


@pytest.fixture(scope="module")
def fuzz():
    """per seed and subdivisions 1 to 3: the generator, exclusions, tiles, boxes and the transcription of every box -- the whole map
    at subdivisions 1 only, the four chunks at all three"""
    out = {}
    for seed in SEEDS:
        excl, boxes = X.fuzz_scene(seed)
        tiles = T.fuzz_tiles(seed)
        for sub in (1, 2, 3):
            gen = G.scene(seed, subdivisions=sub)
            bs = boxes if sub == 1 else boxes[1:]
            out[seed, sub] = (gen, excl, tiles, bs, [T.tile_meshes(gen, excl, tiles, b) for b in bs])
    return out


def test_the_fuzz_scenes_have_both_layouts_many_groups_and_dropped_triangles(fuzz):
    for (seed, sub), (gen, excl, tiles, boxes, results) in fuzz.items():
        assert any(r["keep"] is None for r in results) and any(r["keep"] is not None and not r["keep"].all() for r in results), (seed, sub)
        assert max(r["box_counts"][3] for r in results) >= 5 and min(r["box_counts"][3] for r in results) >= 3, (seed, sub)
        for r in results:
            total = len(r["keep"]) if r["keep"] is not None else 2 * (r["counts"][0] - 1) * (r["counts"][1] - 1)
            kept = int(r["keep"].sum()) if r["keep"] is not None else total
            assert sum(len(g["indices"]) for g in r["groups"]) == kept
            assert [g["slot"] for g in r["groups"]] == sorted({g["slot"] for g in r["groups"]})
    assert sum(len(r["groups"]) for _, _, _, _, results in fuzz.values() for r in results) > 150


# ---- the mirror's CPU partition against the transcription ----
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("sub", [1, 2, 3])
def test_the_mirror_equals_the_transcription_word_for_word(api, fuzz, seed, sub):
    gen, excl, tiles, boxes, results = fuzz[seed, sub]
    mirror = api.TerrainGenerator(**gen.args()).set_exclusions(**excl.args()).set_tiles(**tiles.args())
    cells = max((r["counts"][0] - 1) * (r["counts"][1] - 1) for r in results)
    points = max(r["counts"][0] * r["counts"][1] for r in results)
    mg, vs, ts = 6, 6 * cells + 3, 2 * cells + 3
    box_counts, counts, group_tiles, v, uv, idx = mirror.generate_tile_meshes_cpu(boxes, mg, vs, ts, fill=float(SENTINEL))
    _, h = mirror.grid_heights_cpu(boxes, points)
    for i, res in enumerate(results):
        assert tuple(int(c) for c in box_counts[i]) == res["box_counts"], (i, box_counts[i], res["box_counts"])
        ng = len(res["groups"])
        assert (group_tiles[i, ng:] == NONE).all() and (counts[i, ng:] == 0).all() and (v[i, ng:] == SENTINEL).all() and (uv[i, ng:] == SENTINEL).all()
        for k, g in enumerate(res["groups"]):
            nv, nt = len(g["points"]), len(g["indices"])
            assert int(group_tiles[i, k]) == g["slot"] and tuple(int(c) for c in counts[i, k]) == (nv, nt), (i, k)
            assert (v[i, k, nv:] == SENTINEL).all() and (uv[i, k, nv:] == SENTINEL).all()
            assert np.array_equal(idx[i, k, :nt], g["indices"]), (i, k)
            assert np.array_equal(v[i, k, :nv][:, [0, 2]].view(np.uint32), g["uvs"].view(np.uint32)), (i, k)
            assert np.array_equal(uv[i, k, :nv].view(np.uint32), g["uvs"].view(np.uint32)), (i, k)
            assert (v[i, k, :nv, 3] == F(1.0)).all()
            assert np.array_equal(v[i, k, :nv, 1].view(np.uint32), h[i][g["points"]].view(np.uint32)), (i, k)


def test_the_mirror_leaves_out_a_box_that_does_not_fit(api):
    mirror = api.TerrainGenerator().set_tiles([(0, 0), (1, 1)], [1, 2], 3)
    box_counts, counts, group_tiles, v, uv, idx = mirror.generate_tile_meshes_cpu([(0, 0, 2, 2), (0, 0, 2, 2)], 2, 9, 8, fill=7.0)
    assert box_counts.tolist() == [[3, 3, 0, 0]] * 2 and (counts == 0).all() and (group_tiles == NONE).all() and (v == 7.0).all()   # three groups
    box_counts, counts, group_tiles, v, uv, idx = mirror.generate_tile_meshes_cpu([(0, 0, 2, 2)], 3, 9, 8)
    assert box_counts.tolist() == [[3, 3, 0, 3]] and group_tiles.tolist() == [[0, 1, 2]] and counts[0].tolist() == [[7, 4], [4, 2], [4, 2]]
    assert mirror.generate_tile_meshes_cpu([(0, 0, 2, 2)], 3, 8, 8)[0].tolist() == [[3, 3, 0, 0]]
    assert mirror.generate_tile_meshes_cpu([(0, 0, 2, 2)], 3, 9, 7)[0].tolist() == [[3, 3, 0, 0]]
    with pytest.raises(ValueError):
        mirror.set_tiles([(0, 0), (0, 0)], [1, 2], 3)
    with pytest.raises(ValueError):
        mirror.set_tiles([(0, 0)], [3], 3)


# ---- the first-use closed form against the dictionary walk ----
def slots_of(res):
    tri_slot = np.full(2 * (res["counts"][0] - 1) * (res["counts"][1] - 1), -1, np.int64)
    for g in res["groups"]:
        tri_slot[g["triangles"]] = g["slot"]
    return tri_slot


@pytest.mark.parametrize("seed", SEEDS)
def test_the_first_use_closed_form_equals_the_dictionary_walk(seed):
    # the shared layout: the fuzz tiles without excluded sectors, the map's chunks and two odd boxes, subdivisions 1 to 3
    tiles = T.fuzz_tiles(seed)
    _, boxes = X.fuzz_scene(seed)
    groups = 0
    for sub in (1, 2, 3):
        gen = Generator(subdivisions=sub)
        for box in boxes[1:] + [(-3.5, -2.25, 4.0, 3.0), (44.0, 3.0, 53.0, 4.0)]:
            res = T.tile_meshes(gen, Exclusions(), tiles, box)
            tri_slot = slots_of(res)
            assert (tri_slot >= 0).all()
            closed = T.first_use_closed_form(res["counts"][0], res["counts"][1], tri_slot.tolist())
            assert sorted(closed) == [g["slot"] for g in res["groups"]]
            for g in res["groups"]:
                points, indices = closed[g["slot"]]
                assert np.array_equal(points, g["points"]) and np.array_equal(indices, g["indices"]), (sub, box, g["slot"])
                groups += 1
    assert groups > 60


def test_the_closed_form_on_two_cells_by_hand():
    # cells (0, 0) and (1, 0) of a 3 x 2 grid with slots 0 and 2: the grid points of the shared edge (1 and 4) are in both groups
    closed = T.first_use_closed_form(3, 2, [0, 0, 2, 2])
    assert closed[0][0].tolist() == [0, 3, 1, 4] and closed[2][0].tolist() == [1, 4, 2, 5]
    assert closed[0][1].tolist() == [[0, 1, 2], [2, 1, 3]] and closed[2][1].tolist() == [[0, 1, 2], [2, 1, 3]]
    # ... and with the two triangles of cell (0, 0) in different groups
    closed = T.first_use_closed_form(3, 2, [1, 0, 0, 0])
    assert closed[1][0].tolist() == [0, 3, 1] and closed[0][0].tolist() == [1, 3, 4, 2, 5]
    assert closed[0][1].tolist() == [[0, 1, 2], [0, 2, 3], [3, 2, 4]]


# ---- fix_winding never swaps a generated group ----
def test_fix_winding_swaps_a_mesh_that_faces_down_and_keeps_one_that_faces_up():
    v = np.array([[0, 0, 0, 1], [1, 0, 0, 1], [0, 0, 1, 1]], F)
    assert T.fix_winding(v, [[0, 1, 2]])[1] and not T.fix_winding(v, [[0, 2, 1]])[1]     # (1,0,0) x (0,0,1) = (0,-1,0)
    assert T.fix_winding(v, [[0, 1, 2]])[0].tolist() == [[0, 2, 1]]
    assert not T.fix_winding(v, [[0, 0, 1]])[1]                                           # degenerate: magnitude below 1e-8
    assert not T.fix_winding(v[:2], [[0, 1, 1]])[1] and not T.fix_winding(v, [])[1]


@pytest.mark.parametrize("heights", ["finite", "special"])
def test_fix_winding_swaps_no_group_of_the_fuzz_scenes(fuzz, heights):
    """the y component of every triangle's cross product is cell_z * cell_x - 0 * 0 with exact zeros (two corners of a generated
    triangle share x, two share z), so it is non-negative whatever the heights are; a non-finite height makes the average a NaN, and
    NaN < 0.0 is false"""
    rng = np.random.default_rng(0x7E44E9)
    groups = 0
    for (seed, sub), (gen, excl, tiles, boxes, results) in fuzz.items():
        for res in results:
            h = rng.normal(0.0, 40.0, len(res["points"])).astype(F)   # steep: |slope| far above 1
            if heights == "special":
                pick = rng.random(len(h)) < 0.3
                h[pick] = rng.choice(np.array([INF, -INF, NAN, 3e38, -3e38], F), int(pick.sum()))
            for g in res["groups"]:
                v = np.column_stack([g["uvs"][:, 0], h[g["points"]], g["uvs"][:, 1], np.ones(len(g["points"]), F)]).astype(F)
                out, swapped = T.fix_winding(v, g["indices"])
                assert not swapped and np.array_equal(out, g["indices"]), (seed, sub, g["slot"])
                groups += 1
    assert groups > 150


# ---- rxr_check_terrain_tiles ----
def check(cells=None, slots=None, n=0, n_tiles=1):
    rxr = rusterix_amd.rxr_abi()
    keep = [None if cells is None else np.ascontiguousarray(cells, np.int32), None if slots is None else np.ascontiguousarray(slots, np.uint32)]
    p = [None if a is None else a.ctypes.data for a in keep]
    msg = C.create_string_buffer(256)
    rc = rxr.rxr_check_terrain_tiles(p[0], p[1], n, n_tiles, msg, len(msg))
    return rc, msg.value.decode()


def test_check_accepts():
    assert check() == (RXR_OK, "")
    assert check([(0, 0), (0, 1), (-2 ** 31, 2 ** 31 - 1), (1, 0)], [0, 1, 2, 2], 4, 3)[0] == RXR_OK
    assert check(n_tiles=1 << 12)[0] == RXR_OK


def test_check_refuses_counts_above_the_caps():
    one = np.zeros(16, np.int32)   # (never read: the count is refused first)
    rc, msg = check(one, one, (1 << 20) + 1, 2)
    assert rc == RXR_ERR_UNSUPPORTED and "MAX_CELLS" in msg
    rc, msg = check(one, one, 1, (1 << 12) + 1)
    assert rc == RXR_ERR_UNSUPPORTED and "MAX_TILES" in msg


def test_check_refuses_null_arrays_slots_out_of_range_and_duplicates():
    cells = [(1, 1), (2, 2), (1, 1)]
    for kw in (dict(slots=[0], n=1), dict(cells=cells, n=1)):
        rc, msg = check(**kw)
        assert rc == RXR_ERR_INVALID and "NULL" in msg, (kw, rc, msg)
    rc, msg = check(n_tiles=0)
    assert rc == RXR_ERR_INVALID and "n_tiles" in msg
    rc, msg = check(cells, [0, 2, 0], 2, 2)
    assert rc == RXR_ERR_INVALID and "slots[1]" in msg
    rc, msg = check(cells, [0, 1, 1], 3, 2)
    assert rc == RXR_ERR_INVALID and "(1, 1)" in msg and "twice" in msg and "0 and 2" in msg
    assert check(cells, [0, 1, 1], 2, 2)[0] == RXR_OK
    assert check([(1, -1), (-1, 1), (1, -1)], [0, 0, 0], 3, 1)[0] == RXR_ERR_INVALID   # the same slot twice is still a duplicate cell


def test_the_generated_ffi_is_what_the_header_implies():
    pr = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_ffi.py"), "--check"], capture_output=True, text=True)
    assert pr.returncode == 0, pr.stdout + pr.stderr
    ffi = open(os.path.join(ROOT, "shim", "rusterix-hip-shim", "src", "ffi.rs")).read()
    for name in ("rxr_check_terrain_tiles", "rxr_set_terrain_tiles", "rxr_generated_tile_meshes", "rxr_generated_tile_meshes_to", "RXR_TERRAIN_TILES_MAX_GROUPS"):
        assert name in ffi, name


# ---- sanitizers, on a stand-alone program ----
def test_the_mirror_is_clean_under_asan_and_ubsan(api, tmp_path):
    # (`api`: the program links the device library the build makes; without it the fixture says so)
    # the static runtimes are looked for BEFORE anything is built: once they are there, a failed build or link is a failure
    for lib in ("libasan.a", "libubsan.a"):
        found = subprocess.run(["g++", "-print-file-name=" + lib], capture_output=True, text=True).stdout.strip()
        if not os.path.isabs(found) or not os.path.exists(found):
            pytest.skip(f"this g++ has no static {lib}")
    exe = str(tmp_path / "terrain_tiles_asan")
    csrc = os.path.join(ROOT, "rusterix_amd", "csrc")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-fno-fast-math", "-pthread", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-o", exe, os.path.join(ROOT, "tests", "terrain_tiles_asan_main.cpp"),
           os.path.join(csrc, "host", "rusterix_host.cpp"), "-L" + csrc, "-lrxr_hip", "-Wl,-rpath," + csrc]
    pr = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert pr.returncode == 0, pr.stderr[-4000:]
    # the runtimes are inside the program (-static-libasan): the child takes the environment as it is, plus the sanitizers' options
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    pr = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert pr.returncode == 0 and "terrain tiles under sanitizers: clean" in pr.stdout, (pr.stdout + pr.stderr)[-4000:]
