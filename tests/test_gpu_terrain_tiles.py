"""The generated terrain's per-tile chunk meshes on the device (rxr_terrain_excl.hip: rxr_set_terrain_tiles, rxr_generated_tile_meshes
and its `_to` form) against the numpy-float32 transcription of partition_by_tiles (tests/terrain_tiles_ref.py): box_counts, counts,
group_tiles, indices, x, z, w and uvs bit-equal to the transcription, y bit-equal to rxr_generated_grids' word for that grid point in
the same context.  Every output buffer is filled with a sentinel and carries a guard; slots past a mesh's counts and the guards come
back unchanged."""
import ctypes as C

import numpy as np
import pytest

import rusterix_amd
from rusterix_amd.abi import RXR_ERR_INVALID, RXR_ERR_UNSUPPORTED, RXR_OK
from tests import terrain_exclusion_ref as X
from tests import terrain_gen_ref as G
from tests import terrain_tiles_ref as T
from tests.terrain_exclusion_ref import Exclusions, square
from tests.terrain_gen_ref import F, Generator
from tests.terrain_tiles_ref import Tiles

pytestmark = pytest.mark.gpu
SENTINEL = F(-12345.75)
ISENT = 0xABCDABCD
GUARD = 8   # words behind every output
NONE = 0xFFFFFFFF


def last_error(rxr, ctx):
    return (rxr.rxr_last_error(ctx) or b"").decode()


def set_generator(rxr, ctx, gen):
    a = [np.ascontiguousarray(x) for x in (gen.control_points, gen.ridges, gen.ridge_edge_offsets, gen.ridge_edges, gen.linedefs, gen.map_box)]
    p = [x.ctypes.data if x.size else None for x in a]
    return rxr.rxr_set_terrain_generator(ctx, p[0], len(a[0]), p[1], len(a[1]), p[2], p[3], len(a[3]), p[4], len(a[4]), p[5])


def set_exclusions(rxr, ctx, excl):
    b, o, v = excl.sector_boxes, excl.vertex_offsets, excl.vertices
    return rxr.rxr_set_terrain_exclusions(ctx, b.ctypes.data if b.size else None, o.ctypes.data, v.ctypes.data if v.size else None, len(b), len(v))


def set_tiles(rxr, ctx, tiles):
    c, s = np.ascontiguousarray(tiles.cells), np.ascontiguousarray(tiles.slots)
    return rxr.rxr_set_terrain_tiles(ctx, c.ctypes.data if c.size else None, s.ctypes.data if s.size else None, len(s), tiles.n_tiles)


class Out:
    """sentinel-filled, guarded host buffers of one call"""

    def __init__(self, n, mg, vs, ts):
        self.shape = (n, mg, vs, ts)
        m = n * mg
        self.sizes = [4 * n, 2 * m, m, m * vs * 4, m * vs * 2, m * ts * 3]
        self.raw = [np.full(self.sizes[0] + GUARD, ISENT, np.uint32), np.full(self.sizes[1] + GUARD, ISENT, np.uint32), np.full(self.sizes[2] + GUARD, ISENT, np.uint32),
                    np.full(self.sizes[3] + GUARD, SENTINEL, F), np.full(self.sizes[4] + GUARD, SENTINEL, F), np.full(self.sizes[5] + GUARD, ISENT, np.uint32)]

    def pointers(self):
        return [a.ctypes.data for a in self.raw]

    def guards_intact(self):
        return all((a[k:] == (SENTINEL if a.dtype == F else ISENT)).all() for a, k in zip(self.raw, self.sizes))

    def untouched(self):
        return all((a == (SENTINEL if a.dtype == F else ISENT)).all() for a in self.raw)

    def views(self):
        n, mg, vs, ts = self.shape
        r, k = self.raw, self.sizes
        return (r[0][:k[0]].reshape(n, 4), r[1][:k[1]].reshape(n, mg, 2), r[2][:k[2]].reshape(n, mg), r[3][:k[3]].reshape(n, mg, vs, 4),
                r[4][:k[4]].reshape(n, mg, vs, 2), r[5][:k[5]].reshape(n, mg, ts, 3))

    def same_words(self, other):
        return all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(self.raw, other.raw))


def tile_meshes(rxr, ctx, boxes, subdivisions, mg, vs, ts, expect=RXR_OK):
    b = np.ascontiguousarray(np.asarray(boxes, F).reshape(-1, 4))
    out = Out(len(b), mg, vs, ts)
    rc = rxr.rxr_generated_tile_meshes(ctx, b.ctypes.data, len(b), subdivisions, mg, vs, ts, *out.pointers())
    assert rc == expect, last_error(rxr, ctx)
    assert out.guards_intact()
    if expect != RXR_OK:
        assert out.untouched()
    return out


def grid_heights(rxr, ctx, boxes, subdivisions, stride):
    b = np.ascontiguousarray(np.asarray(boxes, F).reshape(-1, 4))
    n = len(b)
    counts, h = np.zeros(2 * n, np.uint32), np.zeros(n * max(stride, 1), F)
    assert rxr.rxr_generated_grids(ctx, b.ctypes.data, n, subdivisions, stride, counts.ctypes.data, h.ctypes.data) == RXR_OK, last_error(rxr, ctx)
    return h.reshape(n, max(stride, 1))


def groups_bound(tiles, res):
    """the library's bound of a box's groups: slot 0 and the distinct other slots among the override cells between the floor of the
    grid's first and the ceil of its last coordinate"""
    pts = res["points"]
    if res["counts"][0] < 2 or res["counts"][1] < 2:
        return 1
    x0, x1, z0, z1 = np.floor(pts[:, 0].min()), np.ceil(pts[:, 0].max()) - 1, np.floor(pts[:, 1].min()), np.ceil(pts[:, 1].max()) - 1
    return 1 + len({s for (x, z), s in tiles.map.items() if s and x0 <= x <= x1 and z0 <= z <= z1})


def strides_for(results, tiles, slack=3):
    """(max_groups, vertex_stride, triangle_stride) the call needs at least; the strides a little above it"""
    vs = ts = 0
    for r in results:
        sx, sy = r["counts"][0], r["counts"][1]
        cells = max(sx - 1, 0) * max(sy - 1, 0)
        vs = max(vs, 6 * cells if r["counts"][2] else (sx * sy if cells else 0))
        ts = max(ts, 2 * cells)
    return max(groups_bound(tiles, r) for r in results), vs + slack, ts + slack


def compare(rxr, ctx, gen, boxes, results, out):
    """the equality of the header comment, for the boxes of one call"""
    box_counts, counts, group_tiles, v, uv, idx = out.views()
    mg = out.shape[1]
    points = max(max(r["counts"][0] * r["counts"][1] for r in results), 1)
    h = grid_heights(rxr, ctx, boxes, gen.subdivisions, points)
    for i, res in enumerate(results):
        assert tuple(int(c) for c in box_counts[i]) == res["box_counts"], (i, box_counts[i], res["box_counts"])
        ng = len(res["groups"])
        assert (group_tiles[i, ng:] == NONE).all() and (counts[i, ng:] == 0).all(), i
        assert (v[i, ng:] == SENTINEL).all() and (uv[i, ng:] == SENTINEL).all() and (idx[i, ng:] == ISENT).all(), i
        for k, g in enumerate(res["groups"]):
            nv, nt = len(g["points"]), len(g["indices"])
            assert int(group_tiles[i, k]) == g["slot"] and tuple(int(c) for c in counts[i, k]) == (nv, nt), (i, k, group_tiles[i, k], counts[i, k], g["slot"], nv, nt)
            assert (v[i, k, nv:] == SENTINEL).all() and (uv[i, k, nv:] == SENTINEL).all() and (idx[i, k, nt:] == ISENT).all(), (i, k)   # slots past the counts
            assert np.array_equal(idx[i, k, :nt], g["indices"]), (i, k)
            assert np.array_equal(v[i, k, :nv][:, [0, 2]].view(np.uint32), g["uvs"].view(np.uint32)), (i, k)
            assert np.array_equal(uv[i, k, :nv].view(np.uint32), g["uvs"].view(np.uint32)), (i, k)
            assert (v[i, k, :nv, 3].view(np.uint32) == F(1.0).view(np.uint32)).all()
            assert np.array_equal(v[i, k, :nv, 1].view(np.uint32), h[i][g["points"]].view(np.uint32)), (i, k)


def run_case(rxr, ctx, gen, excl, tiles, boxes, strides=None):
    assert set_generator(rxr, ctx, gen) == RXR_OK, last_error(rxr, ctx)
    assert set_exclusions(rxr, ctx, excl) == RXR_OK, last_error(rxr, ctx)
    assert set_tiles(rxr, ctx, tiles) == RXR_OK, last_error(rxr, ctx)
    results = [T.tile_meshes(gen, excl, tiles, b) for b in boxes]
    mg, vs, ts = strides or strides_for(results, tiles)
    out = tile_meshes(rxr, ctx, boxes, gen.subdivisions, mg, vs, ts)
    compare(rxr, ctx, gen, boxes, results, out)
    return results, out


@pytest.fixture()
def dev(product):
    rxr, ctx = rusterix_amd.rxr_abi(), C.c_void_p(product.lib.rxh_context())
    yield rxr, ctx
    set_tiles(rxr, ctx, Tiles())   # the process-wide context goes on to other tests


@pytest.fixture(scope="module")
def hills():
    return G.scene(seed=1)


@pytest.fixture(scope="module")
def fuzz():
    """the shared fuzz scenes and their transcription, computed once"""
    out = {}
    for seed in (1, 2):
        excl, boxes = X.fuzz_scene(seed)
        gen, tiles = G.scene(seed), T.fuzz_tiles(seed)
        out[seed] = (gen, excl, tiles, boxes, [T.tile_meshes(gen, excl, tiles, b) for b in boxes])
    return out


# ---- the smallest shapes at which each mechanism can fail ----
def test_one_cell_without_and_with_an_override(dev, hills):
    rxr, ctx = dev
    box = [(10, 20, 11, 21)]
    res, out = run_case(rxr, ctx, hills, Exclusions(), Tiles(), box)
    assert res[0]["box_counts"] == (2, 2, 0, 1) and res[0]["groups"][0]["indices"].tolist() == [[0, 1, 2], [2, 1, 3]]
    assert res[0]["groups"][0]["points"].tolist() == [0, 2, 1, 3]   # first use: (i0, i2, i1), then i3
    res, out = run_case(rxr, ctx, hills, Exclusions(), Tiles({(10, 20): 3}, n_tiles=5), box)
    assert res[0]["box_counts"] == (2, 2, 0, 1) and [g["slot"] for g in res[0]["groups"]] == [3]
    # an override next door changes nothing, and the unshared layout of the same cell has six vertices
    res, out = run_case(rxr, ctx, hills, Exclusions([square(30, 30, 31, 31)], boxes=[(10, 20, 11, 21)]), Tiles({(11, 20): 1, (10, 21): 1, (9, 20): 1}), box, strides=(1, 6, 2))
    assert res[0]["box_counts"] == (2, 2, 1, 1) and res[0]["groups"][0]["slot"] == 0 and len(res[0]["groups"][0]["points"]) == 6


def test_two_cells_with_different_slots_share_an_edge(dev, hills):
    rxr, ctx = dev
    res, out = run_case(rxr, ctx, hills, Exclusions(), Tiles({(5, 7): 2}), [(4, 7, 6, 8)])
    g0, g2 = res[0]["groups"]
    assert (g0["slot"], g2["slot"]) == (0, 2) and res[0]["box_counts"] == (3, 2, 0, 2)
    # grid points 1 and 4 (x == 5) are in both groups, each in its own first-use order
    assert g0["points"].tolist() == [0, 3, 1, 4] and g2["points"].tolist() == [1, 4, 2, 5]
    assert g0["indices"].tolist() == [[0, 1, 2], [2, 1, 3]] and g2["indices"].tolist() == [[0, 1, 2], [2, 1, 3]]


@pytest.mark.parametrize("pattern", ["stripes", "checkerboard"])
@pytest.mark.parametrize("cells_x, cells_z", [(8, 8), (9, 8), (16, 16), (17, 16)])
def test_cell_counts_around_a_wave_and_a_round(dev, hills, cells_x, cells_z, pattern):
    # vertical stripes: every group straddles every wave and round edge (the carry of the per-group counters); a checkerboard: many
    # groups alternate inside a wave
    rxr, ctx = dev
    tiles = Tiles(T.stripes(0, 32, 0, 32, 3) if pattern == "stripes" else T.checkerboard(0, 32, 0, 32, 5))
    res, out = run_case(rxr, ctx, hills, Exclusions(), tiles, [(0, 0, cells_x, cells_z)])
    assert res[0]["box_counts"] == (cells_x + 1, cells_z + 1, 0, 3 if pattern == "stripes" else 5)
    assert sum(len(g["indices"]) for g in res[0]["groups"]) == 2 * cells_x * cells_z
    # ... and the same cells in the unshared layout (an active sector that holds no point)
    res, out = run_case(rxr, ctx, hills, Exclusions([[(1, 1), (2, 2)]], boxes=[(0, 0, 1, 1)]), tiles, [(0, 0, cells_x, cells_z)])
    assert res[0]["box_counts"][2] == 1 and sum(len(g["points"]) for g in res[0]["groups"]) == 6 * cells_x * cells_z


@pytest.mark.parametrize("subdivisions", [1, 2, 3])
def test_subdivisions_and_negative_cells(dev, hills, subdivisions):
    # a third is inexact in f32; negative coordinates tell floor from truncation
    rxr, ctx = dev
    gen = Generator(**{**hills.args(), "subdivisions": subdivisions})
    tiles = Tiles({**T.checkerboard(-5, 6, -4, 5, 4), (20, 28): 7})
    res, out = run_case(rxr, ctx, gen, Exclusions(), tiles, [(-3.5, -2.25, 4.0, 3.0), (20, 28, 22, 29.5)])
    assert res[0]["box_counts"] == (8 * subdivisions + 1, 6 * subdivisions + 1, 0, 4)
    assert [g["slot"] for g in res[1]["groups"]] == [0, 7] and len(res[1]["groups"][1]["indices"]) == 2 * subdivisions ** 2


@pytest.mark.parametrize("seed", [1, 2])
def test_fuzz_scenes(dev, fuzz, seed):
    # the exclusion fuzz scene with the tile fuzz: both layouts, triangles dropped in the middle of a group
    rxr, ctx = dev
    gen, excl, tiles, boxes, results = fuzz[seed]
    assert set_generator(rxr, ctx, gen) == RXR_OK and set_exclusions(rxr, ctx, excl) == RXR_OK and set_tiles(rxr, ctx, tiles) == RXR_OK
    mg, vs, ts = strides_for(results, tiles)
    out = tile_meshes(rxr, ctx, boxes, 1, mg, vs, ts)
    compare(rxr, ctx, gen, boxes, results, out)
    keep = results[0]["keep"]
    assert 0.1 * len(keep) <= keep.sum() <= 0.9 * len(keep) and len(results[0]["groups"]) == 6
    assert any(r["keep"] is None for r in results) and rxr.rxr_debug_terrain_tile_launches(ctx) == 1


def test_a_slot_inside_an_excluded_square_has_no_group(dev, hills):
    rxr, ctx = dev
    tiles = Tiles({(3, 3): 2, (4, 3): 2, (6, 6): 1, (1, 1): 3})
    excl = Exclusions([square(2.5, 2.5, 5.5, 4.5)])
    res, out = run_case(rxr, ctx, hills, excl, tiles, [(0, 0, 8, 8)], strides=(4, 6 * 64, 128))
    assert [g["slot"] for g in res[0]["groups"]] == [0, 1, 3] and res[0]["box_counts"] == (9, 9, 1, 3)
    # triangles dropped in the middle of group 0: its triangle ids have a gap where the square lies
    assert not res[0]["keep"].all() and len(res[0]["groups"][0]["indices"]) == 128 - 4 - (~res[0]["keep"]).sum()


def test_max_groups_is_a_bound_on_what_the_box_can_have(dev, hills):
    rxr, ctx = dev
    assert set_generator(rxr, ctx, hills) == RXR_OK and set_exclusions(rxr, ctx, Exclusions()) == RXR_OK
    box = [(0, 0, 4, 4)]
    four = Tiles({(0, 0): 1, (1, 1): 2, (2, 2): 3, (4, 0): 9, (0, 4): 9, (-1, 2): 9})   # the 9s lie outside the box's cells
    assert set_tiles(rxr, ctx, four) == RXR_OK
    res = [T.tile_meshes(hills, Exclusions(), four, box[0])]
    out = tile_meshes(rxr, ctx, box, 1, 4, 25, 32)   # exactly max_groups groups fit
    compare(rxr, ctx, hills, box, res, out)
    assert res[0]["box_counts"][3] == 4
    tile_meshes(rxr, ctx, box, 1, 3, 25, 32, expect=RXR_ERR_INVALID)   # one more than max_groups
    assert "box 0" in last_error(rxr, ctx) and "4 tile groups" in last_error(rxr, ctx)
    # the conservative refusal: every cell overridden, so slot 0 never occurs and there would be two groups -- the bound says three
    full = Tiles({(x, z): 1 + (x & 1) for x in range(4) for z in range(4)})
    assert set_tiles(rxr, ctx, full) == RXR_OK
    tile_meshes(rxr, ctx, box, 1, 2, 25, 32, expect=RXR_ERR_INVALID)
    out = tile_meshes(rxr, ctx, box, 1, 3, 25, 32)
    compare(rxr, ctx, hills, box, [T.tile_meshes(hills, Exclusions(), full, box[0])], out)
    assert out.views()[0][0].tolist() == [5, 5, 0, 2]
    # ... and an override cell whose triangles are all excluded still counts
    assert set_tiles(rxr, ctx, Tiles({(1, 1): 5})) == RXR_OK and set_exclusions(rxr, ctx, Exclusions([square(0.5, 0.5, 2.5, 2.5)])) == RXR_OK
    tile_meshes(rxr, ctx, box, 1, 1, 96, 32, expect=RXR_ERR_INVALID)
    out = tile_meshes(rxr, ctx, box, 1, 2, 96, 32)
    assert out.views()[0][0].tolist() == [5, 5, 1, 1]


def test_grids_without_a_cell_have_no_group(dev, hills):
    rxr, ctx = dev
    assert set_generator(rxr, ctx, hills) == RXR_OK and set_exclusions(rxr, ctx, Exclusions([square(0, 0, 20, 20)])) == RXR_OK and set_tiles(rxr, ctx, Tiles({(3, 3): 1})) == RXR_OK
    boxes = [(5, 5, 3, 3), (3, 3, 3, 5), (30, 30, 30, 33), (0, 0, float("inf"), 1)]   # a negative step; one column, in either layout; a saturated extent
    out = tile_meshes(rxr, ctx, boxes, 1, 2, 4, 4)
    box_counts, counts, group_tiles, v, uv, idx = out.views()
    assert box_counts.tolist() == [[0, 0, 1, 0], [1, 3, 1, 0], [1, 4, 0, 0], [0, 2, 1, 0]]
    assert (counts == 0).all() and (group_tiles == NONE).all() and (v == SENTINEL).all() and (uv == SENTINEL).all() and (idx == ISENT).all()
    # ... and strides of 0 hold them
    out = tile_meshes(rxr, ctx, boxes[:2], 1, 1, 0, 0)
    assert out.views()[0].tolist() == [[0, 0, 1, 0], [1, 3, 1, 0]]


def test_a_forced_split_gives_the_same_words(dev, fuzz, monkeypatch):
    rxr, ctx = dev
    gen, excl, tiles, boxes, results = fuzz[1]
    assert set_generator(rxr, ctx, gen) == RXR_OK and set_exclusions(rxr, ctx, excl) == RXR_OK and set_tiles(rxr, ctx, tiles) == RXR_OK
    chunks, want = boxes[1:], results[1:]
    mg, vs, ts = strides_for(want, tiles)
    one = tile_meshes(rxr, ctx, chunks, 1, mg, vs, ts)
    assert rxr.rxr_debug_terrain_tile_launches(ctx) == 1
    monkeypatch.setenv("RXR_TERRAIN_EXCL_LAUNCH_POINTS", "600")   # 289 points a chunk: two chunks a round
    two = tile_meshes(rxr, ctx, chunks, 1, mg, vs, ts)
    assert rxr.rxr_debug_terrain_tile_launches(ctx) == 2
    monkeypatch.setenv("RXR_TERRAIN_EXCL_LAUNCH_POINTS", "100")   # ... and one (a round takes at least one box)
    four = tile_meshes(rxr, ctx, chunks, 1, mg, vs, ts)
    assert rxr.rxr_debug_terrain_tile_launches(ctx) == 4
    assert two.same_words(one) and four.same_words(one)
    compare(rxr, ctx, gen, chunks, want, four)


# ---- forms, refusals, lifetime ----
def test_to_form_equals_blocking_on_a_callers_stream(dev, fuzz):
    import torch

    rxr, ctx = dev
    gen, excl, tiles, boxes, results = fuzz[2]
    assert set_generator(rxr, ctx, gen) == RXR_OK and set_exclusions(rxr, ctx, excl) == RXR_OK and set_tiles(rxr, ctx, tiles) == RXR_OK
    chunks = np.ascontiguousarray(boxes[1:], F)
    n = len(chunks)
    mg, vs, ts = strides_for(results[1:], tiles)
    want = tile_meshes(rxr, ctx, chunks, 1, mg, vs, ts)
    for stream in (None, torch.cuda.Stream()):
        sp = C.c_void_p(stream.cuda_stream) if stream is not None else None
        dev_out = [torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda() for a in Out(n, mg, vs, ts).raw]
        torch.cuda.synchronize()
        p = [d.data_ptr() for d in dev_out]
        assert rxr.rxr_generated_tile_meshes_to(ctx, chunks.ctypes.data, n, 1, mg, vs, ts, *p, sp) == RXR_OK, last_error(rxr, ctx)
        # a second call queued behind the first reuses the scratch in order, and a re-registration waits for both
        assert rxr.rxr_generated_tile_meshes_to(ctx, chunks.ctypes.data, n, 1, mg, vs, ts, *p, sp) == RXR_OK, last_error(rxr, ctx)
        assert set_tiles(rxr, ctx, Tiles()) == RXR_OK
        assert rxr.rxr_synchronize(ctx) == RXR_OK
        if stream is not None:
            stream.synchronize()
        for d, w in zip(dev_out, want.raw):
            assert np.array_equal(d.cpu().numpy().view(np.uint32), w.view(np.uint32))
        assert set_tiles(rxr, ctx, tiles) == RXR_OK
    # host memory where device memory is expected, a misaligned pointer, NULL, n == 0
    names = ["dev_box_counts", "dev_counts", "dev_group_tiles", "dev_vertices", "dev_uvs", "dev_indices"]
    for k, name in enumerate(names):
        q = list(p)
        q[k] = want.raw[k].ctypes.data
        assert rxr.rxr_generated_tile_meshes_to(ctx, chunks.ctypes.data, n, 1, mg, vs, ts, *q, None) == RXR_ERR_INVALID and name in last_error(rxr, ctx)
        q[k] = None
        assert rxr.rxr_generated_tile_meshes_to(ctx, chunks.ctypes.data, n, 1, mg, vs, ts, *q, None) == RXR_ERR_INVALID and "NULL" in last_error(rxr, ctx)
    q = list(p)
    q[3] += 2
    assert rxr.rxr_generated_tile_meshes_to(ctx, chunks.ctypes.data, n, 1, mg, vs, ts, *q, None) == RXR_ERR_INVALID
    assert rxr.rxr_generated_tile_meshes_to(ctx, None, 0, 1, mg, vs, ts, None, None, None, None, None, None, None) == RXR_OK
    assert rxr.rxr_synchronize(ctx) == RXR_OK
    for d, w in zip(dev_out, want.raw):   # the refused calls wrote nothing
        assert np.array_equal(d.cpu().numpy().view(np.uint32), w.view(np.uint32))


def test_refusals_queue_nothing(dev, hills):
    rxr, ctx = dev
    assert set_generator(rxr, ctx, hills) == RXR_OK and set_exclusions(rxr, ctx, Exclusions([square(1, 1, 2, 2)])) == RXR_OK and set_tiles(rxr, ctx, Tiles()) == RXR_OK
    boxes = [(10, 10, 12, 12), (0, 0, 3, 3)]   # shared: 9 vertices, 8 triangles; unshared: 54 vertices, 18 triangles
    tile_meshes(rxr, ctx, boxes, 1, 1, 53, 18, expect=RXR_ERR_INVALID)
    assert "box 1" in last_error(rxr, ctx) and "vertex_stride" in last_error(rxr, ctx)
    tile_meshes(rxr, ctx, boxes, 1, 1, 54, 17, expect=RXR_ERR_INVALID)
    assert "box 1" in last_error(rxr, ctx) and "triangle_stride" in last_error(rxr, ctx)
    tile_meshes(rxr, ctx, boxes[:1], 1, 1, 8, 8, expect=RXR_ERR_INVALID)
    assert "box 0" in last_error(rxr, ctx)
    out = tile_meshes(rxr, ctx, boxes, 1, 1, 54, 18)
    assert out.views()[0].tolist() == [[3, 3, 0, 1], [4, 4, 1, 1]] and out.views()[1].tolist() == [[[9, 8]], [[48, 16]]]
    tile_meshes(rxr, ctx, boxes, 0, 1, 54, 18, expect=RXR_ERR_INVALID)
    assert "subdivisions" in last_error(rxr, ctx)
    tile_meshes(rxr, ctx, boxes, 1, 0, 54, 18, expect=RXR_ERR_INVALID)
    assert "max_groups" in last_error(rxr, ctx)
    tile_meshes(rxr, ctx, boxes, 1, 65, 54, 18, expect=RXR_ERR_UNSUPPORTED)
    b = np.ascontiguousarray(boxes, F)
    p = out.pointers()
    for k in range(6):
        q = list(p)
        q[k] = None
        assert rxr.rxr_generated_tile_meshes(ctx, b.ctypes.data, 2, 1, 1, 54, 18, *q) == RXR_ERR_INVALID and "NULL" in last_error(rxr, ctx)
    assert rxr.rxr_generated_tile_meshes(ctx, None, 2, 1, 1, 54, 18, *p) == RXR_ERR_INVALID
    assert rxr.rxr_generated_tile_meshes(ctx, b.ctypes.data, 0xFFFFFFFF, 1, 64, 0xFFFFFFFF, 18, *p) == RXR_ERR_INVALID and "overflow" in last_error(rxr, ctx)
    assert rxr.rxr_generated_tile_meshes(ctx, None, 0, 1, 1, 54, 18, None, None, None, None, None, None) == RXR_OK


def test_registration_lifetime_on_a_context_of_its_own(product, hills):
    rxr = rusterix_amd.rxr_abi()
    ctx = C.c_void_p()
    assert rxr.rxr_create(C.byref(ctx), 0) == RXR_OK
    try:
        box = [(0, 0, 4, 4)]
        first = Tiles(T.stripes(0, 4, 0, 4, 2))
        assert set_tiles(rxr, ctx, first) == RXR_OK   # independent of the generator: registered first
        tile_meshes(rxr, ctx, box, 1, 2, 25, 32, expect=RXR_ERR_INVALID)
        assert "no terrain generator" in last_error(rxr, ctx)
        assert set_generator(rxr, ctx, hills) == RXR_OK
        out = tile_meshes(rxr, ctx, box, 1, 2, 25, 32)
        compare(rxr, ctx, hills, box, [T.tile_meshes(hills, Exclusions(), first, box[0])], out)
        # a refused registration changes nothing: a cell listed twice, a slot out of range, a count above its cap
        cells, slots = np.array([[1, 1], [2, 2], [1, 1]], np.int32), np.array([1, 1, 0], np.uint32)
        assert rxr.rxr_set_terrain_tiles(ctx, cells.ctypes.data, slots.ctypes.data, 3, 2) == RXR_ERR_INVALID and "twice" in last_error(rxr, ctx)
        assert rxr.rxr_set_terrain_tiles(ctx, cells.ctypes.data, slots.ctypes.data, 2, 1) == RXR_ERR_INVALID and "n_tiles" in last_error(rxr, ctx)
        assert rxr.rxr_set_terrain_tiles(ctx, cells.ctypes.data, slots.ctypes.data, 2, (1 << 12) + 1) == RXR_ERR_UNSUPPORTED
        assert tile_meshes(rxr, ctx, box, 1, 2, 25, 32).same_words(out)
        # re-registration between calls changes the answer
        second = Tiles(T.stripes(0, 4, 0, 4, 2, vertical=False))
        assert set_tiles(rxr, ctx, second) == RXR_OK
        out2 = tile_meshes(rxr, ctx, box, 1, 2, 25, 32)
        compare(rxr, ctx, hills, box, [T.tile_meshes(hills, Exclusions(), second, box[0])], out2)
        assert not out2.same_words(out)
        # n_cells == 0 after a non-empty map: everything is slot 0
        assert set_tiles(rxr, ctx, Tiles()) == RXR_OK
        out3 = tile_meshes(rxr, ctx, box, 1, 1, 25, 32)
        compare(rxr, ctx, hills, box, [T.tile_meshes(hills, Exclusions(), Tiles(), box[0])], out3)
        assert out3.views()[0].tolist() == [[5, 5, 0, 1]] and out3.views()[1].tolist() == [[[25, 32]]]
    finally:
        rxr.rxr_destroy(ctx)


def test_never_registered_is_slot_zero_everywhere(product, hills):
    rxr = rusterix_amd.rxr_abi()
    ctx = C.c_void_p()
    assert rxr.rxr_create(C.byref(ctx), 0) == RXR_OK
    try:
        assert set_generator(rxr, ctx, hills) == RXR_OK
        boxes = [(20.0, 28.5, 27.0, 31.0), (-3.5, -2.25, 1.25, 0.5)]
        results = [T.tile_meshes(hills, Exclusions(), Tiles(), b) for b in boxes]
        out = tile_meshes(rxr, ctx, boxes, 1, 1, 40, 60)
        compare(rxr, ctx, hills, boxes, results, out)
        assert out.views()[0].tolist() == [[8, 4, 0, 1], [7, 5, 0, 1]]
    finally:
        rxr.rxr_destroy(ctx)


def test_multi_device_handles(product, hills):
    rxr = rusterix_amd.rxr_abi()
    multi = C.c_void_p()
    devs = (C.c_int * 2)(0, 0)
    assert rxr.rxr_create_multi(C.byref(multi), devs, 2) == RXR_OK
    try:
        tiles = Tiles({(1, 1): 1})
        assert set_generator(rxr, multi, hills) == RXR_OK and set_tiles(rxr, multi, tiles) == RXR_OK, last_error(rxr, multi)
        out = tile_meshes(rxr, multi, [(0, 0, 4, 4)], 1, 2, 25, 32)
        compare(rxr, multi, hills, [(0, 0, 4, 4)], [T.tile_meshes(hills, Exclusions(), tiles, (0, 0, 4, 4))], out)
        assert rxr.rxr_debug_terrain_tile_launches(multi) == 1
        b = np.zeros(4, F)
        p = [b.ctypes.data] * 6
        assert rxr.rxr_generated_tile_meshes_to(multi, b.ctypes.data, 1, 1, 1, 4, 4, *p, None) == RXR_ERR_UNSUPPORTED and "multi-device" in last_error(rxr, multi)
    finally:
        rxr.rxr_destroy(multi)


# ---- the chain: tile meshes -> vertex normals -> update of the registered meshes, on one stream ----
def host_meshes(gen, tiles, boxes, normals_of):
    """the transcription's tile meshes of `boxes` (no excluded sectors; heights without a powf site are bit-defined) as rxr_set_meshes
    takes them, in mesh-slot order"""
    out = []
    for box in boxes:
        res = T.tile_meshes(gen, Exclusions(), tiles, box)
        h, sites, _, _, _ = gen.sample(res["points"])
        assert (sites == 0).all()
        for g in res["groups"]:
            v = np.column_stack([g["uvs"][:, 0], h[g["points"]], g["uvs"][:, 1], np.ones(len(g["points"]), F)]).astype(F)
            out.append(dict(vertices=v, indices=g["indices"], uvs=g["uvs"], normals=normals_of(v, g["indices"]), list=3))
    return out


def test_the_chain_updates_registered_meshes_without_the_host(product):
    import torch

    from tests.test_gpu_mesh_update import Ctx

    boxes = [(0, 0, 4, 4), (4, 0, 8, 4)]
    tiles = Tiles(T.stripes(0, 8, 0, 4, 2, width=2))   # two stripes a box: every box has exactly max_groups = 2 groups
    before = Generator([(3.0, 2.0, 2.5, 1.5), (6.5, 1.0, 1.0, 1.0)], map_box=(-20, -20, 28, 24))
    after = Generator([(4.5, 2.5, 3.0, 1.5), (6.5, 1.0, 1.0, 1.0)], map_box=(-20, -20, 28, 24))   # one control point moved
    mg, vs, ts, n = 2, 25, 32, 2
    a, b = Ctx(), Ctx()
    try:
        def normals_of(v, idx):   # the device's own normals, through the blocking form
            counts, nr = np.array([[len(v), len(idx)]], np.uint32), np.zeros((len(v), 3), F)
            i = np.ascontiguousarray(idx, np.uint32)
            assert b.rxr.rxr_vertex_normals(b.ctx, 1, counts.ctypes.data, v.ctypes.data, i.ctypes.data, nr.ctypes.data, len(v), len(idx)) == RXR_OK, b.error()
            return nr

        old, new = host_meshes(before, tiles, boxes, normals_of), host_meshes(after, tiles, boxes, normals_of)
        assert len(old) == len(new) == 4 and [len(m["vertices"]) for m in old] == [len(m["vertices"]) for m in new] == [15] * 4
        assert all(not np.array_equal(o["vertices"], w["vertices"]) for o, w in zip(old[:2], new[:2]))
        a.set_meshes(old)                                                   # 1. the four meshes, registered
        b.set_meshes(new)                                                   # ... and what they must become, registered from the host
        assert set_generator(a.rxr, a.ctx, after) == RXR_OK and set_tiles(a.rxr, a.ctx, tiles) == RXR_OK   # 2. the control point moves
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            d_box, d_counts, d_tiles = (torch.zeros(k, dtype=torch.int32, device="cuda") for k in (4 * n, 2 * n * mg, n * mg))
            d_v, d_uv, d_nr = (torch.full((n * mg * vs * k,), float(SENTINEL), device="cuda") for k in (4, 2, 3))
            d_idx = torch.zeros(n * mg * ts * 3, dtype=torch.int32, device="cuda")
        bx = np.ascontiguousarray(boxes, F)
        sp = C.c_void_p(s.cuda_stream)
        rc = a.rxr.rxr_generated_tile_meshes_to(a.ctx, bx.ctypes.data, n, 1, mg, vs, ts, d_box.data_ptr(), d_counts.data_ptr(), d_tiles.data_ptr(), d_v.data_ptr(), d_uv.data_ptr(),
                                                d_idx.data_ptr(), sp)                                       # 3. one stream, nothing crosses PCIe
        assert rc == RXR_OK, a.error()
        rc = a.rxr.rxr_vertex_normals_to(a.ctx, n * mg, d_counts.data_ptr(), d_v.data_ptr(), d_idx.data_ptr(), d_nr.data_ptr(), None, vs, ts, sp)
        assert rc == RXR_OK, a.error()
        named = np.arange(n * mg, dtype=np.uint32)
        rc = a.rxr.rxr_update_meshes_to(a.ctx, named.ctypes.data, n * mg, d_counts.data_ptr(), d_v.data_ptr(), d_idx.data_ptr(), d_nr.data_ptr(), vs, ts, sp)
        assert rc == RXR_OK, a.error()
        torch.cuda.synchronize()
        assert d_box.cpu().numpy().reshape(n, 4).tolist() == [[5, 5, 0, 2]] * 2 and d_tiles.cpu().numpy().tolist() == [0, 1, 0, 1]
        a.meshes = list(new)
        for k in range(n * mg):                                             # 4. the boxes and the rays' hits of the two contexts
            for got, want in zip(a.bounds(k), b.bounds(k)):
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), k
        rng = np.random.default_rng(0x7E44EA)
        o = np.column_stack([rng.uniform(0.7, 7.3, 24), np.full(24, 30.0), rng.uniform(0.7, 3.3, 24)]).astype(F)
        d = np.column_stack([rng.uniform(-0.02, 0.02, 24), np.full(24, -1.0), rng.uniform(-0.02, 0.02, 24)]).astype(F)
        got, want = a.intersect(o, d, full=True), b.intersect(o, d, full=True)
        assert (want["mesh"] < 4).sum() >= 20 and len(set(want["mesh"].tolist())) >= 4
        for key in want:
            assert np.array_equal(got[key].view(np.uint32), want[key].view(np.uint32)), key
    finally:
        a.close()
        b.close()


def test_the_mirror_registers_its_lists_when_they_changed(product, fuzz):
    gen, excl, tiles, boxes, results = fuzz[1]
    mirror = product.TerrainGenerator(**gen.args()).set_exclusions(**excl.args()).set_tiles(**tiles.args())
    mg, vs, ts = strides_for(results[1:], tiles)
    got = mirror.generate_tile_meshes(boxes[1:], mg, vs, ts, fill=float(SENTINEL))
    cpu = mirror.generate_tile_meshes_cpu(boxes[1:], mg, vs, ts, fill=float(SENTINEL))
    for k, (x, y) in enumerate(zip(got, cpu)):
        if k == 3:   # the heights are the device's and the CPU's
            x, y = x[..., [0, 2, 3]], y[..., [0, 2, 3]]
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint32), np.ascontiguousarray(y).view(np.uint32)), k
    assert [tuple(int(c) for c in bc) for bc in got[0]] == [r["box_counts"] for r in results[1:]]
    other = Tiles(T.stripes(16, 32, 0, 16, 2))
    mirror.set_tiles(**other.args())
    got = mirror.generate_tile_meshes(boxes[1:2], 2, vs, ts)
    assert tuple(int(c) for c in got[0][0]) == T.tile_meshes(gen, excl, other, boxes[1])["box_counts"]
    with pytest.raises(Exception):
        mirror.generate_tile_meshes(boxes[1:2], 1, vs, ts)


# ---- end to end: the host mirror's Scene ----
W, H = 160, 96
CHAIN_BOXES = [(0, 0, 4, 4), (4, 0, 8, 4)]


def generated_scene(api, gen, tiles):
    """two chunks of 4 x 4 cells, their tile groups as the chunks' batches3d (from the mirror's CPU partition), a light and a camera;
    returns (mirror generator, scene, render)"""
    from rusterix_amd import binding as B

    mirror = api.TerrainGenerator(**gen.args()).set_tiles(**tiles.args())
    box_counts, counts, group_tiles, v, uv, idx = mirror.generate_tile_meshes_cpu(CHAIN_BOXES, 2, 25, 32)
    scene = api.Scene.empty()
    for b in range(2):
        chunk = scene.add_chunk()
        for g in range(int(box_counts[b, 3])):
            nv, nt = (int(c) for c in counts[b, g])
            colour = (60 + 150 * g, 220 - 90 * b, 90 + 60 * g, 255)
            chunk.add_batch3d(api.Batch3D.new(v[b, g, :nv], idx[b, g, :nt], uv[b, g, :nv]).with_computed_normals().source(B.PixelSource.Pixel(colour)))
    scene.lights([B.Light(B.LIGHT_POINT).with_position((4.0, 9.0, 2.0)).with_color((1.0, 0.95, 0.8)).with_intensity(3.0).with_start_distance(2.0)
                  .with_end_distance(60.0).compile()])
    cam = api.D3OrbitCamera.new()
    cam.set_parameter_f32("distance", 12.0)
    cam.center = (4.0, 0.0, 2.0)
    cam.azimuth, cam.elevation = 0.9, 0.8
    assets = api.Assets.default()

    def render():
        vm, pm = cam.matrices(float(W), float(H))
        out = np.zeros(W * H * 4, np.uint8)
        api.Rasterizer.setup(None, vm, pm).ambient((0.5, 0.5, 0.5, 1.0)).rasterize(scene, out, W, H, 32, assets)
        return out.reshape(H, W, 4)

    return mirror, scene, render


def test_a_moved_control_point_through_the_mirrors_scene(product):
    api = product
    tiles = Tiles(T.stripes(0, 8, 0, 4, 2, width=2))
    before = Generator([(3.0, 2.0, 2.5, 1.5), (6.5, 1.0, 1.0, 1.0)], map_box=(-20, -20, 28, 24))
    after = Generator([(4.5, 2.5, 3.0, 1.5), (6.5, 1.0, 1.0, 1.0)], map_box=(-20, -20, 28, 24))
    api.lib.rxh_set_device_projection(1)
    try:
        _, _, want_render = generated_scene(api, after, tiles)
        want = want_render()
        _, scene, render = generated_scene(api, before, tiles)
        first = render()
        assert first.tobytes() != want.tobytes()
        moved = api.TerrainGenerator(**after.args()).set_tiles(**tiles.args())
        assert scene.rebuild_generated_tile_meshes(moved, CHAIN_BOXES, [0, 1], 2) == 0   # the fast path: the registration is held
        got = render()
        assert got.tobytes() == want.tobytes(), int((got != want).any(axis=2).sum())
        hit = scene.intersect([[4.5, 50.0, 2.5]], [[0.0, -1.0, 0.0]])
        assert hit["mesh"][0] == 2 and 2.0 < hit["hitpoint"][0][1] <= 3.0   # chunk 1's first group, under the moved control point (height 3.0)
        # a chunk whose number of groups changed is refused on the fast path too, before anything is written over a registered mesh
        other = api.TerrainGenerator(**before.args()).set_tiles(**Tiles({(0, 0): 1}).args())
        with pytest.raises(Exception, match="tile groups"):
            scene.rebuild_generated_tile_meshes(other, CHAIN_BOXES, [0, 1], 2)
        assert render().tobytes() == want.tobytes()
        # no registration of this geometry is held: the host path, and the next rasterize registers the scene again
        _, scene2, render2 = generated_scene(api, before, tiles)
        assert scene2.rebuild_generated_tile_meshes(moved, CHAIN_BOXES, [0, 1], 2) == 1
        assert render2().tobytes() == want.tobytes()
        # a chunk whose number of groups changed is the caller's to rebuild
        with pytest.raises(Exception, match="tile groups"):
            scene2.rebuild_generated_tile_meshes(other, CHAIN_BOXES, [0, 1], 2)
    finally:
        api.lib.rxh_set_device_projection(0)
