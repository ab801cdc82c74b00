"""The generated terrain's chunk meshes with their excluded sectors on the device (rxr_terrain_excl.hip: rxr_set_terrain_exclusions,
rxr_generated_meshes and its `_to` form) against the numpy-float32 transcription (tests/terrain_exclusion_ref.py): counts, x, z and w
bit-equal to the transcription, y bit-equal to rxr_generated_grids of the same box in the same context.  Every output buffer is
filled with a sentinel and carries a guard; slots past n_vertices and the guard come back unchanged."""
import ctypes as C

import numpy as np
import pytest

import rusterix_amd
from rusterix_amd.abi import RXR_ERR_INVALID, RXR_ERR_UNSUPPORTED, RXR_OK
from tests import terrain_exclusion_ref as X
from tests import terrain_gen_ref as G
from tests.terrain_exclusion_ref import Exclusions, square
from tests.terrain_gen_ref import F, Generator

pytestmark = pytest.mark.gpu
NAN, INF = float("nan"), float("inf")
SENTINEL = F(-12345.75)
GUARD = 8   # words behind every output


def last_error(rxr, ctx):
    return (rxr.rxr_last_error(ctx) or b"").decode()


def set_generator(rxr, ctx, gen):
    a = [np.ascontiguousarray(x) for x in (gen.control_points, gen.ridges, gen.ridge_edge_offsets, gen.ridge_edges, gen.linedefs, gen.map_box)]
    p = [x.ctypes.data if x.size else None for x in a]
    return rxr.rxr_set_terrain_generator(ctx, p[0], len(a[0]), p[1], len(a[1]), p[2], p[3], len(a[3]), p[4], len(a[4]), p[5])


def set_exclusions(rxr, ctx, excl):
    b, o, v = excl.sector_boxes, excl.vertex_offsets, excl.vertices
    return rxr.rxr_set_terrain_exclusions(ctx, b.ctypes.data if b.size else None, o.ctypes.data, v.ctypes.data if v.size else None, len(b), len(v))


def meshes(rxr, ctx, boxes, subdivisions, stride, expect=RXR_OK):
    """the blocking form into sentinel-filled, guarded buffers: counts [n][4], vertices [n][stride][4]"""
    b = np.ascontiguousarray(np.asarray(boxes, F).reshape(-1, 4))
    n = len(b)
    counts, v = np.full(4 * n + GUARD, 0xABCD, np.uint32), np.full(n * stride * 4 + GUARD, SENTINEL, F)
    rc = rxr.rxr_generated_meshes(ctx, b.ctypes.data, n, subdivisions, stride, counts.ctypes.data, v.ctypes.data)
    assert rc == expect, last_error(rxr, ctx)
    assert (counts[4 * n:] == 0xABCD).all() and (v[n * stride * 4:] == SENTINEL).all()
    return counts[:4 * n].reshape(n, 4), v[:n * stride * 4].reshape(n, stride, 4)


def grid_heights(rxr, ctx, boxes, subdivisions, stride):
    b = np.ascontiguousarray(np.asarray(boxes, F).reshape(-1, 4))
    n = len(b)
    counts, h = np.zeros(2 * n, np.uint32), np.zeros(n * max(stride, 1), F)
    assert rxr.rxr_generated_grids(ctx, b.ctypes.data, n, subdivisions, stride, counts.ctypes.data, h.ctypes.data) == RXR_OK, last_error(rxr, ctx)
    return h.reshape(n, max(stride, 1))


def stride_for(results, slack=5):
    return max(max(6 * max(r["counts"][0] - 1, 0) * max(r["counts"][1] - 1, 0), r["counts"][0] * r["counts"][1]) for r in results) + slack


def compare(rxr, ctx, gen, boxes, results, counts, v):
    """the equality of the header comment, for the boxes of one call"""
    points = max(max(r["counts"][0] * r["counts"][1] for r in results), 1)
    h = grid_heights(rxr, ctx, boxes, gen.subdivisions, points)
    for i, res in enumerate(results):
        nv = res["counts"][3]
        assert tuple(int(c) for c in counts[i]) == res["counts"], (i, counts[i], res["counts"])
        assert (v[i, nv:] == SENTINEL).all(), i   # slots past n_vertices are not written
        if nv:
            want = X.expected_vertices(res)
            assert np.array_equal(v[i, :nv, [0, 2]].T.view(np.uint32), want.view(np.uint32)), i
            assert (v[i, :nv, 3].view(np.uint32) == F(1.0).view(np.uint32)).all()
            assert np.array_equal(v[i, :nv, 1].view(np.uint32), h[i][res["vertex_points"]].view(np.uint32)), i


def run_case(rxr, ctx, gen, excl, boxes, stride=None):
    assert set_generator(rxr, ctx, gen) == RXR_OK, last_error(rxr, ctx)
    assert set_exclusions(rxr, ctx, excl) == RXR_OK, last_error(rxr, ctx)
    results = [X.apply_exclusions(gen, excl, b) for b in boxes]
    stride = stride_for(results) if stride is None else stride
    counts, v = meshes(rxr, ctx, boxes, gen.subdivisions, stride)
    compare(rxr, ctx, gen, boxes, results, counts, v)
    return results, counts, v


@pytest.fixture()
def dev(product):
    return rusterix_amd.rxr_abi(), C.c_void_p(product.lib.rxh_context())


@pytest.fixture(scope="module")
def hills():
    return G.scene(seed=1)


@pytest.fixture(scope="module")
def fuzz():
    """the shared fuzz scenes and their transcription, computed once"""
    out = {}
    for seed in (1, 2):
        excl, boxes = X.fuzz_scene(seed)
        gen = G.scene(seed)
        out[seed] = (gen, excl, boxes, [X.apply_exclusions(gen, excl, b) for b in boxes])
    return out


# ---- the smallest shapes at which each mechanism can fail ----
def test_one_cell_kept_dropped_and_half_dropped(dev, hills):
    rxr, ctx = dev
    box = [(10, 20, 11, 21)]
    res, counts, v = run_case(rxr, ctx, hills, Exclusions([square(30, 30, 31, 31)], boxes=[(10, 20, 11, 21)]), box)
    assert res[0]["counts"] == (2, 2, 1, 6)
    res, _, _ = run_case(rxr, ctx, hills, Exclusions([square(9, 19, 12, 22)]), box)
    assert res[0]["counts"] == (2, 2, 1, 0)
    res, _, v = run_case(rxr, ctx, hills, Exclusions([[(9.5, 19.5), (11.6, 19.5), (9.5, 21.6)]]), box)
    assert res[0]["counts"] == (2, 2, 1, 3) and res[0]["keep"].tolist() == [False, True]
    assert v[0, :3, [0, 2]].T.tolist() == [[11, 20], [10, 21], [11, 21]]
    res, _, _ = run_case(rxr, ctx, hills, Exclusions([[(11.5, 21.5), (9.4, 21.5), (11.5, 19.4)]]), box)
    assert res[0]["keep"].tolist() == [True, False]


def test_a_grid_without_cells_has_no_vertices_in_the_unshared_layout(dev, hills):
    rxr, ctx = dev
    excl = Exclusions([square(0, 0, 20, 20)])
    res, counts, v = run_case(rxr, ctx, hills, excl, [(3, 3, 3, 5), (3, 3, 7, 3), (3, 3, 3, 3), (5, 5, 3, 3), (30, 30, 30, 33)], stride=4)
    assert [r["counts"] for r in res] == [(1, 3, 1, 0), (5, 1, 1, 0), (1, 1, 1, 0), (0, 0, 1, 0), (1, 4, 0, 4)]
    # ... and a stride of 0 holds them
    counts, v = meshes(rxr, ctx, [(3, 3, 3, 5), (5, 5, 3, 3)], 1, 0)
    assert counts.tolist() == [[1, 3, 1, 0], [0, 0, 1, 0]]


@pytest.mark.parametrize("box, cells", [((0, 0, 255, 1), 255), ((0, 0, 16, 16), 256), ((0, 0, 257, 1), 257)])
def test_cell_counts_around_a_round_of_the_scan(dev, hills, box, cells):
    # sectors that take cells out before, across and behind the 256th cell: the carry of the scan's rounds
    rxr, ctx = dev
    excl = Exclusions([square(100.5, -1, 130.5, 2), square(250.5, -1, 300, 2), square(3.5, 3.5, 9.5, 9.5), square(12.5, 12.5, 17, 17)])
    res, _, _ = run_case(rxr, ctx, hills, excl, [box])
    keep = res[0]["keep"]
    assert len(keep) == 2 * cells and not keep[-1] and keep[0] and 0.05 * len(keep) < (~keep).sum() < 0.5 * len(keep)


@pytest.mark.parametrize("box, points", [((0, 0, 8, 6), 63), ((0, 0, 7, 7), 64), ((0, 0, 12, 4), 65)])
def test_point_counts_around_a_wave(dev, hills, box, points):
    rxr, ctx = dev
    res, _, _ = run_case(rxr, ctx, hills, Exclusions([square(2.5, 1.5, 5.5, 4.5), square(6.5, 2.5, 20, 20)]), [box])
    assert res[0]["counts"][0] * res[0]["counts"][1] == points and 0 < (~res[0]["keep"]).sum() < len(res[0]["keep"])


def test_subdivisions_four(dev, hills):
    rxr, ctx = dev
    gen = Generator(**{**hills.args(), "subdivisions": 4})
    excl = Exclusions([[(21.3, 30.1), (23.9, 30.6), (23.2, 33.4), (22.0, 32.0), (20.7, 33.7)], square(22, 28, 23, 29)])
    res, _, _ = run_case(rxr, ctx, gen, excl, [(20, 28, 24, 34), (18.5, 26.25, 22, 30)])
    assert res[0]["counts"][:3] == (17, 25, 2) and 0 < (~res[0]["keep"]).sum() < len(res[0]["keep"])
    assert (res[0]["boundary"] & ~res[0]["ray"]).any()   # the square's top and right edges lie on grid lines


@pytest.mark.parametrize("k", [1, 32, 33, 65])
def test_active_sector_counts_around_a_mask_word(dev, hills, k):
    # sector i holds the four corners of cell (i % 11, 2 * (i // 11)) and of no other: 2 k triangles go, whichever word its bit is in
    rxr, ctx = dev
    polys = [square(i % 11 - 0.25, 2 * (i // 11) - 0.25, i % 11 + 1.25, 2 * (i // 11) + 1.25, clockwise=bool(i & 1)) for i in range(k)]
    res, _, _ = run_case(rxr, ctx, hills, Exclusions(polys), [(0, 0, 12, 12)])
    assert res[0]["counts"][:3] == (13, 13, k) and (~res[0]["keep"]).sum() == 2 * k
    # the last sector alone decides its cell
    last = k - 1
    cell = 12 * 2 * (last // 11) + last % 11
    assert not res[0]["keep"][2 * cell] and not res[0]["keep"][2 * cell + 1]


def test_some_sectors_active_and_layouts_mixed_in_one_call(dev, hills):
    rxr, ctx = dev
    excl = Exclusions([square(2.5, 2.5, 5.5, 5.5), square(20.5, 1.5, 23.5, 6.5), square(40, 40, 42, 42), [(8, 8), (9, 9)]])
    boxes = [(0, 0, 6, 6), (50, 50, 53, 52), (18, 0, 26, 8), (5, 5, 3, 3), (0, 0, 24, 3), (7, 7, 10, 10)]
    res, counts, v = run_case(rxr, ctx, hills, excl, boxes)
    # (the empty box (5, 5, 3, 3) still has an active sector: the four comparisons hold for it)
    assert [r["active"] for r in res] == [[0], [], [1], [0], [0, 1], [3]]
    assert [r["counts"][3] for r in res] == [6 * 36 - 6 * 4, 12, 6 * 64 - 6 * 2 * 4, 0, 6 * 72 - 6 * 2, 54]
    assert rxr.rxr_debug_terrain_excl_launches(ctx) == 1


def test_a_forced_split_gives_the_same_words(dev, fuzz, monkeypatch):
    rxr, ctx = dev
    gen, excl, boxes, results = fuzz[1]
    assert set_generator(rxr, ctx, gen) == RXR_OK and set_exclusions(rxr, ctx, excl) == RXR_OK
    chunks, want = boxes[1:], results[1:]
    stride = stride_for(want)
    counts, v = meshes(rxr, ctx, chunks, 1, stride)
    assert rxr.rxr_debug_terrain_excl_launches(ctx) == 1
    monkeypatch.setenv("RXR_TERRAIN_EXCL_LAUNCH_POINTS", "600")   # 289 points a chunk: two chunks a round
    counts2, v2 = meshes(rxr, ctx, chunks, 1, stride)
    assert rxr.rxr_debug_terrain_excl_launches(ctx) == 2
    monkeypatch.setenv("RXR_TERRAIN_EXCL_LAUNCH_POINTS", "100")   # ... and one (a round takes at least one box)
    counts3, v3 = meshes(rxr, ctx, chunks, 1, stride)
    assert rxr.rxr_debug_terrain_excl_launches(ctx) == 4
    for c, w in ((counts2, v2), (counts3, v3)):
        assert np.array_equal(c, counts) and np.array_equal(w.view(np.uint32), v.view(np.uint32))
    compare(rxr, ctx, gen, chunks, want, counts3, v3)


@pytest.mark.parametrize("seed", [1, 2])
def test_fuzz_scenes(dev, fuzz, seed):
    rxr, ctx = dev
    gen, excl, boxes, results = fuzz[seed]
    assert set_generator(rxr, ctx, gen) == RXR_OK and set_exclusions(rxr, ctx, excl) == RXR_OK
    counts, v = meshes(rxr, ctx, boxes, 1, stride_for(results))
    compare(rxr, ctx, gen, boxes, results, counts, v)
    keep = results[0]["keep"]
    assert 0.1 * len(keep) <= keep.sum() <= 0.9 * len(keep)


# ---- the quirks of tests/test_terrain_exclusion_cpu.py, on the device ----
def test_quirks_of_the_reference(dev):
    rxr, ctx = dev
    flat = Generator()

    def pin(excl, box, want, keep=None):
        res, _, _ = run_case(rxr, ctx, flat, excl, [box])
        assert res[0]["counts"] == want, res[0]["counts"]
        if keep is not None:
            assert res[0]["keep"].tolist() == [bool(x) for x in keep]
        return res[0]

    tri = [(5, 1), (7, 1), (6, 3)]
    up = float(np.nextafter(F(4), F(INF)))
    pin(Exclusions([[(1, 1), (2, 2)]]), (0, 0, 4, 4), (5, 5, 1, 96), [1] * 32)                 # two vertices: active, holds nothing
    pin(Exclusions([[]], boxes=[(1, 1, 2, 2)]), (0, 0, 4, 4), (5, 5, 1, 96))
    pin(Exclusions([tri], boxes=[(up, 1, 7, 3)]), (0, 0, 4, 4), (5, 5, 0, 25))                 # one ulp away
    pin(Exclusions([tri], boxes=[(4, 1, 7, 3)]), (0, 0, 4, 4), (5, 5, 1, 96))                  # touching
    pin(Exclusions([tri], boxes=[(3.75, 1, 7, 3)]), (0.5, 0.5, 3.5, 3.5), (5, 5, 0, 25))       # the box as given decides
    pin(Exclusions([square(1, 1, 3, 3)], boxes=[(1, NAN, 3, 3)]), (0, 0, 4, 4), (5, 5, 0, 25))   # a NaN box
    pin(Exclusions([square(1, 1, 3, 3)]), (0, 0, NAN, 4), (1, 5, 0, 5))
    pin(Exclusions([square(-0.5, -0.5, 0.5, 1.5), square(0.75, -0.5, 2.5, 1.5)]), (0, 0, 2, 1), (3, 2, 2, 6), [1, 1, 0, 0])   # corners in different sectors
    pin(Exclusions([[(-0.5, -0.5), (1.6, -0.5), (-0.5, 1.6)]]), (0, 0, 1, 1), (2, 2, 1, 3), [0, 1])   # (i0, i2, i1) without i3
    twice = [(0.5, 0.5), (0.5, 0.5), (2.5, 0.5), (2.5, 2.5), (2.5, 2.5), (0.5, 2.5)]
    pin(Exclusions([twice]), (0, 0, 3, 3), (4, 4, 1, 48))                                      # zero-length edges
    pin(Exclusions([[(1, 1), (1, 1), (1, 1)]]), (0, 0, 2, 2), (3, 3, 1, 24), [1] * 8)
    res, _, _ = run_case(rxr, ctx, flat, Exclusions([[(0.5, 0.5), (NAN, 0.5), (2.5, 2.5), (0.5, 2.5)]], boxes=[(0, 0, 3, 3)]), [(0, 0, 3, 3)])   # a NaN vertex
    assert res[0]["counts"][:3] == (4, 4, 1)
    pin(Exclusions([[(NAN, NAN)] * 3], boxes=[(0, 0, 3, 3)]), (0, 0, 3, 3), (4, 4, 1, 54))
    r = pin(Exclusions([square(1.005, 1.005, 2.995, 2.995)]), (0, 0, 4, 4), (5, 5, 1, 72))     # the epsilon band: 0.005 outside is inside
    assert r["boundary"].sum() == 8
    pin(Exclusions([square(1.02, 1.02, 2.98, 2.98)]), (0, 0, 4, 4), (5, 5, 1, 96), [1] * 32)   # ... and 0.02 outside is outside


# ---- forms, refusals, lifetime ----
def test_to_form_equals_blocking_on_a_callers_stream(dev, fuzz):
    import torch

    rxr, ctx = dev
    gen, excl, boxes, results = fuzz[2]
    assert set_generator(rxr, ctx, gen) == RXR_OK and set_exclusions(rxr, ctx, excl) == RXR_OK
    chunks = np.ascontiguousarray(boxes[1:], F)
    n, stride = len(chunks), stride_for(results[1:])
    want_counts, want_v = meshes(rxr, ctx, chunks, 1, stride)
    for stream in (None, torch.cuda.Stream()):
        sp = C.c_void_p(stream.cuda_stream) if stream is not None else None
        dc = torch.full((4 * n + GUARD,), 0xABCD, dtype=torch.int32, device="cuda")
        dv = torch.full((n * stride * 4 + GUARD,), float(SENTINEL), device="cuda")
        torch.cuda.synchronize()
        assert rxr.rxr_generated_meshes_to(ctx, chunks.ctypes.data, n, 1, stride, dc.data_ptr(), dv.data_ptr(), sp) == RXR_OK, last_error(rxr, ctx)
        # a second call queued behind the first reuses the scratch in order, and a re-registration waits for both
        assert rxr.rxr_generated_meshes_to(ctx, chunks.ctypes.data, n, 1, stride, dc.data_ptr(), dv.data_ptr(), sp) == RXR_OK, last_error(rxr, ctx)
        assert set_exclusions(rxr, ctx, Exclusions()) == RXR_OK
        assert rxr.rxr_synchronize(ctx) == RXR_OK
        if stream is not None:
            stream.synchronize()
        c, v = dc.cpu().numpy().view(np.uint32), dv.cpu().numpy()
        assert (c[4 * n:] == 0xABCD).all() and (v[n * stride * 4:] == SENTINEL).all()
        assert np.array_equal(c[:4 * n].reshape(n, 4), want_counts)
        assert np.array_equal(v[:n * stride * 4].view(np.uint32), want_v.reshape(-1).view(np.uint32))
        assert set_exclusions(rxr, ctx, excl) == RXR_OK
    # host memory where device memory is expected, a misaligned pointer, NULL, n == 0
    host_counts = np.zeros(4 * n, np.uint32)
    assert rxr.rxr_generated_meshes_to(ctx, chunks.ctypes.data, n, 1, stride, host_counts.ctypes.data, dv.data_ptr(), None) == RXR_ERR_INVALID and "dev_counts" in last_error(rxr, ctx)
    assert rxr.rxr_generated_meshes_to(ctx, chunks.ctypes.data, n, 1, stride, dc.data_ptr(), want_v.ctypes.data, None) == RXR_ERR_INVALID and "dev_vertices" in last_error(rxr, ctx)
    assert rxr.rxr_generated_meshes_to(ctx, chunks.ctypes.data, n, 1, stride, dc.data_ptr(), dv.data_ptr() + 2, None) == RXR_ERR_INVALID
    assert rxr.rxr_generated_meshes_to(ctx, chunks.ctypes.data, n, 1, stride, None, dv.data_ptr(), None) == RXR_ERR_INVALID
    assert rxr.rxr_generated_meshes_to(ctx, None, 0, 1, stride, None, None, None) == RXR_OK
    assert rxr.rxr_synchronize(ctx) == RXR_OK


def test_refusals_queue_nothing(dev, hills):
    rxr, ctx = dev
    assert set_generator(rxr, ctx, hills) == RXR_OK and set_exclusions(rxr, ctx, Exclusions([square(1, 1, 2, 2)])) == RXR_OK
    boxes = [(10, 10, 12, 12), (0, 0, 3, 3)]   # 9 shared vertices; 54 slots of the unshared layout
    counts, v = meshes(rxr, ctx, boxes, 1, 53, expect=RXR_ERR_INVALID)
    assert "box 1" in last_error(rxr, ctx) and (v == SENTINEL).all() and (counts == 0xABCD).all()
    counts, v = meshes(rxr, ctx, boxes, 1, 54)
    assert counts.tolist() == [[3, 3, 0, 9], [4, 4, 1, 48]]
    counts, v = meshes(rxr, ctx, boxes[:1], 1, 8, expect=RXR_ERR_INVALID)
    assert "box 0" in last_error(rxr, ctx) and (v == SENTINEL).all()
    meshes(rxr, ctx, boxes, 0, 54, expect=RXR_ERR_INVALID)
    assert "subdivisions" in last_error(rxr, ctx)
    b = np.ascontiguousarray(boxes, F)
    assert rxr.rxr_generated_meshes(ctx, b.ctypes.data, 2, 1, 54, None, v.ctypes.data) == RXR_ERR_INVALID and "NULL" in last_error(rxr, ctx)
    assert rxr.rxr_generated_meshes(ctx, b.ctypes.data, 2, 1, 54, counts.ctypes.data, None) == RXR_ERR_INVALID
    assert rxr.rxr_generated_meshes(ctx, None, 2, 1, 54, counts.ctypes.data, v.ctypes.data) == RXR_ERR_INVALID
    assert rxr.rxr_generated_meshes(ctx, b.ctypes.data, 0xFFFFFFFF, 1, 0xFFFFFFFF, counts.ctypes.data, v.ctypes.data) == RXR_ERR_INVALID and "overflow" in last_error(rxr, ctx)
    assert rxr.rxr_generated_meshes(ctx, None, 0, 1, 54, None, None) == RXR_OK
    # an extent whose `as i32` saturates wraps to a negative step: an empty grid, in either layout
    counts, v = meshes(rxr, ctx, [(0, 0, INF, 1), (0, 0, 3, 3e9)], 1, 4)
    assert counts.tolist() == [[0, 2, 1, 0], [4, 0, 1, 0]] and (v == SENTINEL).all()


def test_registration_lifetime_on_a_context_of_its_own(product, hills):
    rxr = rusterix_amd.rxr_abi()
    ctx = C.c_void_p()
    assert rxr.rxr_create(C.byref(ctx), 0) == RXR_OK
    try:
        box = [(0, 0, 4, 4)]
        excl = Exclusions([square(0.5, 0.5, 2.5, 2.5)])
        assert set_exclusions(rxr, ctx, excl) == RXR_OK   # independent of the generator: registered first
        meshes(rxr, ctx, box, 1, 96, expect=RXR_ERR_INVALID)
        assert "no terrain generator" in last_error(rxr, ctx)
        assert set_generator(rxr, ctx, hills) == RXR_OK
        first = X.apply_exclusions(hills, excl, box[0])
        counts, v = meshes(rxr, ctx, box, 1, 96)
        compare(rxr, ctx, hills, box, [first], counts, v)
        assert first["counts"] == (5, 5, 1, 96 - 6)
        # a refused call changes nothing: offsets that do not end at the vertex count, a count above its cap
        z = np.zeros(8, F)
        off = np.array([0, 3], np.uint32)
        assert rxr.rxr_set_terrain_exclusions(ctx, z.ctypes.data, off.ctypes.data, z.ctypes.data, 1, 4) == RXR_ERR_INVALID and "vertex_offsets" in last_error(rxr, ctx)
        assert rxr.rxr_set_terrain_exclusions(ctx, z.ctypes.data, off.ctypes.data, z.ctypes.data, (1 << 12) + 1, 4) == RXR_ERR_UNSUPPORTED
        counts2, v2 = meshes(rxr, ctx, box, 1, 96)
        assert np.array_equal(counts2, counts) and np.array_equal(v2.view(np.uint32), v.view(np.uint32))
        # re-registration between calls changes the answer
        other = Exclusions([square(1.5, 1.5, 3.5, 3.5), square(10, 10, 11, 11)])
        assert set_exclusions(rxr, ctx, other) == RXR_OK
        second = X.apply_exclusions(hills, other, box[0])
        counts, v = meshes(rxr, ctx, box, 1, 96)
        compare(rxr, ctx, hills, box, [second], counts, v)
        assert not np.array_equal(second["keep"], first["keep"]) and second["counts"] == first["counts"]
        # S == 0 after S > 0 is the shared layout again
        assert set_exclusions(rxr, ctx, Exclusions()) == RXR_OK
        counts, v = meshes(rxr, ctx, box, 1, 96)
        compare(rxr, ctx, hills, box, [X.apply_exclusions(hills, Exclusions(), box[0])], counts, v)
        assert counts.tolist() == [[5, 5, 0, 25]]
    finally:
        rxr.rxr_destroy(ctx)


def test_no_exclusions_registered_is_the_grid(product, hills):
    rxr = rusterix_amd.rxr_abi()
    ctx = C.c_void_p()
    assert rxr.rxr_create(C.byref(ctx), 0) == RXR_OK
    try:
        assert set_generator(rxr, ctx, hills) == RXR_OK
        boxes = [(20.0, 28.5, 27.0, 31.0), (-3.5, -2.25, 1.25, 0.5)]
        results = [X.apply_exclusions(hills, Exclusions(), b) for b in boxes]
        counts, v = meshes(rxr, ctx, boxes, 1, 40)
        compare(rxr, ctx, hills, boxes, results, counts, v)
        assert counts.tolist() == [[8, 4, 0, 32], [7, 5, 0, 35]]
    finally:
        rxr.rxr_destroy(ctx)


def test_multi_device_handles(product, hills):
    rxr = rusterix_amd.rxr_abi()
    multi = C.c_void_p()
    devs = (C.c_int * 2)(0, 0)
    assert rxr.rxr_create_multi(C.byref(multi), devs, 2) == RXR_OK
    try:
        excl = Exclusions([square(0.5, 0.5, 2.5, 2.5)])
        assert set_generator(rxr, multi, hills) == RXR_OK and set_exclusions(rxr, multi, excl) == RXR_OK, last_error(rxr, multi)
        counts, v = meshes(rxr, multi, [(0, 0, 4, 4)], 1, 96)
        compare(rxr, multi, hills, [(0, 0, 4, 4)], [X.apply_exclusions(hills, excl, (0, 0, 4, 4))], counts, v)
        assert rxr.rxr_debug_terrain_excl_launches(multi) == 1
        b = np.zeros(4, F)
        assert rxr.rxr_generated_meshes_to(multi, b.ctypes.data, 1, 1, 4, b.ctypes.data, b.ctypes.data, None) == RXR_ERR_UNSUPPORTED and "multi-device" in last_error(rxr, multi)
    finally:
        rxr.rxr_destroy(multi)


def test_the_mirror_registers_its_lists_when_they_changed(product, fuzz):
    gen, excl, boxes, results = fuzz[1]
    mirror = product.TerrainGenerator(**gen.args()).set_exclusions(**excl.args())
    stride = stride_for(results[1:])
    counts, v = mirror.generate_meshes(boxes[1:], stride, fill=float(SENTINEL))
    ccounts, cv = mirror.generate_meshes_cpu(boxes[1:], stride, fill=float(SENTINEL))
    assert np.array_equal(counts, ccounts) and [tuple(int(x) for x in c) for c in counts] == [r["counts"] for r in results[1:]]
    assert np.array_equal(v[..., [0, 2, 3]].view(np.uint32), cv[..., [0, 2, 3]].view(np.uint32))
    _, h = mirror.grid_heights(boxes[1:], 289)
    for i, r in enumerate(results[1:]):
        nv = r["counts"][3]
        assert np.array_equal(v[i, :nv, 1].view(np.uint32), h[i][r["vertex_points"]].view(np.uint32)) and (v[i, nv:] == SENTINEL).all()
    other = Exclusions([square(20.5, 4.5, 28.5, 12.5)])
    mirror.set_exclusions(**other.args())
    counts, v = mirror.generate_meshes(boxes[1:2], stride)
    assert tuple(int(x) for x in counts[0]) == X.apply_exclusions(gen, other, boxes[1])["counts"]
    with pytest.raises(Exception):
        mirror.generate_meshes(boxes[1:2], 100)
