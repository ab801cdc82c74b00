"""The generated terrain's height field on the device (rxr_terrain_gen.hip: rxr_set_terrain_generator, rxr_generated_heights,
rxr_generated_grids and their `_to` forms) against the numpy-float32 transcription (tests/terrain_gen_ref.py) by the two-class rule
of tests/test_terrain_gen_cpu.py: bit-equal where no powf was evaluated, inside the transcription's interval elsewhere.  Every
output buffer is filled with a sentinel and carries a guard; words past a grid's count and the guard come back unchanged."""
import ctypes as C

import numpy as np
import pytest

import rusterix_amd
from rusterix_amd.abi import RXR_ERR_INVALID, RXR_ERR_UNSUPPORTED, RXR_OK
from tests import terrain_gen_ref as G
from tests.terrain_gen_ref import F, Generator

pytestmark = pytest.mark.gpu
NAN, INF = float("nan"), float("inf")
SENTINEL = F(-12345.75)
GUARD = 8   # words behind every output


def last_error(rxr, ctx):
    return (rxr.rxr_last_error(ctx) or b"").decode()


def register(rxr, ctx, gen):
    a = [np.ascontiguousarray(x) for x in (gen.control_points, gen.ridges, gen.ridge_edge_offsets, gen.ridge_edges, gen.linedefs, gen.map_box)]
    p = [x.ctypes.data if x.size else None for x in a]
    return rxr.rxr_set_terrain_generator(ctx, p[0], len(a[0]), p[1], len(a[1]), p[2], p[3], len(a[3]), p[4], len(a[4]), p[5])


def heights(rxr, ctx, points, normals=False):
    """the blocking form into sentinel-filled, guarded buffers"""
    p = np.ascontiguousarray(np.asarray(points, F).reshape(-1, 2))
    n = len(p)
    h, nr = np.full(n + GUARD, SENTINEL, F), np.full(3 * n + GUARD, SENTINEL, F)
    rc = rxr.rxr_generated_heights(ctx, p.ctypes.data, n, h.ctypes.data, nr.ctypes.data if normals else None)
    assert rc == RXR_OK, last_error(rxr, ctx)
    assert (h[n:] == SENTINEL).all() and (nr[3 * n if normals else 0:] == SENTINEL).all()
    return (h[:n], nr[:3 * n].reshape(n, 3)) if normals else h[:n]


def grids(rxr, ctx, boxes, subdivisions, stride, expect=RXR_OK):
    b = np.ascontiguousarray(np.asarray(boxes, F).reshape(-1, 4))
    n = len(b)
    counts, h = np.full(2 * n + GUARD, 0xABCD, np.uint32), np.full(n * stride + GUARD, SENTINEL, F)
    rc = rxr.rxr_generated_grids(ctx, b.ctypes.data, n, subdivisions, stride, counts.ctypes.data, h.ctypes.data)
    assert rc == expect, last_error(rxr, ctx)
    assert (counts[2 * n:] == 0xABCD).all() and (h[n * stride:] == SENTINEL).all()
    return counts[:2 * n].reshape(n, 2), h[:n * stride].reshape(n, stride)


@pytest.fixture()
def dev(product):
    return rusterix_amd.rxr_abi(), C.c_void_p(product.lib.rxh_context())


@pytest.fixture(scope="module")
def sampled():
    """the scenes and their transcription, computed once"""
    out = {}
    for name, kw in (("hills_ridges_roads", dict(seed=1)), ("many_roads", dict(seed=2, n_control=2, n_ridges=1, n_lines=6))):
        gen, pts = G.scene(**kw), G.scene_points(kw["seed"], 193)   # (193: three waves and a lane)
        out[name] = (gen, pts, gen.sample(pts))
    return out


@pytest.mark.parametrize("name", ["hills_ridges_roads", "many_roads"])
def test_scenes_by_the_two_class_rule(dev, sampled, name):
    rxr, ctx = dev
    gen, pts, ref = sampled[name]
    assert register(rxr, ctx, gen) == RXR_OK, last_error(rxr, ctx)
    rec = G.compare(name, heights(rxr, ctx, pts), ref)
    print(name, rec)
    assert rxr.rxr_debug_terrain_gen_launches(ctx) == 1


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_point_counts_around_a_wave(dev, sampled, n):
    rxr, ctx = dev
    gen, pts, ref = sampled["hills_ridges_roads"]
    assert register(rxr, ctx, gen) == RXR_OK
    G.compare(f"n={n}", heights(rxr, ctx, pts[:n]), tuple(a[:n] for a in ref), min_class_share=None)


def test_one_point_more_than_a_launch(dev, sampled, monkeypatch):
    rxr, ctx = dev
    gen, pts, ref = sampled["hills_ridges_roads"]
    assert register(rxr, ctx, gen) == RXR_OK
    monkeypatch.setenv("RXR_TERRAIN_GEN_LAUNCH_POINTS", "96")
    G.compare("split", heights(rxr, ctx, pts), ref)
    assert rxr.rxr_debug_terrain_gen_launches(ctx) == 3   # 96 + 96 + 1
    h, nr = heights(rxr, ctx, pts[:97], normals=True)
    assert rxr.rxr_debug_terrain_gen_launches(ctx) == 2
    G.compare("split normals", h, tuple(a[:97] for a in ref), min_class_share=None)


def test_normals_equal_three_separate_height_calls(dev, sampled):
    rxr, ctx = dev
    gen, pts, ref = sampled["many_roads"]
    assert register(rxr, ctx, gen) == RXR_OK
    h, nr = heights(rxr, ctx, pts, normals=True)
    hc = heights(rxr, ctx, pts)
    hr = heights(rxr, ctx, pts + np.array([F(0.1), F(0.0)], F))
    hu = heights(rxr, ctx, pts + np.array([F(0.0), F(0.1)], F))
    assert np.array_equal(h.view(np.uint32), hc.view(np.uint32))
    want = np.array([G.normal_from_heights(*t) for t in zip(hc, hr, hu)])
    assert np.array_equal(nr.view(np.uint32), want.view(np.uint32)), np.nonzero((nr.view(np.uint32) != want.view(np.uint32)).any(axis=1))[0][:8]
    assert len(np.unique(nr, axis=0)) > 50


@pytest.mark.parametrize("n_control", [0, 1, 2, 17])
def test_control_point_counts(dev, n_control):
    # (the kernel stages no tile of records: they arrive through scalar loads, one control point an iteration)
    rxr, ctx = dev
    rng = np.random.default_rng(n_control)
    cps = np.column_stack([rng.uniform(10, 50, n_control), rng.uniform(10, 50, n_control), rng.uniform(1, 5, n_control), rng.uniform(1, 8, n_control)])
    gen = Generator(cps, map_box=(0, 0, 64, 64))
    pts = np.concatenate([G.scene_points(7, 60), cps[:, :2].astype(F)])   # ... and the control points themselves: exact matches
    assert register(rxr, ctx, gen) == RXR_OK
    ref = gen.sample(pts)
    G.compare(f"C={n_control}", heights(rxr, ctx, pts), ref, min_class_share=None)
    assert n_control == 0 or np.abs(ref[0]).max() > 0.5


def test_pins_of_the_reference(dev):
    rxr, ctx = dev

    def pin(gen, pts, want):
        assert register(rxr, ctx, gen) == RXR_OK, last_error(rxr, ctx)
        got = heights(rxr, ctx, pts)
        assert np.array_equal(got.view(np.uint32), np.asarray(want, F).view(np.uint32)), (got, want)

    # two coincident control points with different heights under a query point: the first wins
    pin(Generator([(10, 10, 2, 1), (10, 10, 5, 1)]), [(10, 10)], [2.0])
    pin(Generator([(10, 10, 5, 1), (10, 10, 2, 1)]), [(10, 10)], [5.0])
    # control points with negative heights only: the base is 0 (and -3 on the control point itself)
    pin(Generator([(10, 10, -3, 2), (12, 10, -1, 2)]), [(10.5, 10), (11, 10), (30, 30), (10, 10)], [0.0, 0.0, 0.0, -3.0])
    # t = 0.5 at the radius; height * smoothstep on a control point in the edge band; 0 outside the map box
    pin(Generator([(50, 50, 4, 2)]), [(54, 50), (50, 46), (58, 50)], [2.0, 2.0, 0.0])
    pin(Generator([(-95, 0, 3, 1), (-95, 1, 9, 50)]), [(-95, 0), (150, 0)], [1.5, 0.0])
    # ridges: zero edges, one degenerate edge, a query point on a vertex (distance 0: the plateau), the band (0.5^2 is exact in any powf)
    pin(Generator([], [(7, 1, 4, 2), (2, 5, 1, 1)], [0, 0, 1], [(3, 4, 3, 4)]), [(0, 0), (3, 4)], [2.0, 2.0])
    pin(Generator([], [(2, 1, 4, 2)], [0, 1], [(0, 0, 10, 0)]), [(0, 0), (10, 0), (5, 0.5), (5, 3), (5, 5), (13, 4)], [2.0, 2.0, 2.0, 0.5, 0.0, 0.0])
    # linedefs: none, one, and overlapping ones whose total influence exceeds 1
    pin(Generator([(20, 20, 4, 2)], map_box=(0, 0, 64, 64)), [(24, 20)], [2.0])
    pin(Generator(linedefs=[(0, 0, 8, 0, 1, 5, 1, 1, 1)]), [(2, 0.5), (-3, 0), (4, 5)], [2.0, 0.0, 0.0])
    pin(Generator(linedefs=[(0, 0, 10, 0, 1, 1, 2, 3, 2), (0, 1, 10, 1, 3, 3, 2, 3, 2)]), [(5, 0)], [1.5])
    pin(Generator(linedefs=[(0, 0, 10, 0, 1, 1, 2, 3, 2), (0, 1, 10, 1, 3, 3, 2, 3, 2), (0, -1, 10, -1, 5, 5, 2, 3, 2)]), [(5, 0)], [5 * (1 - 1.0) + 0 * 1.0])


def test_three_overlapping_roads_by_the_rule(dev):
    rxr, ctx = dev
    gen = Generator([(30, 30, 3, 6)], linedefs=[(4, 28, 60, 30, 1, 2, 1, 6, 2), (4, 31, 60, 29, 2, 0, 1.5, 5, 0.7), (30, 4, 31, 60, 0.5, 1.5, 1, 7, 1.5)], map_box=(0, 0, 64, 64))
    pts = G.scene_points(11, 128) * F(0.5) + F(15.0)
    assert register(rxr, ctx, gen) == RXR_OK
    rec = G.compare("three roads", heights(rxr, ctx, pts), gen.sample(pts), min_class_share=None)
    assert rec["pow"] >= 32


def test_nan_and_infinite_records_and_points(dev):
    rxr, ctx = dev
    gen, pts = G.special_scene()
    assert register(rxr, ctx, gen) == RXR_OK
    ref = gen.sample(pts)
    assert 3 <= np.isnan(ref[0]).sum() <= len(pts) - 6 and np.isinf(ref[0]).any()
    G.compare("special", heights(rxr, ctx, pts), ref, min_class_share=None)
    heights(rxr, ctx, pts, normals=True)   # (runs; NaN normals are NaNs)


@pytest.mark.parametrize("subdivisions", [1, 2, 3])
def test_grids(dev, sampled, subdivisions):
    rxr, ctx = dev
    gen = sampled["hills_ridges_roads"][0]
    gen = Generator(**{**gen.args(), "subdivisions": subdivisions})
    assert register(rxr, ctx, gen) == RXR_OK
    # negative and fractional coordinates, two boxes of different counts in one call, an empty grid, a single point
    boxes = [(-3.5, -2.25, 1.25, 0.5), (20.0, 28.5, 27.0, 31.0), (5.0, 5.0, 3.0, 3.0), (40.0, 40.0, 40.0, 40.0)]
    want = [gen.generate_grid(b) for b in boxes]
    stride = max(s[0] * s[1] for s, _ in want) + 5
    counts, h = grids(rxr, ctx, boxes, subdivisions, stride)
    for i, ((sx, sy), pts) in enumerate(want):
        assert tuple(counts[i]) == (max(sx, 0), max(sy, 0)), (i, counts[i], sx, sy)
        k = len(pts)
        assert (h[i, k:] == SENTINEL).all()   # slots past the count are not written
        if k:
            G.compare(f"box {i}", h[i, :k], gen.sample(pts), min_class_share=None)
            # ... and the points are the reference's: the same heights as a call on the transcription's grid points
            assert np.array_equal(h[i, :k].view(np.uint32), heights(rxr, ctx, pts).view(np.uint32))
    assert len(want[0][1]) != len(want[1][1]) and len(want[2][1]) == 0 and len(want[3][1]) == 1


def test_a_box_refused_for_its_stride_queues_nothing(dev, sampled):
    rxr, ctx = dev
    assert register(rxr, ctx, sampled["hills_ridges_roads"][0]) == RXR_OK
    boxes = [(0, 0, 2, 2), (0, 0, 3, 3)]   # 9 and 16 points
    counts, h = grids(rxr, ctx, boxes, 1, 15, expect=RXR_ERR_INVALID)
    assert "box 1" in last_error(rxr, ctx) and (h == SENTINEL).all() and (counts == 0xABCD).all()
    counts, h = grids(rxr, ctx, boxes, 1, 16)
    assert counts.tolist() == [[3, 3], [4, 4]] and (h[0, 9:] == SENTINEL).all() and (h[1] != SENTINEL).all()
    assert grids(rxr, ctx, boxes, 0, 16, expect=RXR_ERR_INVALID) is not None and "subdivisions" in last_error(rxr, ctx)
    assert rxr.rxr_generated_grids(ctx, None, 0, 1, 16, None, None) == RXR_OK
    # an extent whose `as i32` saturates wraps to a negative step with the + 1: an empty grid, as the mirror and the reference have it
    counts, h = grids(rxr, ctx, [(0, 0, INF, 1), (0, 0, 1, 1), (0, 0, 1, 3e9)], 1, 16)
    assert counts.tolist() == [[0, 2], [2, 2], [2, 0]] and (h[0] == SENTINEL).all() and (h[2] == SENTINEL).all() and (h[1, :4] != SENTINEL).all()


def test_to_forms_on_a_second_stream_next_to_a_queued_frame(dev, product, sampled):
    import torch

    from rusterix_amd import scenes

    rxr, ctx = dev
    gen, pts, ref = sampled["hills_ridges_roads"]
    cfg = scenes.map_scene(product, width=320, height=192, logo_size=128, n_lights=4)
    frame = scenes.render(cfg).copy()
    r = cfg.setup()
    assert product.lib.rxh_rasterizer_upload(r._h, cfg.scene._h, cfg.width, cfg.height, cfg.tile_size, cfg.assets._h) == 0
    assert register(rxr, ctx, gen) == RXR_OK
    n = len(pts)
    stream = torch.cuda.Stream()
    sp = C.c_void_p(stream.cuda_stream)
    dp = torch.from_numpy(pts).cuda()
    dh = torch.full((n + GUARD,), float(SENTINEL), device="cuda")
    dn = torch.full((3 * n + GUARD,), float(SENTINEL), device="cuda")
    boxes = np.array([(20.0, 28.5, 27.0, 31.0), (-3.5, -2.25, 1.25, 0.5)], F)
    stride = 64
    dc = torch.full((4 + GUARD,), 0xABCD, dtype=torch.int32, device="cuda")
    dg = torch.full((2 * stride + GUARD,), float(SENTINEL), device="cuda")
    torch.cuda.synchronize()
    assert rxr.rxr_render_rows(ctx, 0, cfg.height) == RXR_OK, last_error(rxr, ctx)   # a frame queued on the context's stream
    assert rxr.rxr_generated_heights_to(ctx, dp.data_ptr(), n, dh.data_ptr(), dn.data_ptr(), sp) == RXR_OK, last_error(rxr, ctx)
    assert rxr.rxr_generated_grids_to(ctx, boxes.ctypes.data, 2, 1, stride, dc.data_ptr(), dg.data_ptr(), sp) == RXR_OK, last_error(rxr, ctx)
    # re-registration behind queued evaluations waits for them: the answers above are the first generator's
    other = G.scene(seed=5)
    assert register(rxr, ctx, other) == RXR_OK
    stream.synchronize()
    h, nr = dh.cpu().numpy(), dn.cpu().numpy()
    assert (h[n:] == SENTINEL).all() and (nr[3 * n:] == SENTINEL).all()
    G.compare("_to", h[:n], ref)
    blocking = heights(rxr, ctx, pts)
    G.compare("re-registered", blocking, other.sample(pts), min_class_share=None)
    assert register(rxr, ctx, gen) == RXR_OK
    hb, nb = heights(rxr, ctx, pts, normals=True)
    assert np.array_equal(hb.view(np.uint32), h[:n].view(np.uint32)) and np.array_equal(nb.view(np.uint32), nr[:3 * n].reshape(n, 3).view(np.uint32))
    counts, g = dc.cpu().numpy().view(np.uint32), dg.cpu().numpy()
    bc, bg = grids(rxr, ctx, boxes, 1, stride)
    assert np.array_equal(counts[:4].reshape(2, 2), bc) and (counts[4:] == 0xABCD).all()
    assert np.array_equal(g[:2 * stride].view(np.uint32), bg.reshape(-1).view(np.uint32)) and (g[2 * stride:] == SENTINEL).all()
    # the frame is the frame
    got = np.zeros_like(frame)
    assert rxr.rxr_render_download(ctx, got.ctypes.data) == RXR_OK, last_error(rxr, ctx)
    assert np.array_equal(got, frame)
    # host memory where device memory is expected, a misaligned pointer, NULL, n == 0
    assert rxr.rxr_generated_heights_to(ctx, pts.ctypes.data, n, dh.data_ptr(), None, sp) == RXR_ERR_INVALID and "dev_points" in last_error(rxr, ctx)
    assert rxr.rxr_generated_heights_to(ctx, dp.data_ptr(), n, dh.data_ptr() + 2, None, sp) == RXR_ERR_INVALID and "dev_heights" in last_error(rxr, ctx)
    assert rxr.rxr_generated_heights_to(ctx, dp.data_ptr(), n, None, None, sp) == RXR_ERR_INVALID
    assert rxr.rxr_generated_heights_to(ctx, None, 0, None, None, sp) == RXR_OK
    assert rxr.rxr_generated_heights(ctx, None, 0, None, None) == RXR_OK
    host_counts = np.zeros(4, np.uint32)
    assert rxr.rxr_generated_grids_to(ctx, boxes.ctypes.data, 2, 1, stride, host_counts.ctypes.data, dg.data_ptr(), sp) == RXR_ERR_INVALID
    assert rxr.rxr_synchronize(ctx) == RXR_OK


def test_registration_lifetime_on_a_context_of_its_own(product, sampled):
    rxr = rusterix_amd.rxr_abi()
    ctx = C.c_void_p()
    assert rxr.rxr_create(C.byref(ctx), 0) == RXR_OK
    try:
        gen, pts, ref = sampled["many_roads"]
        out = np.zeros(4, F)
        assert rxr.rxr_generated_heights(ctx, pts.ctypes.data, 4, out.ctypes.data, None) == RXR_ERR_INVALID and "no terrain generator" in last_error(rxr, ctx)
        assert rxr.rxr_generated_grids(ctx, pts.ctypes.data, 1, 1, 4, out.ctypes.data, out.ctypes.data) == RXR_ERR_INVALID
        assert register(rxr, ctx, gen) == RXR_OK, last_error(rxr, ctx)
        G.compare("first", heights(rxr, ctx, pts), ref)
        # a refused call leaves the old answers: offsets that do not end at the edge count, a count above its cap
        a = gen.args()
        assert register(rxr, ctx, Generator(**{**a, "ridge_edge_offsets": a["ridge_edge_offsets"] + 1})) == RXR_ERR_INVALID
        assert "ridge_edge_offsets" in last_error(rxr, ctx)
        z = np.zeros(4, F)
        assert rxr.rxr_set_terrain_generator(ctx, z.ctypes.data, (1 << 16) + 1, None, 0, None, None, 0, None, 0, z.ctypes.data) == RXR_ERR_UNSUPPORTED
        G.compare("after refused calls", heights(rxr, ctx, pts), ref)
        # every count 0: the field is 0.0 everywhere
        assert register(rxr, ctx, Generator()) == RXR_OK
        assert (heights(rxr, ctx, pts).view(np.uint32) == 0).all()
        # independent of the terrain heights: none are resident here, and a pick still says so
        hit = np.zeros(1, np.uint32)
        assert rxr.rxr_terrain_hits(ctx, z.ctypes.data, z.ctypes.data, 1, 1.0, hit.ctypes.data, None, None, None) == RXR_ERR_INVALID
    finally:
        rxr.rxr_destroy(ctx)


def test_multi_device_handles(product, sampled):
    rxr = rusterix_amd.rxr_abi()
    multi = C.c_void_p()
    devs = (C.c_int * 2)(0, 0)
    assert rxr.rxr_create_multi(C.byref(multi), devs, 2) == RXR_OK
    try:
        gen, pts, ref = sampled["hills_ridges_roads"]
        out = np.zeros(len(pts), F)
        assert rxr.rxr_generated_heights(multi, pts.ctypes.data, 4, out.ctypes.data, None) == RXR_ERR_INVALID and "no terrain generator" in last_error(rxr, multi)
        assert register(rxr, multi, gen) == RXR_OK, last_error(rxr, multi)
        assert rxr.rxr_generated_heights_to(multi, pts.ctypes.data, 4, out.ctypes.data, None, None) == RXR_ERR_UNSUPPORTED and "multi-device" in last_error(rxr, multi)
        assert rxr.rxr_generated_grids_to(multi, pts.ctypes.data, 1, 1, 4, out.ctypes.data, out.ctypes.data, None) == RXR_ERR_UNSUPPORTED
        G.compare("member 0", heights(rxr, multi, pts), ref)
        counts, h = grids(rxr, multi, [(20.0, 28.5, 27.0, 31.0)], 1, 40)
        assert counts.tolist() == [[8, 4]] and rxr.rxr_debug_terrain_gen_launches(multi) == 1
    finally:
        rxr.rxr_destroy(multi)


def test_the_mirror_registers_its_lists_when_they_changed(product, sampled):
    gen, pts, ref = sampled["hills_ridges_roads"]
    mirror = product.TerrainGenerator(**gen.args())
    G.compare("mirror", mirror.sample_heights(pts), ref)
    h, nr = mirror.sample_normals(pts[:70])
    assert np.array_equal(h.view(np.uint32), mirror.sample_heights(pts[:70]).view(np.uint32)) and nr.shape == (70, 3)
    other = G.scene(seed=5)
    mirror.set(**{k: v for k, v in other.args().items() if k != "subdivisions"})
    G.compare("mirror, other lists", mirror.sample_heights(pts), other.sample(pts), min_class_share=None)
    boxes = [(20.0, 28.5, 27.0, 31.0), (-3.5, -2.25, 1.25, 0.5)]
    counts, g = mirror.grid_heights(boxes, 48, fill=float(SENTINEL))
    ccounts, cg = mirror.grid_heights_cpu(boxes, 48, fill=float(SENTINEL))
    assert np.array_equal(counts, ccounts) and counts.tolist() == [[8, 4], [7, 5]]
    for i in range(2):
        k = int(counts[i, 0] * counts[i, 1])
        G.compare(f"mirror grid {i}", g[i, :k], other.sample(other.generate_grid(boxes[i])[1]), min_class_share=None)
        assert (g[i, k:] == SENTINEL).all() and (cg[i, k:] == SENTINEL).all()
    with pytest.raises(Exception):
        mirror.grid_heights(boxes, 30)
    wrapped = [(0, 0, INF, 1), (0, 0, 1, 1)]
    assert mirror.grid_heights(wrapped, 4)[0].tolist() == mirror.grid_heights_cpu(wrapped, 4)[0].tolist() == [[0, 2], [2, 2]]
