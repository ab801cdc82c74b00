"""The terrain pick on the device (rxr_set_terrain_heights / rxr_terrain_hits / rxr_terrain_hits_to, Terrain::ray_terrain_hit) against
the numpy restatement of tests/terrain_hit_ref.py: every output array equal bit for bit, no tolerance (a NaN, which only world_pos
can hold, must be a NaN: its sign and payload are the hardware's, tests/terrain_hit_ref.py `bits`).  Both march kernels (one ray
per lane, one ray per wave) are forced through RXR_TERRAIN_HIT_ROUTE and proven to have run by name.  Shapes are the smallest at
which each can go wrong: steps on both sides of the per-wave kernel's rounds of 64 (63 / 64 / 65, 127 / 128, the last step, a miss
after all 1500), a wave whose lanes leave at 64 different steps, ray counts that are no multiple of the workgroup, launches split
down to one ray."""
import ctypes as C

import numpy as np
import pytest

import rusterix_amd
from rusterix_amd import binding as B
from rusterix_amd import scenes
from tests import terrain_hit_ref as H
from tests.terrain_hit_ref import F, TK, HeightSpec, RXR_ERR_INVALID, RXR_ERR_UNSUPPORTED, RXR_OK

pytestmark = pytest.mark.gpu

NAN = float("nan")
ROUTES = {"lane": "k_terrain_hit_lane", "wave": "k_terrain_hit_wave"}


def context_of(product):
    return C.c_void_p(product.lib.rxh_context())


def last_error(rxr, ctx):
    return (rxr.rxr_last_error(ctx) or b"").decode()


def set_heights(rxr, ctx, spec):
    keep, args = spec.arrays()
    return rxr.rxr_set_terrain_heights(ctx, *args)


def hits(rxr, ctx, origins, dirs, max_distance, only_hit=False):
    o = np.ascontiguousarray(np.asarray(origins, F).reshape(-1, 3))
    d = np.ascontiguousarray(np.asarray(dirs, F).reshape(-1, 3))
    n = len(o)
    out = dict(hit=np.full(n, 7, np.uint32), t=np.full(n, 7, F), world_pos=np.full((n, 3), 7, F), grid_pos=np.full((n, 2), 7, np.int32))
    opt = [None] * 3 if only_hit else [out[k].ctypes.data for k in ("t", "world_pos", "grid_pos")]
    rc = rxr.rxr_terrain_hits(ctx, o.ctypes.data, d.ctypes.data, n, max_distance, out["hit"].ctypes.data, *opt)
    assert rc == RXR_OK, last_error(rxr, ctx)
    return out


def kernel_of(rxr, ctx):
    launches = C.c_uint32(0)
    name = rxr.rxr_debug_terrain_hit_kernel(ctx, C.byref(launches))
    return (name or b"").decode(), launches.value


def expect(got, want, label=""):
    assert not H.first_difference(got, want), f"{label}: {H.first_difference(got, want)}"


@pytest.fixture()
def dev(product):
    """the library, the mirror's context and a function that registers a HeightSpec there"""
    rxr, ctx = rusterix_amd.rxr_abi(), context_of(product)

    def register(spec):
        assert set_heights(rxr, ctx, spec) == RXR_OK, last_error(rxr, ctx)
        # (the mirror does not know: its next Terrain registers its own heights again, by generation stamp)
        return spec

    return rxr, ctx, register


@pytest.fixture(params=sorted(ROUTES))
def route(request, monkeypatch):
    monkeypatch.setenv("RXR_TERRAIN_HIT_ROUTE", request.param)
    return request.param


def run(dev, route, spec, o, d, md, label=""):
    """one forced-route call against the reference; returns the reference's answers"""
    rxr, ctx, register = dev
    register(spec)
    want = spec.hits(o, d, md)
    expect(hits(rxr, ctx, o, d, md), want, f"{route} {label}")
    assert kernel_of(rxr, ctx)[0] == ROUTES[route]
    return want


# ---- per route -------------------------------------------------------------------------------------------------------------------------
def test_vertical_rays_at_the_round_boundaries(dev, route):
    o, d = H.vertical_rays()
    want = run(dev, route, HeightSpec(), o, d, NAN)
    assert want["step"].tolist() == H.VERTICAL_STEPS
    beyond = F(TK[1499] + F(0.1))
    o2 = np.concatenate([o, np.array([[0.2, beyond + F(0.005), 0.2]], F)])            # ... and a miss after all 1500 steps
    d2 = np.concatenate([d, d[:1]])
    assert run(dev, route, HeightSpec(), o2, d2, NAN)["step"].tolist() == H.VERTICAL_STEPS + [-1]
    assert run(dev, route, HeightSpec(), o2, d2, 100.0)["step"].tolist() == H.VERTICAL_STEPS[:-1] + [-1, -1]
    # every single step, one ray each
    o3, d3 = H.vertical_rays(list(range(0, 1500, 7)) + [1498, 1499])
    assert (run(dev, route, HeightSpec(), o3, d3, NAN)["step"] >= 0).all()


def test_a_horizontal_ray_over_two_walls_takes_the_lowest_step(dev, route):
    o = np.array([[0, 2, 0], [-10, 2, 0], [0, 6, 0], [-3.3, 2, 0], [-9.9, 2, 1]], F)
    d = np.array([[1, 0, 0]] * 5, F)
    want = run(dev, route, H.walls_spec(), o, d, NAN)
    # ray 0: steps 26-35 and 66-75 hold (one round, and a later one); ray 1: 125-134 hold, across the rounds' boundary at 128
    assert want["step"][:3].tolist() == [26, 125, -1]


def test_nan_and_infinite_components(dev, route):
    spec = HeightSpec().height(0, 0, 5.0).height(0, 1, 7.0)
    inf = float("inf")
    o = np.array([[0, NAN, 0], [0, 1, 0], [0, 1, 0], [NAN, 6, 1], [3, 6, NAN], [0, 1, 0], [0, 1, 0], [inf, 1, 0], [0, -inf, 0], [0, inf, 0], [-inf, -inf, inf]], F)
    d = np.array([[0, -1, 0], [0, NAN, 0], [NAN, 0, 0], [0, 0, 0], [0, 0, 0], [inf, -1, 0], [0, -inf, 0], [0, -1, 0], [0, 1, 0], [0, -1, 0], [1, 1, 1]], F)
    want = run(dev, route, spec, o, d, 2.0)
    assert want["hit"][:10].tolist() == [0, 0, 1, 1, 0, 1, 1, 1, 1, 0]


@pytest.mark.parametrize("md", [-1.0, 0.0, 1.0, 100.0, NAN])
def test_max_distance(dev, route, md):
    o, d = H.vertical_rays([0, 1, 9, 10, 11, 1000, 1001, 1499])
    want = run(dev, route, HeightSpec(), o, d, md, f"max_distance {md}")
    k = H.steps_tested(md)
    assert want["step"].tolist() == [s if s < k else -1 for s in [0, 1, 9, 10, 11, 1000, 1001, 1499]]


@pytest.mark.parametrize("corner", [(2 ** 30 - 2, 2 ** 30 - 2), (-2 ** 30, -2 ** 30), (2 ** 30 - 2, -2 ** 30)])
def test_a_height_grid_at_the_coordinate_bound(dev, route, corner):
    """a 3 x 3 grid whose far corner is +-2^30: f32 is 64 (below 2^30) or 128 apart there, rays land on few cells and the bilinear
    neighbours x0 + 1 leave the grid"""
    cx, cy = corner
    spec = HeightSpec()
    rng = np.random.default_rng(3)
    for y in range(3):
        for x in range(3):
            spec.height(cx + x, cy + y, rng.uniform(1.0, 4.0))
    n = 96
    o = np.stack([F(cx) + rng.uniform(-200, 200, n), rng.uniform(0.5, 6, n), F(cy) + rng.uniform(-200, 200, n)], axis=1).astype(F)
    o[: n // 2, 0], o[: n // 2, 2] = F(cx), F(cy)                      # half of them right over the corner cell
    d = np.stack([rng.choice([-64.0, 0.0, 64.0, 640.0], n), rng.uniform(-1, 0.2, n), rng.choice([-64.0, 0.0, 64.0, 640.0], n)], axis=1).astype(F)
    want = run(dev, route, spec, o, d, 50.0, f"corner {corner}")
    assert 0 < want["hit"].sum() < n
    # i32::MAX itself: floor saturates, x0 + 1 wraps, the height is 0 either way
    o2 = np.array([[3.0e9, 1, 0], [-3.0e9, 1, 3.0e9], [2147483520.0, 1, -2147483648.0]], F)
    d2 = np.array([[0, -1, 0], [0, -1, 0], [128, -1, -256]], F)
    assert run(dev, route, spec, o2, d2, 5.0)["hit"].all()


def test_a_scale_other_than_one(dev, route):
    spec = H.fuzz_spec(2, (0.75, 1.5))
    o, d, _ = H.fuzz_rays(2, 300)
    want = run(dev, route, spec, o, d, 30.0)
    same = H.fuzz_spec(2).hits(o, d, 30.0)
    assert np.array_equal(want["world_pos"], same["world_pos"]) and not np.array_equal(want["grid_pos"], same["grid_pos"])


@pytest.mark.parametrize("seed", range(6))
def test_fuzz(dev, route, seed):
    spec, o, d, md, want = H.fuzz_case(seed)
    rxr, ctx, register = dev
    register(spec)
    expect(hits(rxr, ctx, o, d, md), want, f"{route} seed {seed} (max_distance {md})")
    assert kernel_of(rxr, ctx)[0] == ROUTES[route]
    if md != 1.0:
        assert 0.2 <= float(want["hit"].mean()) <= 0.8


def test_optional_arrays_may_be_null(dev, route):
    rxr, ctx, register = dev
    spec, o, d, md, want = H.fuzz_case(1)
    register(spec)
    got = hits(rxr, ctx, o[:130], d[:130], md, only_hit=True)
    assert np.array_equal(got["hit"], want["hit"][:130]) and (got["t"] == 7).all() and (got["grid_pos"] == 7).all()


# ---- default routing ---------------------------------------------------------------------------------------------------------------------
def test_the_threshold_picks_the_kernel(dev, monkeypatch):
    monkeypatch.delenv("RXR_TERRAIN_HIT_ROUTE", raising=False)
    rxr, ctx, register = dev
    few = rxr.rxr_debug_terrain_hit_few_rays()
    assert 1 <= few < 1 << 20
    spec, o, d, md, want = H.fuzz_case(3)
    register(spec)
    sizes = sorted({1, few, few + 1, 257, 1000})
    m = max(sizes)
    reps = -(-m // len(o))
    oo, dd = np.tile(o, (reps, 1))[:m], np.tile(d, (reps, 1))[:m]
    ww = {k: np.tile(want[k], (reps,) + (1,) * (want[k].ndim - 1))[:m] for k in H.KEYS}
    for n in sizes:
        got = hits(rxr, ctx, oo[:n], dd[:n], md)
        expect(got, {k: ww[k][:n] for k in H.KEYS}, f"{n} rays")
        assert kernel_of(rxr, ctx) == (ROUTES["wave" if n <= few else "lane"], 1), n
    monkeypatch.setenv("RXR_TERRAIN_HIT_ROUTE", "sideways")
    out = np.zeros(1, np.uint32)
    assert rxr.rxr_terrain_hits(ctx, oo.ctypes.data, dd.ctypes.data, 1, md, out.ctypes.data, None, None, None) == RXR_ERR_INVALID
    assert "RXR_TERRAIN_HIT_ROUTE" in last_error(rxr, ctx)


# ---- the per-lane kernel under divergence --------------------------------------------------------------------------------------------------
def test_one_wave_whose_lanes_leave_at_64_different_steps(dev, monkeypatch):
    monkeypatch.setenv("RXR_TERRAIN_HIT_ROUTE", "lane")
    rng = np.random.default_rng(8)
    steps = rng.permutation(64)
    o, d = H.vertical_rays(steps.tolist())
    miss = rng.random(64) < 0.25
    d[miss] = [0.0, 1.0, 0.0]                       # upwards: never a hit (except from step 0's height)
    o[miss, 1] = 5.0
    want = run(dev, "lane", HeightSpec(), o, d, NAN)
    assert want["step"].tolist() == [-1 if m else int(s) for s, m in zip(steps, miss)] and 5 < miss.sum() < 30


def test_1000_rays_are_no_multiple_of_the_workgroup(dev, monkeypatch):
    monkeypatch.setenv("RXR_TERRAIN_HIT_ROUTE", "lane")
    spec, o, d, md, want = H.fuzz_case(2)
    rxr, ctx, register = dev
    register(spec)
    for n in (1000, 255, 1):
        expect(hits(rxr, ctx, o[:n], d[:n], md), {k: want[k][:n] for k in H.KEYS}, f"{n} rays")


# ---- launch splitting ------------------------------------------------------------------------------------------------------------------------
def test_launch_splitting(dev, route, monkeypatch):
    rxr, ctx, register = dev
    spec, o, d, md, want = H.fuzz_case(1)
    register(spec)
    n = 700
    whole = hits(rxr, ctx, o[:n], d[:n], md)
    assert kernel_of(rxr, ctx) == (ROUTES[route], 1)
    expect(whole, {k: want[k][:n] for k in H.KEYS})
    monkeypatch.setenv("RXR_TERRAIN_HIT_LAUNCH_RAYS", "256")
    expect(hits(rxr, ctx, o[:n], d[:n], md), whole, "256 rays a launch")
    assert kernel_of(rxr, ctx) == (ROUTES[route], 3)
    monkeypatch.setenv("RXR_TERRAIN_HIT_LAUNCH_RAYS", "1")
    expect(hits(rxr, ctx, o[:70], d[:70], md), {k: whole[k][:70] for k in H.KEYS}, "one ray a launch")
    assert kernel_of(rxr, ctx) == (ROUTES[route], 70)
    monkeypatch.delenv("RXR_TERRAIN_HIT_LAUNCH_RAYS")
    expect(hits(rxr, ctx, o[:n], d[:n], md), whole)
    assert kernel_of(rxr, ctx)[1] == 1


# ---- through the mirror -------------------------------------------------------------------------------------------------------------------
def test_the_mirror_registers_its_heights_when_they_changed(product):
    spec, o, d, md, want = H.fuzz_case(0)
    t = spec.product(product)
    expect(t.ray_terrain_hits(o, d, md), want, "first")
    other = H.fuzz_spec(4).product(product)
    expect(other.ray_terrain_hits(o, d, md), H.fuzz_spec(4).hits(o, d, md), "another terrain")
    expect(t.ray_terrain_hits(o, d, md), want, "back")
    t.set_height(0, 0, 9.0)                                       # an edit: registered again by the generation stamp
    spec2 = H.fuzz_spec(0).height(0, 0, 9.0)
    want2 = spec2.hits(o, d, md)
    assert H.first_difference(want2, want)
    expect(t.ray_terrain_hits(o, d, md), want2, "after set_height")
    empty = product.Terrain().ray_terrain_hits(o[:5], d[:5], md)
    expect(empty, HeightSpec().hits(o[:5], d[:5], md), "no heights at all")
    assert len(t.ray_terrain_hits(np.zeros((0, 3), F), np.zeros((0, 3), F), md)["hit"]) == 0


# ---- stream and lifetime -------------------------------------------------------------------------------------------------------------------
def test_to_form_on_another_stream_equals_the_blocking_call(dev, monkeypatch):
    import torch

    monkeypatch.delenv("RXR_TERRAIN_HIT_ROUTE", raising=False)
    rxr, ctx, register = dev
    spec, o, d, md, want = H.fuzz_case(3)
    register(spec)
    n = len(o)
    expect(hits(rxr, ctx, o, d, md), want, "blocking")
    stream = torch.cuda.Stream()
    do, dd = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    hit = torch.zeros(n, dtype=torch.int32, device="cuda")
    t = torch.zeros(n, dtype=torch.float32, device="cuda")
    wp = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
    gp = torch.zeros((n, 2), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    sp = C.c_void_p(stream.cuda_stream)
    args = (do.data_ptr(), dd.data_ptr(), n, md, hit.data_ptr(), t.data_ptr(), wp.data_ptr(), gp.data_ptr())
    assert rxr.rxr_terrain_hits_to(ctx, *args, sp) == RXR_OK, last_error(rxr, ctx)
    assert rxr.rxr_synchronize(ctx) == RXR_OK, last_error(rxr, ctx)
    stream.synchronize()
    got = dict(hit=hit.cpu().numpy().view(np.uint32), t=t.cpu().numpy(), world_pos=wp.cpu().numpy(), grid_pos=gp.cpu().numpy())
    expect(got, want, "_to")
    # only `hit`; host memory where device memory is expected, a misaligned pointer, NULL
    hit.zero_()
    assert rxr.rxr_terrain_hits_to(ctx, do.data_ptr(), dd.data_ptr(), n, md, hit.data_ptr(), None, None, None, sp) == RXR_OK
    stream.synchronize()
    assert np.array_equal(hit.cpu().numpy().view(np.uint32), want["hit"])
    assert rxr.rxr_terrain_hits_to(ctx, o.ctypes.data, *args[1:], sp) == RXR_ERR_INVALID and "device memory" in last_error(rxr, ctx)
    assert rxr.rxr_terrain_hits_to(ctx, *args[:5], t.data_ptr() + 2, *args[6:], sp) == RXR_ERR_INVALID and "dev_t" in last_error(rxr, ctx)
    host_wp = np.zeros((n, 3), F)
    assert rxr.rxr_terrain_hits_to(ctx, *args[:6], host_wp.ctypes.data, args[7], sp) == RXR_ERR_INVALID and "dev_world_pos" in last_error(rxr, ctx)
    assert rxr.rxr_terrain_hits_to(ctx, *args[:4], None, *args[5:], sp) == RXR_ERR_INVALID
    assert rxr.rxr_terrain_hits_to(ctx, None, *args[1:], sp) == RXR_ERR_INVALID
    assert rxr.rxr_terrain_hits_to(ctx, None, None, 0, md, None, None, None, None, sp) == RXR_OK
    assert rxr.rxr_terrain_hits(ctx, None, None, 0, md, None, None, None, None) == RXR_OK
    assert rxr.rxr_terrain_hits(ctx, o.ctypes.data, d.ctypes.data, 1, md, None, None, None, None) == RXR_ERR_INVALID
    assert rxr.rxr_synchronize(ctx) == RXR_OK
    expect(hits(rxr, ctx, o, d, md), want, "afterwards")


def test_screen_rays_go_straight_in(dev, product, monkeypatch):
    """rxr_screen_rays_to at 64 x 48 feeds rxr_terrain_hits_to on the same stream: a picking buffer without a host round trip"""
    import torch

    monkeypatch.delenv("RXR_TERRAIN_HIT_ROUTE", raising=False)
    rxr, ctx, register = dev
    spec = register(H.fuzz_spec(5))
    w, h = 64, 48
    cam = product.D3OrbitCamera.new()
    cam.set_parameter_f32("distance", 14.0)
    cam.center = (0.0, 0.0, 0.0)
    cam.azimuth, cam.elevation = 0.9, 0.7
    view, proj = cam.matrices(float(w), float(h))
    iv, ip, _ = product.Rasterizer.setup(None, view, proj).derived()
    n = w * h
    do, dd = torch.zeros((n, 3), device="cuda"), torch.zeros((n, 3), device="cuda")
    hit = torch.zeros(n, dtype=torch.int32, device="cuda")
    t, wp = torch.zeros(n, device="cuda"), torch.zeros((n, 3), device="cuda")
    gp = torch.zeros((n, 2), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    sp = C.c_void_p(stream.cuda_stream)
    assert rxr.rxr_screen_rays_to(ctx, iv.ctypes.data, ip.ctypes.data, float(w), float(h), 0, 0, w, h, do.data_ptr(), dd.data_ptr(), sp) == RXR_OK, last_error(rxr, ctx)
    assert rxr.rxr_terrain_hits_to(ctx, do.data_ptr(), dd.data_ptr(), n, 60.0, hit.data_ptr(), t.data_ptr(), wp.data_ptr(), gp.data_ptr(), sp) == RXR_OK, last_error(rxr, ctx)
    stream.synchronize()
    o, d = do.cpu().numpy(), dd.cpu().numpy()
    want = spec.hits(o, d, 60.0)
    got = dict(hit=hit.cpu().numpy().view(np.uint32), t=t.cpu().numpy(), world_pos=wp.cpu().numpy(), grid_pos=gp.cpu().numpy())
    expect(got, want, "screen rays")
    assert 0.2 < want["hit"].mean() <= 1.0 and len(np.unique(want["grid_pos"], axis=0)) > 30
    assert kernel_of(rxr, ctx) == (ROUTES["wave" if n <= rxr.rxr_debug_terrain_hit_few_rays() else "lane"], 1)


def test_re_registration_and_removal(product):
    rxr = rusterix_amd.rxr_abi()
    ctx = C.c_void_p()
    assert rxr.rxr_create(C.byref(ctx), 0) == RXR_OK
    try:
        _, o, d, md, _ = H.fuzz_case(2)
        o, d = o[:300], d[:300]
        out = np.zeros(300, np.uint32)
        assert rxr.rxr_terrain_hits(ctx, o.ctypes.data, d.ctypes.data, 300, md, out.ctypes.data, None, None, None) == RXR_ERR_INVALID
        assert "no terrain heights" in last_error(rxr, ctx)
        assert rxr.rxr_terrain_hits_to(ctx, o.ctypes.data, d.ctypes.data, 300, md, out.ctypes.data, None, None, None, None) == RXR_ERR_INVALID
        first, second = H.fuzz_spec(2), H.fuzz_spec(3, (0.5, 2.0))
        assert set_heights(rxr, ctx, first) == RXR_OK, last_error(rxr, ctx)
        expect(hits(rxr, ctx, o, d, md), first.hits(o, d, md), "first")
        assert set_heights(rxr, ctx, second) == RXR_OK, last_error(rxr, ctx)
        expect(hits(rxr, ctx, o, d, md), second.hits(o, d, md), "second")
        # a refused call leaves the resident heights as they were
        assert set_heights(rxr, ctx, HeightSpec((0.0, 1.0)).height(0, 0, 1)) == RXR_ERR_INVALID and "scale" in last_error(rxr, ctx)
        assert set_heights(rxr, ctx, HeightSpec().height(2 ** 30 + 1, 0, 1)) == RXR_ERR_INVALID and "2^30" in last_error(rxr, ctx)
        expect(hits(rxr, ctx, o, d, md), second.hits(o, d, md), "after refused calls")
        # n_cells == 0: the plane at 0, with the new scale
        empty = HeightSpec((2.0, 0.5))
        assert set_heights(rxr, ctx, empty) == RXR_OK
        got = hits(rxr, ctx, o, d, md)
        expect(got, empty.hits(o, d, md), "empty")
        assert (got["world_pos"][:, 1] == 0).all() and got["hit"].any()
        # a coordinate given twice: the later entry wins
        keep, args = first.arrays()
        xy, hh = np.concatenate([keep["xy"], keep["xy"][:1]]), np.concatenate([keep["h"], np.array([9.0], F)])
        assert rxr.rxr_set_terrain_heights(ctx, args[0], xy.ctypes.data, hh.ctypes.data, len(hh)) == RXR_OK, last_error(rxr, ctx)
        x, y = (int(v) for v in keep["xy"][0])
        first.height(x, y, 9.0)
        oo = np.array([[x, 9.5, y], [x + 0.4, 12, y - 0.4]], F)
        dd = np.array([[0, -1, 0], [0.01, -1, 0.01]], F)
        expect(hits(rxr, ctx, oo, dd, md), first.hits(oo, dd, md), "later entry")
        assert first.hits(oo, dd, md)["world_pos"][0, 1] == 9.0
        # independent of rxr_set_terrain: no terrain is resident here, and a bake still says so
        zero = np.zeros((1, 2), np.int32)
        px = np.zeros((4, 4, 4), np.uint8)
        assert rxr.rxr_bake_terrain(ctx, zero.ctypes.data, 1, 1, px.ctypes.data) == RXR_ERR_INVALID and "no terrain is resident" in last_error(rxr, ctx)
    finally:
        rxr.rxr_destroy(ctx)


def test_multi_device_handles(product):
    rxr = rusterix_amd.rxr_abi()
    multi = C.c_void_p()
    devs = (C.c_int * 2)(0, 0)
    assert rxr.rxr_create_multi(C.byref(multi), devs, 2) == RXR_OK
    try:
        o, d = H.vertical_rays([0, 5, 70])
        out = np.zeros(3, np.uint32)
        assert rxr.rxr_terrain_hits(multi, o.ctypes.data, d.ctypes.data, 3, NAN, out.ctypes.data, None, None, None) == RXR_ERR_INVALID
        assert "no terrain heights" in last_error(rxr, multi)
        spec = HeightSpec().height(0, 0, 0.25)
        assert set_heights(rxr, multi, spec) == RXR_OK, last_error(rxr, multi)
        assert rxr.rxr_terrain_hits_to(multi, o.ctypes.data, d.ctypes.data, 3, NAN, out.ctypes.data, None, None, None, None) == RXR_ERR_UNSUPPORTED
        assert "multi-device" in last_error(rxr, multi)
        expect(hits(rxr, multi, o, d, NAN), spec.hits(o, d, NAN), "member 0")
        assert kernel_of(rxr, multi) == (ROUTES["wave"], 1)
    finally:
        rxr.rxr_destroy(multi)


def test_a_frame_renders_the_same_after_a_pick(product):
    from tests.test_gpu_terrain import H as FH, W as FW, terrain_frame
    from tests import terrain_ref as R

    tex = R.uniform_scene(R.RADIUS, 1, chunk_size=8, seed=9).bake((0, 0), 8)
    given = B.Texture(tex.reshape(-1).copy(), 64, 64)
    cfg = terrain_frame(product, given, (0, 0), 8)
    ref_frame = scenes.render(cfg).copy()
    assert len(np.unique(ref_frame.reshape(-1, 4), axis=0)) > 100
    lib, rxr = product.lib, rusterix_amd.rxr_abi()
    r = cfg.setup()
    assert lib.rxh_rasterizer_upload(r._h, cfg.scene._h, cfg.width, cfg.height, cfg.tile_size, cfg.assets._h) == 0
    spec, o, d, md, want = H.fuzz_case(1)
    expect(spec.product(product).ray_terrain_hits(o, d, md), want, "between upload and render")
    got = np.zeros((FH, FW, 4), np.uint8)
    ctx = context_of(product)
    assert rxr.rxr_render_download(ctx, got.ctypes.data) == RXR_OK, last_error(rxr, ctx)
    assert np.array_equal(got, ref_frame)
