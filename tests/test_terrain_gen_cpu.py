"""The generated terrain's height field without a GPU (reference src/chunkbuilder/terrain_generator.rs): hand-derived pins of the
reference, the host mirror's CPU TerrainGenerator against the numpy-float32 transcription (tests/terrain_gen_ref.py) by the
two-class rule -- bit-equal where no powf was evaluated, inside the transcription's interval elsewhere --, the transcription's own
height inside its interval, the refusals of rxr_check_terrain_generator, and the mirror's CPU functions under AddressSanitizer and
UBSan in a stand-alone program."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rusterix_amd
from rusterix_amd.abi import RXR_ERR_INVALID, RXR_ERR_UNSUPPORTED, RXR_OK
from tests import terrain_gen_ref as G
from tests.terrain_gen_ref import F, Generator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def api():
    return rusterix_amd.load()


def both(api, gen, points):
    """the transcription's and the mirror's f32 heights, which the pins below must both give"""
    ref = gen.sample(points)[0]
    mirror = api.TerrainGenerator(**gen.args()).sample_heights_cpu(points)
    return ref, mirror


def pin(api, gen, points, want):
    ref, mirror = both(api, gen, points)
    want = np.asarray(want, F)
    assert np.array_equal(ref.view(np.uint32), want.view(np.uint32)), (ref, want)
    assert np.array_equal(mirror.view(np.uint32), want.view(np.uint32)), (mirror, want)


def test_status_codes_are_the_headers():
    from rusterix_amd import binding as B

    assert (B.RXR_ERR_INVALID, B.RXR_ERR_UNSUPPORTED) == (RXR_ERR_INVALID, RXR_ERR_UNSUPPORTED)


# ---- hand-derived pins ----
def test_a_point_at_the_radius_has_t_one_half(api):
    # smoothness 2 -> radius 4 = smoothing; at distance 4 the sdf is 0: t = (4 - 0) / (2 * 4) = 0.5, smoothstep(0.5) = 0.5
    gen = Generator([(50, 50, 4, 2)])
    pin(api, gen, [(54, 50), (50, 46), (50, 50.5), (58, 50), (50, 59)], [2.0, 2.0, 4.0 * (0.9375 ** 2) * (3 - 2 * 0.9375), 0.0, 0.0])


def test_a_point_on_a_control_point_in_the_edge_band(api):
    # the exact match returns height * edge factor: 5 from the left edge, t = 0.5, smoothstep 0.5; the cones are not looked at
    # (the second control point would give 9 there)
    gen = Generator([(-95, 0, 3, 1), (-95, 1, 9, 50)])
    pin(api, gen, [(-95, 0)], [1.5])


def test_the_first_of_two_coincident_control_points_wins(api):
    gen = Generator([(10, 10, 2, 1), (10, 10, 5, 1)])
    pin(api, gen, [(10, 10)], [2.0])
    pin(api, Generator([(10, 10, 5, 1), (10, 10, 2, 1)]), [(10, 10)], [5.0])


def test_outside_the_map_box_the_base_is_zero(api):
    gen = Generator([(90, 0, 5, 30)])
    pin(api, gen, [(150, 0), (100, 0), (0, -100.5)], [0.0, 0.0, 0.0])


def test_no_control_points_means_no_edge_factor(api):
    # the ridge's height is not scaled by the map edge either way; with no control point the base is +0.0, not 0.0 * NaN
    gen = Generator([], [(2, 1, 4, 2)], [0, 1], [(0, 0, 10, 0)])
    pin(api, gen, [(5, 0.5), (NAN, 0.0)][:1], [2.0])
    ref, mirror = both(api, Generator(), [(NAN, NAN), (3, 4)])
    assert list(ref) == [0.0, 0.0] and list(mirror) == [0.0, 0.0]


def test_negative_heights_never_raise_the_maximum(api):
    gen = Generator([(10, 10, -3, 2), (12, 10, -1, 2)])
    pin(api, gen, [(10.5, 10), (11, 10), (30, 30)], [0.0, 0.0, 0.0])
    # ... but the exact match returns one
    pin(api, gen, [(10, 10)], [-3.0])


def test_a_ridge_plateau_band_and_beyond(api):
    # one edge (0,0)-(10,0), height 2, plateau 1, falloff 4, steepness 2: distance 0.5 -> 2; distance 3 -> t = 1 - 2/4, 2 * 0.5^2;
    # distance 5 -> falloff_dist 4 >= 4 -> 0; beyond the end point (13, 4): distance 5 -> 0
    gen = Generator([], [(2, 1, 4, 2)], [0, 1], [(0, 0, 10, 0)])
    pin(api, gen, [(5, 0.5), (5, 3), (5, 5), (13, 4), (5, -1)], [2.0, 0.5, 0.0, 0.0, 2.0])


def test_a_ridge_without_edges_and_a_degenerate_edge(api):
    # no edges: distance +inf, contribution 0.0.  The edge (3,4)-(3,4) is a point: (0,0) is 5 away -- inside a plateau of 5, and
    # with plateau 4.5, falloff 1, steepness 1: 2 * (1 - 0.5)
    gen = Generator([], [(7, 1, 4, 2), (2, 5, 1, 1), (2, 4.5, 1, 1)], [0, 0, 1, 2], [(3, 4, 3, 4), (3, 4, 3, 4)])
    pin(api, gen, [(0, 0), (3, 4)], [3.0, 4.0])


def test_two_overlapping_roads_with_total_influence_above_one(api):
    # both roads cover (5, 0) fully: after the first 0 * 0 + 1 * 1, after the second 1 * 0 + 3 * 1; total 2 -> excess 1:
    # 3 * (1 - 0.5) + 0 * 0.5
    gen = Generator(linedefs=[(0, 0, 10, 0, 1, 1, 2, 3, 2), (0, 1, 10, 1, 3, 3, 2, 3, 2)])
    pin(api, gen, [(5, 0)], [1.5])
    # the target is interpolated along the segment: a quarter of the way from 1 to 5
    gen = Generator(linedefs=[(0, 0, 8, 0, 1, 5, 1, 1, 1)])
    pin(api, gen, [(2, 0.5), (-3, 0), (20, 0.25), (4, 5)], [2.0, 0.0, 0.0, 0.0])


@pytest.mark.parametrize("box, subdivisions, want", [
    ((0.5, -1.5, 3.2, 2.0), 1, (5, 5)), ((0.5, -1.5, 3.2, 2.0), 2, (9, 9)), ((0.5, -1.5, 3.2, 2.0), 3, (13, 13)),
    ((-3.5, -2.25, -1.25, -0.5), 1, (4, 4)), ((-3.5, -2.25, -1.25, -0.5), 2, (7, 7)), ((-3.5, -2.25, -1.25, -0.5), 3, (10, 10)),
    ((2.0, 2.0, 2.0, 3.0), 1, (1, 2)), ((5.0, 5.0, 3.0, 3.0), 1, (-1, -1)), ((0.0, 0.0, NAN, 1.0), 2, (1, 3)),
    ((0.0, 0.0, INF, 1.0), 1, (-2 ** 31, 2)), ((0.0, 0.0, 3e9, 1.0), 1, (-2 ** 31, 2))])
def test_grid_counts(api, box, subdivisions, want):
    # floor / ceil of the box, then ceil(extent / cell_size) as i32 + 1: (0.5 .. 3.2) is 0 .. 4, four cells, five points; at
    # subdivisions 3 the cell is 0.33333334 and 4 / 0.33333334 rounds to 12.0; an extent beyond i32 saturates at i32::MAX and the + 1
    # wraps to i32::MIN as in a release build: no points (and none are allocated to find that out)
    gen = Generator(subdivisions=subdivisions)
    steps, pts = gen.generate_grid(box)
    assert steps == want
    msteps, mpts = api.TerrainGenerator(**gen.args()).generate_grid(box)
    assert msteps == want
    if want[0] > 0 and not np.isnan(box).any():
        assert np.array_equal(mpts.reshape(-1, 2).view(np.uint32), pts.view(np.uint32))
        assert np.array_equal(pts[0], np.floor(np.asarray(box[:2], F))) and len(pts) == want[0] * want[1]
        if want[0] > 1:
            assert np.array_equal(pts[1], pts[0] + np.array([F(1.0) / F(subdivisions), 0], F))   # iy-major: x runs first


@pytest.mark.parametrize("steps", [(1, 1), (2, 2), (5, 3), (2, 7), (1, 4)])
def test_triangulate_is_a_closed_form_of_the_counts(api, steps):
    got = api.TerrainGenerator.triangulate(*steps)
    assert np.array_equal(got, G.triangulate(*steps))
    assert len(got) == 2 * (steps[0] - 1) * (steps[1] - 1)


# ---- the mirror against the transcription ----
SCENES = {"hills_ridges_roads": dict(seed=1), "many_roads": dict(seed=2, n_control=2, n_ridges=1, n_lines=6), "ridges_only": dict(seed=3, n_control=3, n_ridges=4, n_lines=0)}


@pytest.fixture(scope="module")
def sampled():
    out = {}
    for name, kw in SCENES.items():
        gen, pts = G.scene(**kw), G.scene_points(kw["seed"], 240)
        out[name] = (gen, pts, gen.sample(pts))
    return out


@pytest.mark.parametrize("name", sorted(SCENES))
def test_the_transcription_lies_inside_its_own_interval_and_fills_both_classes(sampled, name):
    gen, pts, ref = sampled[name]
    rec = G.compare(name, ref[0], ref)
    print(name, rec)
    assert rec["largest_difference_ulp"] == 0.0 and rec["widest_interval_ulp"] >= 2 * G.POW_ULPS * 0.5


@pytest.mark.parametrize("name", sorted(SCENES))
def test_the_mirror_equals_the_transcription(api, sampled, name):
    gen, pts, ref = sampled[name]
    mirror = api.TerrainGenerator(**gen.args())
    rec = G.compare(name, mirror.sample_heights_cpu(pts), ref)
    print(name, rec)
    # normals: from the mirror's own three heights, by the transcription's tail of sample_normal_at
    h, nr = mirror.sample_normals_cpu(pts[:40])
    assert np.array_equal(h.view(np.uint32), mirror.sample_heights_cpu(pts[:40]).view(np.uint32))
    hr = mirror.sample_heights_cpu(pts[:40] + np.array([F(0.1), F(0.0)], F))
    hu = mirror.sample_heights_cpu(pts[:40] + np.array([F(0.0), F(0.1)], F))
    want = np.array([G.normal_from_heights(*t) for t in zip(h, hr, hu)])
    assert np.array_equal(nr.view(np.uint32), want.view(np.uint32))


def test_special_values_run_through_the_mirror_as_through_the_transcription(api):
    gen, pts = G.special_scene()
    ref = gen.sample(pts)
    assert 3 <= np.isnan(ref[0]).sum() <= len(pts) - 6 and np.isinf(ref[0]).any()
    G.compare("special", api.TerrainGenerator(**gen.args()).sample_heights_cpu(pts), ref, min_class_share=None)


def test_tile_normal_and_outline(api):
    gen = G.scene(seed=1, subdivisions=3)
    mirror = api.TerrainGenerator(**gen.args())
    want = gen.normals([(20.5, 31.5)])[0]
    # (inside an interval's width of the transcription's normal: the tile's three heights may have powf sites)
    assert np.allclose(mirror.tile_normal((20, 31)), want, rtol=0, atol=1e-4)
    outline = mirror.tile_outline_world((20, 31))
    step = F(1.0) / F(3.0)
    xz = [(F(20) + F(i) * step, F(31)) for i in range(3)] + [(F(21), F(31) + F(i) * step) for i in range(3)]
    xz += [(F(21) - F(i) * step, F(32)) for i in range(3)] + [(F(20), F(32) - F(i) * step) for i in range(3)]
    assert np.array_equal(outline[:, [0, 2]].view(np.uint32), np.array(xz, F).view(np.uint32))
    G.compare("outline", outline[:, 1], gen.sample(np.array(xz, F)), min_class_share=None)


# ---- rxr_check_terrain_generator ----
def check(cps=None, C_=0, ridges=None, R=0, off=None, edges=None, E=0, lines=None, L=0, box=(0, 0, 1, 1)):
    rxr = rusterix_amd.rxr_abi()
    keep = [None if a is None else np.ascontiguousarray(a, np.uint32 if i == 2 else F) for i, a in enumerate((cps, ridges, off, edges, lines, box))]
    p = [None if a is None else a.ctypes.data for a in keep]
    msg = C.create_string_buffer(256)
    rc = rxr.rxr_check_terrain_generator(p[0], C_, p[1], R, p[2], p[3], E, p[4], L, p[5], msg, len(msg))
    return rc, msg.value.decode()


def test_check_accepts():
    assert check() == (RXR_OK, "")
    assert check(np.zeros((2, 4)), 2, np.zeros((2, 4)), 2, [0, 0, 3], np.full((3, 4), NAN), 3, np.zeros((1, 9)), 1)[0] == RXR_OK
    assert check(off=[0], R=0)[0] == RXR_OK


def test_check_refuses_counts_above_the_caps():
    one = np.zeros(16, F)   # (never read: the count is refused first)
    for kw, name in ((dict(cps=one, C_=(1 << 16) + 1), "CONTROL_POINTS"), (dict(ridges=one, R=(1 << 12) + 1, off=one), "MAX_RIDGES"),
                     (dict(edges=one, E=(1 << 16) + 1), "RIDGE_EDGES"), (dict(lines=one, L=(1 << 14) + 1), "LINEDEFS")):
        rc, msg = check(**kw)
        assert rc == RXR_ERR_UNSUPPORTED and name in msg, (rc, msg)


def test_check_refuses_null_arrays():
    z = np.zeros((1, 9), F)
    for kw in (dict(C_=1), dict(R=1, off=[0, 0]), dict(R=1, ridges=z), dict(R=1, ridges=z, off=[0, 1], E=1), dict(L=1), dict(box=None)):
        rc, msg = check(**kw)
        assert rc == RXR_ERR_INVALID and "NULL" in msg, (kw, rc, msg)


def test_check_refuses_inconsistent_offsets():
    z = np.zeros((4, 4), F)
    for off, E in (([1, 2, 2], 2), ([0, 2, 1], 1), ([0, 1, 2], 3), ([0, 1, 4], 3)):
        rc, msg = check(ridges=z, R=2, off=off, edges=z, E=E)
        assert rc == RXR_ERR_INVALID and "ridge_edge_offsets" in msg, (off, rc, msg)
    rc, msg = check(edges=z, E=2)
    assert rc == RXR_ERR_INVALID and "without a ridge" in msg


# ---- sanitizers, on a stand-alone program ----
def test_the_mirror_is_clean_under_asan_and_ubsan(api, tmp_path):
    # (`api`: the program links the device library the build makes; without it the fixture says so)
    exe = str(tmp_path / "terrain_gen_asan")
    csrc = os.path.join(ROOT, "rusterix_amd", "csrc")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-fno-fast-math", "-pthread", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-o", exe, os.path.join(ROOT, "tests", "terrain_gen_asan_main.cpp"), os.path.join(csrc, "host", "rusterix_host.cpp"),
           "-L" + csrc, "-lrxr_hip", "-Wl,-rpath," + csrc]
    pr = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if pr.returncode != 0 and ("-lasan" in pr.stderr or "-lubsan" in pr.stderr or "libasan" in pr.stderr or "libubsan" in pr.stderr):
        pytest.skip("no static sanitizer runtimes for this g++: " + pr.stderr[-200:])
    assert pr.returncode == 0, pr.stderr[-4000:]
    # the runtimes are inside the program (-static-libasan): the child takes the environment as it is, plus the sanitizers' options
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    pr = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert pr.returncode == 0 and "terrain generator under sanitizers: clean" in pr.stdout, (pr.stdout + pr.stderr)[-4000:]
