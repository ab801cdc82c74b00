"""The generated terrain's excluded sectors without a GPU (reference src/chunkbuilder/terrain_generator.rs: collect_excluded_sectors
:438-457, apply_exclusions :747-825, point_in_sector :891-950): the transcription (tests/terrain_exclusion_ref.py) against itself
(one point at a time against whole arrays), the conditions the shared fuzz scenes must satisfy, the host mirror's CPU
apply_exclusions against the transcription word for word, hand-derived pins of the reference's quirks, the refusals of
rxr_check_terrain_exclusions, the generated ffi, and the mirror's CPU functions under AddressSanitizer and UBSan in a stand-alone
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
from tests.terrain_exclusion_ref import Exclusions, square
from tests.terrain_gen_ref import F, Generator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")
SENTINEL = F(-12345.75)
SEEDS = [1, 2, 3]


@pytest.fixture(scope="module")
def api():
    return rusterix_amd.load()


def mirror_of(api, gen, excl):
    return api.TerrainGenerator(**gen.args()).set_exclusions(**excl.args())


def check_box(mirror, gen, excl, box, stride=None):
    """one box through the mirror's CPU apply_exclusions against the transcription: counts, x, z, w word for word, y the mirror's own
    grid height of the vertex's grid point, slots past n_vertices untouched.  Returns the transcription's record"""
    res = X.apply_exclusions(gen, excl, box)
    sx, sy, active, nv = res["counts"]
    if stride is None:
        stride = max(6 * max(sx - 1, 0) * max(sy - 1, 0), sx * sy) + 3
    counts, v = mirror.generate_meshes_cpu([box], stride, fill=float(SENTINEL))
    assert tuple(int(c) for c in counts[0]) == (sx, sy, active, nv), (counts[0], res["counts"])
    assert (v[0, nv:] == SENTINEL).all()
    if nv:
        want = X.expected_vertices(res)
        assert np.array_equal(v[0, :nv, [0, 2]].T.view(np.uint32), want.view(np.uint32))
        assert (v[0, :nv, 3] == F(1.0)).all()
        _, h = mirror.grid_heights_cpu([box], sx * sy)
        assert np.array_equal(v[0, :nv, 1].view(np.uint32), h[0][res["vertex_points"]].view(np.uint32))
    return res


# ---- the transcription against itself, and the fuzz scenes' conditions ----
@pytest.fixture(scope="module")
def fuzz():
    out = {}
    for seed in SEEDS:
        excl, boxes = X.fuzz_scene(seed)
        gen = G.scene(seed)
        out[seed] = (gen, excl, boxes, [X.apply_exclusions(gen, excl, b) for b in boxes])
    return out


def test_the_array_form_equals_the_line_by_line_form(fuzz):
    gen, excl, boxes, results = fuzz[1]
    res = results[0]
    rng = np.random.default_rng(5)
    pick = np.concatenate([rng.choice(len(res["points"]), 160, replace=False), np.nonzero(res["boundary"].any(axis=1))[0][:60]])
    extra = np.array([(NAN, 3), (3, NAN), (INF, 10), (-INF, -INF), (25, 13), (-0.0, 0.0)], F)
    for a, s in enumerate(res["active"]):
        verts = excl.polygons[s]
        for i in pick:
            inside, by_boundary = X.point_in_sector(*res["points"][i], verts)
            assert by_boundary == res["boundary"][i, a] and inside == (res["boundary"][i, a] or res["ray"][i, a]), (s, i)
        b, r = X.classify(extra, verts)
        for k, p in enumerate(extra):
            inside, by_boundary = X.point_in_sector(*p, verts)
            assert by_boundary == b[k] and inside == (b[k] or r[k]), (s, p)
    # rclamp01 is what `classify` restates with np.where: a NaN stays, -0.0 stays
    for t in (F(NAN), F(-0.0), F(-1.0), F(2.0), F(0.25)):
        w = np.where(np.array([t]) < F(0.0), F(0.0), np.where(np.array([t]) > F(1.0), F(1.0), np.array([t]))).astype(F)
        assert w.view(np.uint32)[0] == np.array([G.rclamp01(t)], F).view(np.uint32)[0]


@pytest.mark.parametrize("seed", SEEDS)
def test_the_fuzz_scenes_exercise_every_mechanism(fuzz, seed):
    gen, excl, boxes, results = fuzz[seed]
    res = results[0]   # the whole map
    keep, tris = res["keep"], res["triangles"]
    assert len(keep) == 2 * 64 * 64
    assert (~keep).sum() >= 0.10 * len(keep) and keep.sum() >= 0.10 * len(keep), ((~keep).sum(), keep.sum())
    inside = res["boundary"] | res["ray"]
    assert (res["boundary"] & ~res["ray"]).any(axis=1).sum() >= 8    # the boundary pass decided; the ray cast would have said outside
    assert (~res["boundary"] & res["ray"]).any(axis=1).sum() >= 8    # decided by the ray cast
    covered = inside.any(axis=1)
    spread = covered[tris].all(axis=1) & keep    # every corner inside a sector, no sector holding all three
    assert spread.sum() >= 1
    assert len(res["active"]) == len(excl.polygons)
    # the chunk boxes see some of the sectors only, and not all the same ones
    assert len({tuple(r["active"]) for r in results[1:]}) >= 3 and all(len(r["active"]) < len(excl.polygons) for r in results[1:])


# ---- the mirror against the transcription ----
@pytest.mark.parametrize("seed", SEEDS)
def test_the_mirror_equals_the_transcription_on_the_fuzz_scenes(api, fuzz, seed):
    gen, excl, boxes, results = fuzz[seed]
    mirror = mirror_of(api, gen, excl)
    for box in boxes:
        check_box(mirror, gen, excl, box)
    # ... point by point as well
    res = results[0]
    for a, s in enumerate(res["active"]):
        assert np.array_equal(mirror.points_in_sector_cpu(res["points"], s), res["boundary"][:, a] | res["ray"][:, a]), s
    # subdivisions 4 on a chunk
    gen4 = Generator(**{**gen.args(), "subdivisions": 4})
    r4 = check_box(mirror_of(api, gen4, excl), gen4, excl, boxes[2])
    assert r4["counts"][:2] == (65, 65) and 0 < (~r4["keep"]).sum() < len(r4["keep"])


def test_no_sector_is_the_shared_layout(api):
    gen = G.scene(1)
    res = check_box(mirror_of(api, gen, Exclusions()), gen, Exclusions(), (3.5, 2.0, 7.0, 6.25))
    assert res["counts"] == (5, 6, 0, 30)
    # an empty grid, a single point, and sectors that are all inactive
    far = Exclusions([square(50, 50, 52, 52)])
    for box, want in (((5, 5, 3, 3), (0, 0, 0, 0)), ((40, 40, 40, 40), (1, 1, 0, 1)), ((0, 0, 3, 2), (4, 3, 0, 12))):
        assert check_box(mirror_of(api, gen, far), gen, far, box)["counts"] == want


# ---- quirks pinned by hand ----
def pin(api, excl, box, counts, keep=None, subdivisions=1):
    gen = Generator(subdivisions=subdivisions)
    res = check_box(mirror_of(api, gen, excl), gen, excl, box)
    assert res["counts"] == counts, res["counts"]
    if keep is not None:
        assert res["keep"].tolist() == [bool(k) for k in keep], res["keep"]
    return res


def test_a_two_vertex_sector_is_active_and_holds_nothing(api):
    # its box hits the chunk: the layout is unshared, 16 cells, every triangle kept
    pin(api, Exclusions([[(1, 1), (2, 2)]]), (0, 0, 4, 4), (5, 5, 1, 96), [1] * 32)
    # ... and so is one without vertices (a sector whose linedefs are all missing), given its box
    pin(api, Exclusions([[]], boxes=[(1, 1, 2, 2)]), (0, 0, 4, 4), (5, 5, 1, 96))


def test_a_box_one_ulp_away_is_inactive_and_a_touching_one_is_active(api):
    tri = [(5, 1), (7, 1), (6, 3)]
    up, down = float(np.nextafter(F(4), F(INF))), float(np.nextafter(F(4), F(-INF)))
    pin(api, Exclusions([tri], boxes=[(up, 1, 7, 3)]), (0, 0, 4, 4), (5, 5, 0, 25))
    pin(api, Exclusions([tri], boxes=[(4, 1, 7, 3)]), (0, 0, 4, 4), (5, 5, 1, 96))
    pin(api, Exclusions([tri], boxes=[(4, 4, 7, 7)]), (0, 0, 4, 4), (5, 5, 1, 96))          # a corner
    pin(api, Exclusions([tri], boxes=[(-3, -3, 0, 0)]), (0, 0, 4, 4), (5, 5, 1, 96))
    pin(api, Exclusions([tri], boxes=[(-3, -3, -0.0, 0.0)]), (0.0, -0.0, 4, 4), (5, 5, 1, 96))   # -0.0 >= 0.0
    pin(api, Exclusions([tri], boxes=[(1, up, 3, 9)]), (0, 0, 4, 4), (5, 5, 0, 25))
    # the RAW box decides, not the floored and ceiled one the grid is made from: (0.5 .. 3.5) has the grid 0 .. 4
    pin(api, Exclusions([tri], boxes=[(3.75, 1, 7, 3)]), (0.5, 0.5, 3.5, 3.5), (5, 5, 0, 25))
    pin(api, Exclusions([tri], boxes=[(1, 1, 3, down)]), (0, 4, 4, 8), (5, 5, 0, 25))


def test_a_nan_box_is_inactive(api):
    sq = square(1, 1, 3, 3)
    for k in range(4):
        box = [1.0, 1.0, 3.0, 3.0]
        box[k] = NAN
        pin(api, Exclusions([sq], boxes=[box]), (0, 0, 4, 4), (5, 5, 0, 25))
    # ... and a NaN in the chunk's box makes every sector inactive
    pin(api, Exclusions([sq]), (0, 0, NAN, 4), (1, 5, 0, 5))


def test_corners_in_different_sectors_do_not_drop_a_triangle(api):
    # the grid 3 x 2 of (0,0)-(2,1): A holds the column x = 0, B the columns x = 1 and x = 2.  Cell 0's triangles have corners in
    # both and stay; cell 1 lies in B and goes
    a, b = square(-0.5, -0.5, 0.5, 1.5), square(0.75, -0.5, 2.5, 1.5)
    res = pin(api, Exclusions([a, b]), (0, 0, 2, 1), (3, 2, 2, 6), [1, 1, 0, 0])
    assert (res["boundary"] | res["ray"]).any(axis=1).all()   # every grid point lies in a sector
    assert res["vertex_points"].tolist() == [0, 3, 1, 1, 3, 4]


def test_a_sector_holding_three_corners_of_a_cell_drops_its_first_triangle_only(api):
    # the triangle x + y <= 1.1 holds (0,0), (0,1), (1,0) = (i0, i2, i1) and not (1,1)
    res = pin(api, Exclusions([[(-0.5, -0.5), (1.6, -0.5), (-0.5, 1.6)]]), (0, 0, 1, 1), (2, 2, 1, 3), [0, 1])
    assert res["vertex_points"].tolist() == [1, 2, 3]
    # ... and the mirror image holds (i1, i2, i3) and not i0
    pin(api, Exclusions([[(1.5, 1.5), (-0.6, 1.5), (1.5, -0.6)]]), (0, 0, 1, 1), (2, 2, 1, 3), [1, 0])
    # one cell kept, dropped (steps 2 x 2)
    pin(api, Exclusions([square(5, 5, 6, 6)], boxes=[(0, 0, 1, 1)]), (0, 0, 1, 1), (2, 2, 1, 6), [1, 1])
    pin(api, Exclusions([square(-1, -1, 2, 2)]), (0, 0, 1, 1), (2, 2, 1, 0), [0, 0])


def test_a_zero_length_edge_is_skipped(api):
    plain = pin(api, Exclusions([square(0.5, 0.5, 2.5, 2.5)]), (0, 0, 3, 3), (4, 4, 1, 6 * 9 - 6), None)
    twice = [(0.5, 0.5), (0.5, 0.5), (2.5, 0.5), (2.5, 2.5), (2.5, 2.5), (0.5, 2.5)]
    res = pin(api, Exclusions([twice]), (0, 0, 3, 3), (4, 4, 1, 6 * 9 - 6), plain["keep"])
    assert np.array_equal(res["ray"], plain["ray"]) and np.array_equal(res["boundary"], plain["boundary"])
    # every edge of length zero: three vertices, no boundary, no crossing
    pin(api, Exclusions([[(1, 1), (1, 1), (1, 1)]]), (0, 0, 2, 2), (3, 3, 1, 24), [1] * 8)


def test_a_nan_polygon_vertex(api):
    # the edges at the NaN vertex have a NaN squared length (not > 0.0: no boundary test) and compare false in the ray cast
    poly = [(0.5, 0.5), (NAN, 0.5), (2.5, 2.5), (0.5, 2.5)]
    gen = Generator()
    excl = Exclusions([poly], boxes=[(0, 0, 3, 3)])
    res = check_box(mirror_of(api, gen, excl), gen, excl, (0, 0, 3, 3))
    assert res["counts"][:3] == (4, 4, 1)
    for i, p in enumerate(res["points"]):
        inside, by_boundary = X.point_in_sector(*p, excl.polygons[0])
        assert inside == (res["boundary"][i, 0] or res["ray"][i, 0])
    excl = Exclusions([[(NAN, NAN), (NAN, NAN), (NAN, NAN)]], boxes=[(0, 0, 3, 3)])
    assert check_box(mirror_of(api, gen, excl), gen, excl, (0, 0, 3, 3))["counts"] == (4, 4, 1, 54)


def test_the_epsilon_band(api):
    # corners 0.005 inside the grid lines: the grid points on the lines x, y = 1 and 3 lie 0.005 (the corners 0.00707) outside the
    # square and are inside by the boundary pass; the ray cast calls them outside.  All 3 x 3 points in, the four cells between go
    res = pin(api, Exclusions([square(1.005, 1.005, 2.995, 2.995)]), (0, 0, 4, 4), (5, 5, 1, 96 - 24))
    inside = (res["boundary"] | res["ray"])[:, 0].reshape(5, 5)
    assert inside[1:4, 1:4].all() and inside.sum() == 9
    assert res["boundary"][:, 0].sum() == 8 and res["ray"][:, 0].reshape(5, 5)[2, 2] and res["ray"][:, 0].sum() == 1
    # at 0.02 they are outside: (2, 2) alone is in, nothing goes
    res = pin(api, Exclusions([square(1.02, 1.02, 2.98, 2.98)]), (0, 0, 4, 4), (5, 5, 1, 96), [1] * 32)
    assert (res["boundary"] | res["ray"]).sum() == 1 and not res["boundary"].any()


# ---- rxr_check_terrain_exclusions ----
def check(boxes=None, off=None, verts=None, S=0, V=0):
    rxr = rusterix_amd.rxr_abi()
    keep = [None if a is None else np.ascontiguousarray(a, np.uint32 if i == 1 else F) for i, a in enumerate((boxes, off, verts))]
    p = [None if a is None else a.ctypes.data for a in keep]
    msg = C.create_string_buffer(256)
    rc = rxr.rxr_check_terrain_exclusions(p[0], p[1], p[2], S, V, msg, len(msg))
    return rc, msg.value.decode()


def test_check_accepts():
    assert check() == (RXR_OK, "")
    assert check(np.full((2, 4), NAN), [0, 0, 3], np.full((3, 2), INF), 2, 3)[0] == RXR_OK
    assert check(np.zeros((1, 4)), [0, 0], None, 1, 0)[0] == RXR_OK   # a sector without vertices


def test_check_refuses_counts_above_the_caps():
    one = np.zeros(16, F)   # (never read: the count is refused first)
    rc, msg = check(one, one, one, (1 << 12) + 1, 4)
    assert rc == RXR_ERR_UNSUPPORTED and "MAX_EXCLUDED_SECTORS" in msg
    rc, msg = check(one, one, one, 1, (1 << 16) + 1)
    assert rc == RXR_ERR_UNSUPPORTED and "MAX_EXCLUSION_VERTICES" in msg


def test_check_refuses_null_arrays_and_inconsistent_offsets():
    z = np.zeros((4, 4), F)
    for kw in (dict(S=1, off=[0, 0]), dict(S=1, boxes=z), dict(S=1, boxes=z, off=[0, 2], V=2)):
        rc, msg = check(**kw)
        assert rc == RXR_ERR_INVALID and "NULL" in msg, (kw, rc, msg)
    for off, V in (([1, 2, 2], 2), ([0, 2, 1], 1), ([0, 1, 2], 3), ([0, 1, 4], 3)):
        rc, msg = check(z, off, z, 2, V)
        assert rc == RXR_ERR_INVALID and "vertex_offsets" in msg, (off, rc, msg)
    rc, msg = check(verts=z, V=2)
    assert rc == RXR_ERR_INVALID and "without a sector" in msg


def test_the_mirror_refuses_offsets_that_do_not_fit(api):
    m = api.TerrainGenerator()
    with pytest.raises(ValueError):
        m.set_exclusions([(0, 0, 1, 1)], [0, 2], [(0, 0), (1, 1), (2, 2)])
    with pytest.raises(ValueError):
        m.set_exclusions([(0, 0, 1, 1)], [0], [])


def test_the_generated_ffi_is_what_the_header_implies():
    pr = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_ffi.py"), "--check"], capture_output=True, text=True)
    assert pr.returncode == 0, pr.stdout + pr.stderr
    ffi = open(os.path.join(ROOT, "shim", "rusterix-hip-shim", "src", "ffi.rs")).read()
    for name in ("rxr_check_terrain_exclusions", "rxr_set_terrain_exclusions", "rxr_generated_meshes", "rxr_generated_meshes_to", "RXR_TERRAIN_GEN_MAX_EXCLUDED_SECTORS"):
        assert name in ffi, name


# ---- sanitizers, on a stand-alone program ----
def test_the_mirror_is_clean_under_asan_and_ubsan(api, tmp_path):
    # (`api`: the program links the device library the build makes; without it the fixture says so)
    exe = str(tmp_path / "terrain_exclusion_asan")
    csrc = os.path.join(ROOT, "rusterix_amd", "csrc")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-fno-fast-math", "-pthread", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-o", exe, os.path.join(ROOT, "tests", "terrain_exclusion_asan_main.cpp"),
           os.path.join(csrc, "host", "rusterix_host.cpp"), "-L" + csrc, "-lrxr_hip", "-Wl,-rpath," + csrc]
    pr = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if pr.returncode != 0 and ("-lasan" in pr.stderr or "-lubsan" in pr.stderr or "libasan" in pr.stderr or "libubsan" in pr.stderr):
        pytest.skip("no static sanitizer runtimes for this g++: " + pr.stderr[-200:])
    assert pr.returncode == 0, pr.stderr[-4000:]
    # the runtimes are inside the program (-static-libasan): the child takes the environment as it is, plus the sanitizers' options
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    pr = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert pr.returncode == 0 and "terrain exclusions under sanitizers: clean" in pr.stdout, (pr.stdout + pr.stderr)[-4000:]
