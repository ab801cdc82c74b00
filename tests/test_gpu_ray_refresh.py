"""The ranged refresh after rxr_update_meshes (rxr_set_ray_refresh, include/rxr.h): under
RXR_RAY_REFRESH_RANGED the next query rewrites only the updated meshes' pick records and refits the box tree in the order of its last
build.  After every update and one query each case asserts
  (a) every output word of rxr_intersect, plain and full, is tests/intersect_ref.py's on the moved meshes -- and the same context's
      answer with the tree off;
  (b) rxr_ray_refresh_verify finds no pick-record word, no sorted-record word and no node that differs from a recomputation of all of
      them (a box left too large answers every ray correctly: only this catches it);
  (c) the build counter did not move, the tree is valid and nothing is pending;
  (d) the wild count is what a second context reports after registering the moved meshes fresh.
Every test calls rxr_set_ray_refresh: none can pass on a library without it."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from rusterix_amd import trace as T
from rusterix_amd.abi import RXR_ERR_INVALID, RXR_OK
from tests import intersect_ref as R
from tests import mesh_update_ref as M
from tests import pick_fuzz as P
from tests import ray_accel_ref as A
from tests import test_gpu_ray_accel as TA
from tests import trace_scenes as S

pytestmark = pytest.mark.gpu
F = np.float32
OFF, ON = T.RAY_ACCEL_OFF, T.RAY_ACCEL_ON
FULL, RANGED = T.RAY_REFRESH_FULL, T.RAY_REFRESH_RANGED
L = A.LEAF
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "rxr.h")).read()
SMALL_MAX = int(re.search(r"#define RXR_RAY_REFIT_SMALL_MAX (\d+)u", HEADER).group(1))
ROUTE_NONE, ROUTE_SMALL, ROUTE_GENERAL = (int(re.search(rf"#define RXR_RAY_REFIT_{k} (\d+)u", HEADER).group(1)) for k in ("NONE", "SMALL", "GENERAL"))
grid, aimed, accel_info = TA.grid, TA.aimed, TA.info


@pytest.fixture(scope="module")
def contexts():
    with P.PickContext() as a, P.PickContext() as b:
        yield a, b


@pytest.fixture
def pick(contexts):
    """a context in mode RANGED with the tree on; handed back with both defaults"""
    ctx = contexts[0]
    assert set_refresh(ctx, RANGED) == RXR_OK and TA.set_mode(ctx, ON) == RXR_OK
    yield ctx
    ctx.set_meshes([])
    assert set_refresh(ctx, FULL) == RXR_OK and TA.set_mode(ctx, OFF) == RXR_OK


@pytest.fixture
def fresh(contexts):
    """the second context: registers the moved meshes from scratch, tree on, refresh mode at its default"""
    ctx = contexts[1]
    assert TA.set_mode(ctx, ON) == RXR_OK
    yield ctx
    ctx.set_meshes([])
    assert TA.set_mode(ctx, OFF) == RXR_OK


def set_refresh(ctx, mode):
    return ctx.rxr.rxr_set_ray_refresh(ctx.ctx, mode)


def refresh_info(ctx):
    out = (C.c_uint64 * len(T.RAY_REFRESH_INFO))()
    assert ctx.rxr.rxr_ray_refresh_info(ctx.ctx, out) == RXR_OK, ctx.error()
    return dict(zip(T.RAY_REFRESH_INFO, (int(x) for x in out)))


def verify(ctx):
    out = (C.c_uint64 * len(T.RAY_REFRESH_VERIFY))()
    assert ctx.rxr.rxr_ray_refresh_verify(ctx.ctx, out) == RXR_OK, ctx.error()
    return dict(zip(T.RAY_REFRESH_VERIFY, (int(x) for x in out)))


def update(ctx, named, new_meshes):
    """rxr_update_meshes for meshes `named` (indices) with the geometry of `new_meshes`; the status"""
    counts, v, idx, nr = M.pack(new_meshes)
    named = np.asarray(named, np.uint32)
    return ctx.rxr.rxr_update_meshes(ctx.ctx, named.ctypes.data, len(named), counts.ctypes.data, v.ctypes.data, idx.ctypes.data, nr.ctypes.data,
                                     v.shape[1], idx.shape[1])


def regrid(m, seed, offset=(0.0, 0.0, 0.0), scale=1.0):
    """the counts, uvs, list and profile id of grid mesh `m` (an update changes none of them) over another seed's geometry"""
    n = len(m["indices"])
    new = grid(n, seed)
    assert len(new["vertices"]) == len(m["vertices"])
    v = new["vertices"].copy()
    v[:, :3] = v[:, :3] * F(scale) + np.asarray(offset, F)
    return dict(m, vertices=v, indices=new["indices"], normals=new["normals"])


def start(ctx, meshes, rays=None):
    """registers `meshes` and runs one many-ray query: records and tree stand; (builds, refresh info) after it"""
    ctx.set_meshes(meshes)
    o, d = rays if rays is not None else aimed(meshes, (0.3, 6.0, 2.5), np.random.default_rng(1), 80)
    ctx.intersect(o, d)
    i = accel_info(ctx)
    assert i["valid"] == 1 and refresh_info(ctx)["pending"] == 0
    return i["builds"], refresh_info(ctx)


def apply(ctx, meshes, changes):
    """one update call naming dict `changes` (mesh index -> new mesh); the mesh list afterwards"""
    named = sorted(changes)
    rc = update(ctx, named, [changes[k] for k in named])
    assert rc == RXR_OK, ctx.error()
    return [changes.get(k, m) for k, m in enumerate(meshes)]


def the_four(ctx, fresh, meshes, builds, label, eye=(0.3, 6.0, 2.5), seed=3, targets=None, n_rays=300, min_hits=30):
    """(a) to (d) of the module's docstring for `ctx` holding `meshes` with updates pending; returns the refresh info after the query"""
    rng = np.random.default_rng(seed)
    o, d = aimed(targets if targets is not None else meshes, eye, rng, n_rays)
    ref = R.intersect_many(meshes, o, d, full=True)
    assert accel_info(ctx)["valid"] == 0 and refresh_info(ctx)["pending"] > 0, label
    stale = verify(ctx)      # nothing is refreshed yet: the verification sees the old records and, where a tree stands, the old boxes
    assert stale["pick_words"] > 0 and (stale["checked"] == 1 or (stale["sorted_words"] > 0 and stale["nodes"] > 0)), (label, stale)
    got = ctx.intersect(o, d, full=True)      # the query that refreshes
    info = refresh_info(ctx)
    bad = P.differences(got, ref, f"{label}: full, against the restatement,")
    assert bad is None, bad
    bad = P.differences(ctx.intersect(o, d, full=False), P.plain_of(ref), f"{label}: plain, against the restatement,")
    assert bad is None, bad
    assert TA.set_mode(ctx, OFF) == RXR_OK
    for full in (True, False):
        bad = P.differences(ctx.intersect(o, d, full=full), ref if full else P.plain_of(ref), f"{label}: tree off, full={full},")
        assert bad is None, bad
    assert TA.set_mode(ctx, ON) == RXR_OK
    assert (ref["mesh"] != R.MISS).sum() >= min_hits, label
    v = verify(ctx)                                                                                           # (b)
    assert (v["pick_words"], v["sorted_words"], v["nodes"], v["checked"]) == (0, 0, 0, 3), (label, v)
    i = accel_info(ctx)                                                                                       # (c)
    assert (i["builds"], i["valid"]) == (builds, 1) and refresh_info(ctx)["pending"] == 0, (label, builds, i)
    fresh.set_meshes(meshes)                                                                                  # (d)
    fresh.intersect(o, d)
    f = accel_info(fresh)
    assert f["valid"] == 1 and i["wild"] == f["wild"] == v["wild"], (label, i["wild"], f["wild"], v["wild"])
    return info


# ---- a leaf across two meshes ---------------------------------------------------------------------------------------------------------
def test_a_leaf_straddling_two_meshes(pick, fresh):
    """13 and 11 triangles: positions 8 .. 15 are one leaf over both meshes.  The first alone, the second alone, then both"""
    meshes = [grid(13, 1), grid(11, 2, list=R.LIST_DYNAMIC)]
    builds, r0 = start(pick, meshes)
    meshes = apply(pick, meshes, {0: regrid(meshes[0], 11, (0.5, 0.2, 0.0))})
    r1 = the_four(pick, fresh, meshes, builds, "first mesh")
    assert (r1["triangles"], r1["leaves"], r1["nodes"], r1["route"]) == (13, 2, 3, ROUTE_SMALL) and r1["refits"] == r0["refits"] + 1
    meshes = apply(pick, meshes, {1: regrid(meshes[1], 12, (-0.5, 0.0, 0.3))})
    r2 = the_four(pick, fresh, meshes, builds, "second mesh")
    assert (r2["triangles"], r2["leaves"], r2["nodes"]) == (11, 2, 3)
    meshes = apply(pick, meshes, {0: regrid(meshes[0], 13), 1: regrid(meshes[1], 14)})
    r3 = the_four(pick, fresh, meshes, builds, "both meshes")
    assert (r3["triangles"], r3["leaves"], r3["nodes"]) == (24, 3, 4) and r3["refreshes"] == r0["refreshes"] + 3


# ---- totals at which a level fills ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", (0, 1, 2))
@pytest.mark.parametrize("total", (64, 65, 512, 513, 4097))
def test_level_edges(pick, fresh, total, which):
    """2, 3, 3, 4 and 5 levels; the dirty mesh first, in the middle and last"""
    assert len(A.levels(total)) == {64: 2, 65: 3, 512: 3, 513: 4, 4097: 5}[total]
    a = total // 3
    sizes = (a, a + 1, total - 2 * a - 1)
    meshes = [grid(n, 20 + k, list=(R.LIST_STATIC, R.LIST_DYNAMIC, R.LIST_OVERLAY)[k]) for k, n in enumerate(sizes)]
    builds, _ = start(pick, meshes)
    meshes = apply(pick, meshes, {which: regrid(meshes[which], 40 + which, (0.3, -0.2, 0.1))})
    r = the_four(pick, fresh, meshes, builds, f"{total} triangles, mesh {which}", targets=[meshes[which]] + meshes)
    b, e = sum(sizes[:which]), sum(sizes[:which + 1])
    leaves = (e - 1) // L - b // L + 1
    assert (r["triangles"], r["leaves"]) == (sizes[which], leaves) and r["nodes"] >= leaves + len(A.levels(total)) - 1


# ---- boxes that must shrink and grow --------------------------------------------------------------------------------------------------
def test_a_box_that_must_shrink(pick, fresh):
    """a mesh registered 500 units away comes into the middle of the others: verify proves its leaves and every ancestor shrank"""
    meshes = [grid(200, 1), regrid(grid(120, 2), 2, (500.0, -300.0, 400.0)), grid(90, 3, list=R.LIST_DYNAMIC)]
    builds, _ = start(pick, meshes)
    meshes = apply(pick, meshes, {1: regrid(meshes[1], 5)})
    the_four(pick, fresh, meshes, builds, "moved in", targets=[meshes[1]])


def test_a_box_that_must_grow(pick, fresh):
    """a mesh moves 500 units away and the rays follow it: a tree with the old boxes culls them at the root"""
    meshes = [grid(200, 1), grid(120, 2), grid(90, 3, list=R.LIST_DYNAMIC)]
    builds, _ = start(pick, meshes)
    far = regrid(meshes[1], 6, (500.0, -300.0, 400.0))
    meshes = apply(pick, meshes, {1: far})
    the_four(pick, fresh, meshes, builds, "moved away", eye=(480.0, -290.0, 420.0), targets=[far], min_hits=100)


# ---- wildness -------------------------------------------------------------------------------------------------------------------------
def test_triangles_that_become_wild_and_tame_again(pick, fresh):
    base = [grid(300, 1), grid(150, 2, list=R.LIST_DYNAMIC)]
    builds, _ = start(pick, base)
    assert accel_info(pick)["wild"] == 0
    nan = dict(base[1], vertices=base[1]["vertices"].copy())
    bad = int(nan["indices"][70, 1])
    nan["vertices"][bad, 1] = np.nan
    n_nan = int((nan["indices"] == bad).any(axis=1).sum())
    meshes = apply(pick, base, {1: nan})
    the_four(pick, fresh, meshes, builds, "a NaN vertex")
    assert accel_info(pick)["wild"] == n_nan > 0
    # a sliver: the third vertex of triangle 5 of mesh 0 goes next to the middle of its first edge, kappa far above the cap (every
    # triangle that shares the vertex changes with it; the restatement says how many end up wild); and the NaN goes away again
    thin = dict(base[0], vertices=base[0]["vertices"].copy())
    i0, i1, i2 = (int(x) for x in thin["indices"][5])
    thin["vertices"][i2, :3] = (thin["vertices"][i0, :3] + thin["vertices"][i1, :3]) * F(0.5) + np.array([0, 1e-7, 0], F)
    p0, e1, e2 = A.records(*(thin["vertices"][thin["indices"][:, k].astype(np.int64), :3] for k in range(3)))
    n_thin = int(A.wild(p0, e1, e2).sum())
    assert n_thin >= 1
    meshes = apply(pick, meshes, {0: thin, 1: base[1]})
    the_four(pick, fresh, meshes, builds, "a sliver, the NaN gone")
    assert accel_info(pick)["wild"] == n_thin
    meshes = apply(pick, meshes, {0: base[0]})
    the_four(pick, fresh, meshes, builds, "tame again")
    assert accel_info(pick)["wild"] == 0


# ---- an update that changes only the indices -------------------------------------------------------------------------------------------
def test_changed_indices_only(pick, fresh):
    meshes = [grid(100, 1), grid(333, 2, list=R.LIST_DYNAMIC), grid(50, 3, list=R.LIST_OVERLAY)]
    builds, _ = start(pick, meshes)
    perm = np.random.default_rng(9).permutation(333)
    shuffled = dict(meshes[1], indices=np.ascontiguousarray(meshes[1]["indices"][perm]))
    meshes = apply(pick, meshes, {1: shuffled})
    r = the_four(pick, fresh, meshes, builds, "permuted triangles", targets=[shuffled])
    assert r["triangles"] == 333


# ---- dirty sets -----------------------------------------------------------------------------------------------------------------------
def many(sizes, seed=0):
    lists = (R.LIST_STATIC, R.LIST_STATIC, R.LIST_DYNAMIC, R.LIST_OVERLAY, R.LIST_OVERLAY)
    return [grid(n, seed + 10 * k + 1, list=lists[min(k * len(lists) // len(sizes), len(lists) - 1)]) for k, n in enumerate(sizes)]


def test_two_adjacent_meshes_whose_intervals_merge(pick, fresh):
    meshes = many((90, 70, 61, 45, 200, 33))
    builds, _ = start(pick, meshes)
    meshes = apply(pick, meshes, {2: regrid(meshes[2], 71, (0.2, 0, 0)), 3: regrid(meshes[3], 72, (0, 0.2, 0))})
    r = the_four(pick, fresh, meshes, builds, "adjacent")
    b, e = sum(len(m["indices"]) for m in meshes[:2]), sum(len(m["indices"]) for m in meshes[:4])
    assert r["leaves"] == (e - 1) // L - b // L + 1      # one merged interval, the shared leaf counted once


def test_two_meshes_far_apart(pick, fresh):
    meshes = many((90, 70, 61, 45, 200, 33, 800, 12))
    builds, _ = start(pick, meshes)
    meshes = apply(pick, meshes, {0: regrid(meshes[0], 73), 7: regrid(meshes[7], 74, (0, 0, 0.3))})
    the_four(pick, fresh, meshes, builds, "far apart", targets=[meshes[0], meshes[7]])


def test_all_meshes(pick, fresh):
    meshes = many((90, 70, 61, 45, 200, 33))
    builds, _ = start(pick, meshes)
    meshes = apply(pick, meshes, {k: regrid(m, 80 + k) for k, m in enumerate(meshes)})
    r = the_four(pick, fresh, meshes, builds, "all meshes")
    total = sum(len(m["indices"]) for m in meshes)
    assert (r["triangles"], r["leaves"], r["nodes"]) == (total, A.levels(total)[0], sum(A.levels(total)))


def test_a_mesh_without_triangles_among_the_named(pick, fresh):
    meshes = [grid(90, 1), grid(0, 2), grid(70, 3, list=R.LIST_DYNAMIC)]
    builds, r0 = start(pick, meshes)
    meshes = apply(pick, meshes, {1: regrid(meshes[1], 5), 2: regrid(meshes[2], 6)})
    assert refresh_info(pick)["pending"] == 2
    r = the_four(pick, fresh, meshes, builds, "an empty mesh named")
    assert r["triangles"] == 70
    # the empty mesh alone: nothing to rewrite, nothing pending afterwards, the tree stays valid
    meshes = apply(pick, meshes, {1: regrid(meshes[1], 7)})
    o, d = aimed(meshes, (0.3, 6.0, 2.5), np.random.default_rng(2), 100)
    assert P.differences(pick.intersect(o, d, full=True), R.intersect_many(meshes, o, d, full=True), "only the empty mesh:") is None
    r2 = refresh_info(pick)
    assert (r2["pending"], r2["triangles"], r2["leaves"], r2["route"]) == (0, 0, 0, ROUTE_NONE) and r2["refits"] == r["refits"]
    assert accel_info(pick)["valid"] == 1 and accel_info(pick)["builds"] == builds
    v = verify(pick)
    assert (v["pick_words"], v["sorted_words"], v["nodes"]) == (0, 0, 0)


def test_257_one_triangle_meshes_in_one_call(pick, fresh):
    """past the 256 meshes one launch of the update's kernels names"""
    meshes = [grid(1, 100 + k) for k in range(257)] + [grid(150, 5, list=R.LIST_DYNAMIC)]
    builds, _ = start(pick, meshes)
    meshes = apply(pick, meshes, {k: regrid(meshes[k], 500 + k, (0.1, 0.0, 0.1)) for k in range(257)})
    assert refresh_info(pick)["pending"] == 257
    r = the_four(pick, fresh, meshes, builds, "257 meshes", min_hits=20)
    assert (r["triangles"], r["leaves"]) == (257, 33)


def test_two_update_calls_before_one_query(pick, fresh):
    """the set is a union: mesh 2 is named by both calls and counted once; its second geometry is the one that stands"""
    meshes = many((90, 70, 61, 45, 200, 33))
    builds, r0 = start(pick, meshes)
    meshes = apply(pick, meshes, {1: regrid(meshes[1], 91), 2: regrid(meshes[2], 92)})
    assert refresh_info(pick)["pending"] == 2
    meshes = apply(pick, meshes, {2: regrid(meshes[2], 93, (0.0, 0.4, 0.0)), 4: regrid(meshes[4], 94)})
    assert refresh_info(pick)["pending"] == 3
    r = the_four(pick, fresh, meshes, builds, "two calls")
    assert r["triangles"] == sum(len(meshes[k]["indices"]) for k in (1, 2, 4)) and r["refreshes"] == r0["refreshes"] + 1


# ---- both refit routes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("leaves", (SMALL_MAX - 1, SMALL_MAX, SMALL_MAX + 1))
def test_both_refit_routes(pick, fresh, leaves):
    """the dirty mesh starts at position 0 and ends on a leaf's edge: exactly `leaves` dirty leaves"""
    meshes = [grid(leaves * L, 1), grid(100, 2, list=R.LIST_DYNAMIC)]
    builds, _ = start(pick, meshes)
    meshes = apply(pick, meshes, {0: regrid(meshes[0], 3, (0.2, 0.1, 0.0))})
    r = the_four(pick, fresh, meshes, builds, f"{leaves} dirty leaves")
    assert r["leaves"] == leaves and r["route"] == (ROUTE_SMALL if leaves <= SMALL_MAX else ROUTE_GENERAL), r
    assert SMALL_MAX * 32 <= 65536      # the nodes the one-launch route keeps in LDS


# ---- tree off, RANGED on --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rays", (8, 300))
def test_tree_off(pick, n_rays):
    """8 rays take the thread-per-triangle path, 300 the brute many-ray path: both read the refreshed pick records"""
    assert TA.set_mode(pick, OFF) == RXR_OK
    meshes = [grid(200, 1), grid(120, 2, list=R.LIST_DYNAMIC)]
    pick.set_meshes(meshes)
    o, d = aimed(meshes, (0.3, 6.0, 2.5), np.random.default_rng(4), n_rays)
    pick.intersect(o, d)
    r0, a0 = refresh_info(pick), accel_info(pick)
    meshes = apply(pick, meshes, {1: regrid(meshes[1], 8, (0.3, 0.3, 0.0))})
    assert refresh_info(pick)["pending"] == 1
    o, d = aimed([meshes[1]], (0.3, 6.0, 2.5), np.random.default_rng(5), n_rays)
    ref = R.intersect_many(meshes, o, d, full=True)
    assert P.differences(pick.intersect(o, d, full=True), ref, f"{n_rays} rays, tree off:") is None
    assert P.differences(pick.intersect(o, d), P.plain_of(ref), f"{n_rays} rays, tree off, plain:") is None
    assert (ref["mesh"] == 1).sum() >= 2
    r1, a1 = refresh_info(pick), accel_info(pick)
    assert (r1["pending"], r1["refreshes"], r1["refits"], r1["triangles"], r1["leaves"], r1["route"]) == (0, r0["refreshes"] + 1, r0["refits"], 120, 0, ROUTE_NONE)
    assert (a1["builds"], a1["batches"], a1["valid"]) == (a0["builds"], a0["batches"], 0)
    v = verify(pick)
    assert (v["pick_words"], v["checked"]) == (0, 1)


# ---- mode transitions -----------------------------------------------------------------------------------------------------------------
def test_the_tree_is_switched_on_after_updates_are_pending(pick, fresh):
    assert TA.set_mode(pick, OFF) == RXR_OK
    meshes = [grid(200, 1), grid(120, 2, list=R.LIST_DYNAMIC)]
    pick.set_meshes(meshes)
    o, d = aimed(meshes, (0.3, 6.0, 2.5), np.random.default_rng(4), 100)
    pick.intersect(o, d)
    r0, a0 = refresh_info(pick), accel_info(pick)
    meshes = apply(pick, meshes, {0: regrid(meshes[0], 8)})
    assert TA.set_mode(pick, ON) == RXR_OK
    r = the_four(pick, fresh, meshes, a0["builds"] + 1, "switched on while pending")      # no tree stood: a plain build, no refit
    assert (r["refreshes"], r["refits"], r["leaves"]) == (r0["refreshes"] + 1, r0["refits"], 0)


def test_a_tree_that_stands_while_the_mode_is_off_is_dropped(pick):
    meshes = [grid(200, 1), grid(120, 2, list=R.LIST_DYNAMIC)]
    builds, r0 = start(pick, meshes)
    assert TA.set_mode(pick, OFF) == RXR_OK
    meshes = apply(pick, meshes, {0: regrid(meshes[0], 8)})
    o, d = aimed(meshes, (0.3, 6.0, 2.5), np.random.default_rng(4), 100)
    ref = R.intersect_many(meshes, o, d, full=True)
    assert P.differences(pick.intersect(o, d, full=True), ref, "dropped:") is None
    assert refresh_info(pick)["refits"] == r0["refits"] and accel_info(pick)["valid"] == 0
    assert TA.set_mode(pick, ON) == RXR_OK
    assert P.differences(pick.intersect(o, d, full=True), ref, "built again:") is None
    assert accel_info(pick)["builds"] == builds + 1 and verify(pick)["nodes"] == 0


def test_invalidate_is_followed_by_exactly_one_build(pick, fresh):
    meshes = [grid(200, 1), grid(120, 2, list=R.LIST_DYNAMIC)]
    builds, r0 = start(pick, meshes)
    o, d = aimed(meshes, (0.3, 6.0, 2.5), np.random.default_rng(4), 100)
    assert pick.rxr.rxr_ray_accel_invalidate(pick.ctx) == RXR_OK
    assert accel_info(pick)["valid"] == 0
    pick.intersect(o, d)
    pick.intersect(o, d)
    assert accel_info(pick)["builds"] == builds + 1 and accel_info(pick)["valid"] == 1
    # with a mesh pending: its pick records are refreshed, the tree is built, not refitted
    meshes = apply(pick, meshes, {1: regrid(meshes[1], 9)})
    assert pick.rxr.rxr_ray_accel_invalidate(pick.ctx) == RXR_OK
    r = the_four(pick, fresh, meshes, builds + 2, "invalidated while pending")
    assert (r["refreshes"], r["refits"]) == (r0["refreshes"] + 1, r0["refits"])


def test_set_meshes_clears_the_pending_set(pick, fresh):
    meshes = [grid(200, 1), grid(120, 2, list=R.LIST_DYNAMIC)]
    builds, r0 = start(pick, meshes)
    apply(pick, meshes, {1: regrid(meshes[1], 9)})
    assert refresh_info(pick)["pending"] == 1
    other = [grid(77, 5), grid(40, 6, list=R.LIST_OVERLAY)]
    pick.set_meshes(other)
    assert refresh_info(pick)["pending"] == 0 and accel_info(pick)["valid"] == 0
    o, d = aimed(other, (0.3, 6.0, 2.5), np.random.default_rng(4), 100)
    assert P.differences(pick.intersect(o, d, full=True), R.intersect_many(other, o, d, full=True), "after rxr_set_meshes:") is None
    r = refresh_info(pick)
    assert (r["refreshes"], r["refits"]) == (r0["refreshes"], r0["refits"]) and accel_info(pick)["builds"] == builds + 1
    v = verify(pick)
    assert (v["pick_words"], v["sorted_words"], v["nodes"], v["checked"]) == (0, 0, 0, 3)


def test_a_refused_update_leaves_nothing_pending(pick):
    meshes = [grid(200, 1), grid(120, 2, list=R.LIST_DYNAMIC)]
    builds, r0 = start(pick, meshes)
    o, d = aimed(meshes, (0.3, 6.0, 2.5), np.random.default_rng(4), 100)
    before = pick.intersect(o, d, full=True)
    assert update(pick, [1], [grid(121, 7, list=R.LIST_DYNAMIC)]) == RXR_ERR_INVALID      # a triangle count that differs
    assert "count differs" in pick.error()
    assert refresh_info(pick)["pending"] == 0 and accel_info(pick)["valid"] == 1
    assert P.differences(pick.intersect(o, d, full=True), before, "after the refusal:") is None
    assert P.differences(before, R.intersect_many(meshes, o, d, full=True), "against the restatement:") is None
    r = refresh_info(pick)
    assert (r["refreshes"], r["refits"]) == (r0["refreshes"], r0["refits"]) and accel_info(pick)["builds"] == builds


def test_full_while_pending_gives_one_build(pick):
    meshes = [grid(200, 1), grid(120, 2, list=R.LIST_DYNAMIC)]
    builds, r0 = start(pick, meshes)
    meshes = apply(pick, meshes, {1: regrid(meshes[1], 9)})
    assert set_refresh(pick, FULL) == RXR_OK
    r = refresh_info(pick)
    assert (r["mode"], r["pending"]) == (FULL, 0) and accel_info(pick)["valid"] == 0
    o, d = aimed(meshes, (0.3, 6.0, 2.5), np.random.default_rng(4), 100)
    ref = R.intersect_many(meshes, o, d, full=True)
    assert P.differences(pick.intersect(o, d, full=True), ref, "FULL while pending:") is None
    pick.intersect(o, d)
    r = refresh_info(pick)
    assert (r["refreshes"], r["refits"]) == (r0["refreshes"], r0["refits"]) and accel_info(pick)["builds"] == builds + 1
    # and under FULL an update invalidates, as it always did
    meshes = apply(pick, meshes, {0: regrid(meshes[0], 10)})
    assert refresh_info(pick)["pending"] == 0 and accel_info(pick)["valid"] == 0
    assert P.differences(pick.intersect(o, d, full=True), R.intersect_many(meshes, o, d, full=True), "under FULL:") is None
    assert accel_info(pick)["builds"] == builds + 2


def test_other_modes_are_refused_and_change_nothing(pick):
    assert refresh_info(pick)["mode"] == RANGED
    assert set_refresh(pick, 2) == RXR_ERR_INVALID and "rxr_set_ray_refresh" in pick.error()
    assert set_refresh(pick, 0xFFFFFFFF) == RXR_ERR_INVALID
    assert refresh_info(pick)["mode"] == RANGED
    assert set_refresh(pick, FULL) == RXR_OK and set_refresh(pick, 2) == RXR_ERR_INVALID and refresh_info(pick)["mode"] == FULL
    assert pick.rxr.rxr_set_ray_refresh(None, RANGED) == RXR_ERR_INVALID


# ---- the tracer -----------------------------------------------------------------------------------------------------------------------
def test_trace_after_an_update_equals_a_fresh_registration():
    """the 96-triangle room at 64 x 36; the inner box moves by rxr_update_meshes, then one sample in mode RANGED: every float of the
    accumulation buffer is what a second context writes that registered the moved room, seed and frame the same"""
    w, h, seed, inner = 64, 36, 5, 6
    scene = S.diffuse_room()
    assert sum(len(m["indices"]) for m in scene["meshes"]) == 96
    cam = S.cameras(w, h)["firstp"]
    box = S.box(3.4, 0.0, 3.2, 2, 2, 2)
    moved = dict(scene["meshes"][inner], vertices=box["vertices"], indices=box["indices"], normals=box["normals"])
    with T.Tracer() as tr, T.Tracer() as other:
        S.load(tr, scene)
        tr.ray_accel, tr.ray_refresh = ON, RANGED
        first = T.AccumBuffer(w, h)
        tr.trace(cam, first, n_frames=1, seed=seed, bounces=4)
        a0, r0 = tr.ray_accel_info(), tr.ray_refresh_info()
        assert a0["valid"] == 1
        counts, v, idx, nr = M.pack([moved])
        named = np.array([inner], np.uint32)
        rc = tr.rxr.rxr_update_meshes(tr.ctx, named.ctypes.data, 1, counts.ctypes.data, v.ctypes.data, idx.ctypes.data, nr.ctypes.data, v.shape[1], idx.shape[1])
        assert rc == RXR_OK, tr.error()
        assert tr.ray_refresh_info()["pending"] == 1 and tr.ray_accel_info()["valid"] == 0
        got = T.AccumBuffer(w, h)
        tr.trace(cam, got, n_frames=1, seed=seed, bounces=4)
        a1, r1 = tr.ray_accel_info(), tr.ray_refresh_info()
        assert (a1["builds"], a1["valid"]) == (a0["builds"], 1) and (r1["pending"], r1["refits"], r1["triangles"]) == (0, r0["refits"] + 1, 12)
        v1 = tr.ray_refresh_verify()
        assert (v1["pick_words"], v1["sorted_words"], v1["nodes"], v1["checked"]) == (0, 0, 0, 3)
        S.load(other, dict(scene, meshes=[moved if k == inner else m for k, m in enumerate(scene["meshes"])]))
        other.ray_accel = ON
        want = T.AccumBuffer(w, h)
        other.trace(cam, want, n_frames=1, seed=seed, bounces=4)
        assert a1["wild"] == other.ray_accel_info()["wild"]
    bits = got.pixels.view(np.uint32) == want.pixels.view(np.uint32)
    assert bits.all(), f"{int((~bits).sum())} floats differ from the fresh registration's"
    assert (got.pixels.view(np.uint32) != first.pixels.view(np.uint32)).any()      # the box did move in the picture


# ---- seeded scenes --------------------------------------------------------------------------------------------------------------------
def jittered(m, rng):
    """the same counts: vertices shifted and scaled, and for half of the meshes the triangles in another order"""
    v = m["vertices"].copy()
    v[:, :3] = (v[:, :3] * F(rng.uniform(0.7, 1.3)) + rng.standard_normal(3).astype(F) * F(0.4)).astype(F)
    idx = m["indices"]
    if rng.random() < 0.5 and len(idx):
        idx = np.ascontiguousarray(idx[rng.permutation(len(idx))])
    return dict(m, vertices=v, indices=idx)


@pytest.mark.parametrize("seed", P.SEEDS[:4])
def test_seeded_scenes_ten_strokes_each(pick, seed):
    """a random subset of a generated scene's meshes, ten times: (a) and (b) after every stroke"""
    meshes = P.random_pick_scene(seed)
    o, d = P.random_rays(meshes, seed, 200)
    builds, _ = start(pick, meshes, rays=(o, d))
    rng = np.random.default_rng([seed, 77])
    for stroke in range(10):
        named = [k for k in range(len(meshes)) if rng.random() < 0.3] or [int(rng.integers(len(meshes)))]
        meshes = apply(pick, meshes, {k: jittered(meshes[k], rng) for k in named})
        ref = R.intersect_many(meshes, o, d, full=True)
        label = f"seed {seed}, stroke {stroke} ({len(named)} meshes)"
        bad = P.differences(pick.intersect(o, d, full=True), ref, label + ":")
        assert bad is None, bad
        bad = P.differences(pick.intersect(o[:65], d[:65]), P.prefix(P.plain_of(ref), 65), label + ", 65 rays, plain:")
        assert bad is None, bad
        v = verify(pick)
        assert (v["pick_words"], v["sorted_words"], v["nodes"]) == (0, 0, 0), (label, v)
        assert v["wild"] == accel_info(pick)["wild"], label
    assert accel_info(pick)["builds"] == builds and refresh_info(pick)["pending"] == 0


def test_scene_ray_refresh_through_the_mirror(product):
    """Scene.ray_refresh hands the mode to the context next to ray_accel"""
    meshes = [grid(300, 61), grid(50, 62, list=R.LIST_OVERLAY)]
    scene = P.host_scene(product, meshes)
    o, d = aimed(meshes, (0.3, 6.0, 2.0), np.random.default_rng(15), 200)
    try:
        assert scene.ray_refresh == FULL
        scene.intersect(o, d)
        assert scene.ray_refresh_info()["mode"] == FULL
        scene.ray_refresh = RANGED
        got = scene.intersect(o, d, full=True)
        i = scene.ray_refresh_info()
        assert (i["mode"], i["pending"]) == (RANGED, 0)
        assert P.differences(got, R.intersect_many(meshes, o, d, full=True), "the mirror:") is None
    finally:
        scene.ray_refresh = FULL
        scene.intersect(o[:1], d[:1])    # (hands the default back to the shared context)
