"""rxr_resize_meshes / rxr_resize_meshes_to on the GPU (include/rxr.h; kernels k_mesh_resize_check, k_mesh_repack in rxr_project.hip).

The main assertion is the EQUIVALENCE of tests/test_gpu_mesh_update.py: context A gets rxr_set_meshes(new geometry); context B gets
rxr_set_meshes(old geometry), one frame and one pick, then a resize to the new geometry.  Then the same device-projected 160 x 96
frame is byte-equal, rxr_read_projected_mesh is word-equal for every mesh (the unnamed neighbours, whose bases moved, included),
rxr_mesh_bounds is equal under == and rxr_intersect is bit-equal on seeded rays.  A refused call leaves B rendering (WITHOUT a new
upload), picking and bounded exactly as before it.  The `to` form writes its inputs on a fresh stream immediately before the call."""
import ctypes as C

import numpy as np
import pytest

from rusterix_amd import binding as B
from rusterix_amd import trace as T
from rusterix_amd.abi import RXR_ERR_INVALID, RXR_ERR_UNSUPPORTED, RXR_OK, rxr_texture, rxr_tile
from tests import mesh_resize_ref as MR
from tests import mesh_update_ref as M
from tests.pick_fuzz import IDENTITY, Mesh3D
from tests.test_gpu_mesh_update import FORMS, LIGHT, Ctx, assert_same, camera, snapshot, three, with_extreme

pytestmark = pytest.mark.gpu
F = np.float32
TEXEL = np.random.default_rng(77).integers(0, 256, (16, 16, 4), dtype=np.uint8)
TEXEL[..., 3] = 255


class RCtx(Ctx):
    """the update tests' context plus both resize forms; a mesh with a key `tile` is drawn from static tile 0 through its uvs"""

    def __init__(self):
        super().__init__()
        tex = rxr_texture(TEXEL.ctypes.data, 16, 16)
        tile = rxr_tile(C.pointer(tex), 1)
        assert self.rxr.rxr_set_textures(self.ctx, C.byref(tile), 1, None, 0) == RXR_OK, self.error()

    def set_meshes(self, meshes, expect=RXR_OK):
        if not any("tile" in m for m in meshes):
            return super().set_meshes(meshes, expect)
        arr = (Mesh3D * len(meshes))()
        keep = []
        for k, (a, m) in enumerate(zip(arr, meshes)):
            v, i, uv, nr = (np.ascontiguousarray(m[key], t) for key, t in (("vertices", F), ("indices", np.uint32), ("uvs", F), ("normals", F)))
            keep += [v, i, uv, nr]
            a.vertices, a.indices, a.uvs, a.normals = v.ctypes.data, i.ctypes.data, uv.ctypes.data, nr.ctypes.data
            a.n_vertices, a.n_triangles = len(v.reshape(-1, 4)), len(i.reshape(-1, 3))
            a.transform_3d = IDENTITY
            a.repeat_mode = B.REPEAT_REPEAT_XY
            if "tile" in m:
                a.source.kind, a.source.index = B.SOURCE_STATIC_TILE, m["tile"]
            else:
                a.source.kind = B.SOURCE_PIXEL
                a.source.pixel = (C.c_uint8 * 4)(200, 40 + 60 * k % 200, 90, 255)
            a.shader, a.list, a.chunk = -1, m["list"], m.get("chunk", -1)
        rc = self.rxr.rxr_set_meshes(self.ctx, C.cast(arr, C.c_void_p), len(meshes))
        assert rc == expect, f"rxr_set_meshes: {rc}: {self.error()}"
        self.meshes = list(meshes)

    def resize(self, named, new_meshes, form="host", uvs=True, **pack):
        """the resize of meshes `named` to `new_meshes` (same order); the status"""
        counts, v, uv, i, nr = MR.pack(new_meshes, **pack)
        return self.resize_arrays(named, counts, v, uv if uvs else None, i, nr, form)

    def resize_arrays(self, named, counts, v, uv, i, nr, form="host"):
        named = np.ascontiguousarray(named, np.uint32)
        if form == "host":
            return self.rxr.rxr_resize_meshes(self.ctx, named.ctypes.data, len(named), counts.ctypes.data, v.ctypes.data, None if uv is None else uv.ctypes.data,
                                              i.ctypes.data, nr.ctypes.data, v.shape[1], i.shape[1])
        import torch

        s = torch.cuda.Stream()
        with torch.cuda.stream(s):     # written on a fresh stream just before the call: the call must order itself behind them
            dev = [None if a is None else torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to("cuda", non_blocking=False).clone()
                   for a in (counts, v, uv, i, nr)]
        rc = self.rxr.rxr_resize_meshes_to(self.ctx, named.ctypes.data, len(named), *(None if d is None else (d.data_ptr() or None) for d in dev), v.shape[1], i.shape[1],
                                           s.cuda_stream)
        torch.cuda.synchronize()
        return rc


@pytest.fixture(scope="module")
def pair(product):
    a, b = RCtx(), RCtx()
    yield a, b, camera(product)
    a.close()
    b.close()


def equivalent(pair, old, new, named, form, order=None, uvs=True, **pack):
    """A: set_meshes(new).  B: set_meshes(old), a frame and a pick (so a resident frame and pick records exist), then the resize of `named`."""
    a, b, cam = pair
    a.set_meshes(new)
    want = snapshot(a, cam)
    b.set_meshes(old)
    before = snapshot(b, cam)
    order = list(named) if order is None else order
    rc = b.resize(order, [new[k] for k in order], form, uvs=uvs, **pack)
    assert rc == RXR_OK, b.error()
    assert b.render()[0] == RXR_ERR_INVALID, "the resident frame must be dropped by an accepted resize"
    b.meshes = list(new)
    got = snapshot(b, cam)
    assert_same(got, want, f"{form} {named}")
    return before, got


def recount(old, named, how, seed=100):
    """`old` with the named meshes at other counts: how = grow, shrink or mixed (by position in the scene)"""
    new = list(old)
    for k in named:
        nv, nt = len(old[k]["vertices"]), len(old[k]["indices"])
        up = how == "grow" or (how == "mixed" and k % 2 == 0)
        new[k] = MR.resized(old[k], nv + 17 if up else nv - 11, nt + 9 if up else nt - 7, seed + k)
    return new


# ---- equivalence ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("how", ["grow", "shrink", "mixed"])
@pytest.mark.parametrize("named", [[0], [1], [2], [2, 0, 1]], ids=["first", "middle", "last", "all-shuffled"])
def test_one_of_three_meshes_and_all_three(pair, named, how, form):
    old = three()
    new = recount(old, named, how)
    before, got = equivalent(pair, old, new, named, form)
    assert before["frame"].tobytes() != got["frame"].tobytes(), "the resize should show in the frame"
    assert len(np.unique(got["frame"].reshape(-1, 4), axis=0)) > 20 and (got["ray_mesh"] != 0xFFFFFFFF).any()


@pytest.mark.parametrize("form", FORMS)
def test_a_mesh_resized_to_nothing_and_one_resized_from_nothing(pair, form):
    old = three()
    new = list(old)
    old[0] = M.grid_mesh(0, 0, 0)
    new[1] = M.grid_mesh(0, 0, 1)
    _, got = equivalent(pair, old, new, [0, 1], form)
    assert (got["lo1"] == np.inf).all() and (got["hi1"] == -np.inf).all() and np.isfinite(got["lo0"]).all()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("nv", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_vertex_counts_with_the_extreme_vertex_first_last_and_in_the_last_partial_wave(pair, nv, form):
    places = [0, nv - 1, (nv - 1) // 64 * 64]
    old = [M.grid_mesh(40, 4, 10 + k, extent=1.5) for k in range(3)]
    new = [with_extreme(MR.resized(m, nv, 4, 200 + k, extent=1.5, centre=(0.0, 0.0, -6.0)), places[k]) for k, m in enumerate(old)]
    _, got = equivalent(pair, old, new, [0, 1, 2], form)
    for k in range(3):
        lo, hi = M.box_fast(new[k]["vertices"])
        assert (got[f"lo{k}"] == lo).all() and (got[f"hi{k}"] == hi).all()
        assert hi[0] == F(3.25) and lo[1] == F(-3.5) and lo[2] == F(-9.75)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("nt", [1, 85, 86, 8192])
def test_triangle_counts_around_256_index_words(pair, nt, form):
    old = [M.grid_mesh(40, 30, 20, extent=1.2), M.grid_mesh(7, 3, 21, centre=(2.5, 0, -6), extent=0.5)]
    new = [MR.resized(old[0], 40, nt, 300, extent=1.2), old[1]]
    new[0]["indices"][-1] = (39, 0, 39)      # (the largest legal index in the last word)
    equivalent(pair, old, new, [0], form)


@pytest.mark.parametrize("form", FORMS)
def test_300_one_triangle_meshes_every_second_one_resized_to_two(pair, form):
    rng = np.random.default_rng(7)
    old = [M.grid_mesh(3, 1, 500 + k, centre=(rng.uniform(-3, 3), rng.uniform(-2, 2), -6.0), extent=0.3) for k in range(300)]
    for m in old:
        m["indices"][:] = (0, 1, 2)
    named = list(range(0, 300, 2))
    new = list(old)
    for k in named:
        new[k] = MR.resized(old[k], 4, 2, 900 + k, extent=0.3)
        new[k]["indices"][:] = ((2, 1, 0), (3, 2, 0))
    equivalent(pair, old, new, named, form, order=[named[j] for j in rng.permutation(len(named))])


@pytest.mark.parametrize("form", FORMS)
def test_strides_beyond_the_counts_with_poisoned_slack(pair, form):
    old = three()
    new = recount(old, [0, 1, 2], "mixed", seed=600)
    equivalent(pair, old, new, [0, 1, 2], form, vstride=131, tstride=77, slack=True)


@pytest.mark.parametrize("form", FORMS)
def test_nan_vertices_are_ignored_and_zero_bounds_of_either_sign_compare_equal(pair, form):
    old = three()
    new = recount(old, [0, 1, 2], "grow", seed=700)
    new[0]["vertices"][5, 0] = np.nan       # one coordinate: the vertex's y and z still count
    new[0]["vertices"][9, :3] = np.nan
    new[1]["vertices"][:, :3] = np.nan      # nothing but NaN
    new[1]["vertices"].view(np.uint32)[3, 1] = 0x7FC12345     # (a payload: copied as words)
    v = new[2]["vertices"]
    v[:, 0] = np.where(np.arange(len(v)) % 2 == 0, F(-0.0), F(0.0))      # x: lo == hi == 0, of whichever sign
    _, got = equivalent(pair, old, new, [0, 1, 2], form)
    lo, hi = M.box(new[0]["vertices"])
    assert np.isfinite(lo).all() and (got["lo0"] == lo).all() and (got["hi0"] == hi).all()
    assert (got["lo1"] == np.inf).all() and (got["hi1"] == -np.inf).all()
    assert got["lo2"][0] == 0 and got["hi2"][0] == 0


@pytest.mark.parametrize("form", FORMS)
def test_uvs_reach_the_frame_and_clipped_uvs_and_null_means_zero(pair, form):
    old = three()
    old[1] = dict(old[1], tile=0)
    new = recount(old, [1, 2], "grow", seed=720)
    before, got = equivalent(pair, old, new, [2, 1], form)
    assert before["frame"].tobytes() != got["frame"].tobytes()
    # NULL uvs: A is registered with zero uvs for the named meshes
    zero = [dict(m, uvs=np.zeros_like(m["uvs"])) if k in (1, 2) else m for k, m in enumerate(new)]
    equivalent(pair, old, zero, [1, 2], form, uvs=False)


@pytest.mark.parametrize("form", FORMS)
def test_two_resizes_in_a_row_on_one_context(pair, form):
    """old -> mid -> new: the second call names meshes 1 and 0 only, so mesh 2 -- resized by the first call -- is copied out of the
    blob the first call built, into the blob the registration started in"""
    a, b, cam = pair
    old = three()
    mid = recount(old, [0, 2], "grow", seed=740)
    new = recount(mid, [0, 1], "shrink", seed=750)
    a.set_meshes(new)
    want = snapshot(a, cam)
    b.set_meshes(old)
    snapshot(b, cam)
    assert b.resize([0, 2], [mid[0], mid[2]], form) == RXR_OK, b.error()
    b.meshes = list(mid)
    snapshot(b, cam)
    assert b.resize([1, 0], [new[1], new[0]], form) == RXR_OK, b.error()
    b.meshes = list(new)
    assert_same(snapshot(b, cam), want, form)


@pytest.mark.parametrize("form", FORMS)
def test_an_update_after_a_resize_takes_the_new_counts(pair, form):
    a, b, cam = pair
    old = three()
    mid = recount(old, [1], "grow", seed=760)
    new = [mid[0], M.moved(mid[1], 761), M.moved(mid[2], 762)]
    a.set_meshes(new)
    want = snapshot(a, cam)
    b.set_meshes(old)
    snapshot(b, cam)
    assert b.resize([1], [mid[1]], form) == RXR_OK, b.error()
    # the update that the old registration accepted, with strides that fit either registration: refused for its counts
    assert b.update([1, 2], [M.moved(old[1], 763), new[2]], form, vstride=80, tstride=60) == RXR_ERR_INVALID and "vertex count differs" in b.error()
    assert b.update([2, 1], [new[2], new[1]], form) == RXR_OK, b.error()
    b.meshes = list(new)
    assert_same(snapshot(b, cam), want, form)


# ---- the ray queries' state ---------------------------------------------------------------------------------------------------------------
def test_a_pending_ranged_refresh_and_the_box_tree_do_not_survive_a_resize(pair):
    a, b, cam = pair
    old = three()
    moved = [M.moved(old[0], 770), old[1], old[2]]
    new = recount(moved, [1], "grow", seed=771)
    verify = lambda c: dict(zip(T.RAY_REFRESH_VERIFY, (int(x) for x in _verify(c))))

    def _verify(c):
        out = (C.c_uint64 * len(T.RAY_REFRESH_VERIFY))()
        assert c.rxr.rxr_ray_refresh_verify(c.ctx, out) == RXR_OK, c.error()
        return out

    for c in (a, b):
        assert c.rxr.rxr_set_ray_accel(c.ctx, T.RAY_ACCEL_ON) == RXR_OK and c.rxr.rxr_set_ray_refresh(c.ctx, T.RAY_REFRESH_RANGED) == RXR_OK
    try:
        a.set_meshes(new)
        want = snapshot(a, cam)
        b.set_meshes(old)
        snapshot(b, cam)                                              # (pick records and a tree exist)
        assert b.update([0], [moved[0]], "host") == RXR_OK, b.error()   # mesh 0 is pending a ranged refresh ...
        assert b.resize([1], [new[1]], "to") == RXR_OK, b.error()       # ... when the resize arrives
        b.meshes = list(new)
        got = snapshot(b, cam)
        assert_same(got, want, "ranged")
        found = verify(b)
        assert found["pick_words"] == 0 and found["sorted_words"] == 0 and found["nodes"] == 0, found
    finally:
        for c in (a, b):
            assert c.rxr.rxr_set_ray_accel(c.ctx, T.RAY_ACCEL_OFF) == RXR_OK and c.rxr.rxr_set_ray_refresh(c.ctx, T.RAY_REFRESH_FULL) == RXR_OK


def test_a_trace_is_refused_after_a_resize_until_the_trace_scene_is_set_again(pair):
    a, b, _ = pair
    old = three()
    new = recount(old, [0, 2], "mixed", seed=780)
    kind, consts = T.camera_firstp((0.0, 0.0, 0.0), (0.0, 0.0, -6.0), 60.0, 64, 36)

    def trace(c):
        acc = np.zeros((36, 64, 4), F)
        return c.rxr.rxr_trace(c.ctx, kind, consts.ctypes.data, 64, 36, 0, 1, 1, 2, acc.ctypes.data), acc

    light = (B.RxrLight * 1)(LIGHT)      # (direct light at the first hit: the sample is not all zero)
    set_scene = lambda c: c.rxr.rxr_set_trace_scene(c.ctx, None, None, 3, light, 1, 0, 1, None, 0)
    a.set_meshes(old)
    b.set_meshes(old)
    assert set_scene(a) == RXR_OK and set_scene(b) == RXR_OK, (a.error(), b.error())
    assert trace(b)[0] == RXR_OK, b.error()
    a.set_meshes(new)
    assert b.resize([0, 2], [new[0], new[2]], "to") == RXR_OK, b.error()
    rc_a, rc_b = trace(a)[0], trace(b)[0]
    assert rc_a == rc_b == RXR_ERR_INVALID, (rc_a, rc_b)                  # refused exactly as after rxr_set_meshes
    assert set_scene(a) == RXR_OK and set_scene(b) == RXR_OK, (a.error(), b.error())
    (rc_a, acc_a), (rc_b, acc_b) = trace(a), trace(b)
    assert rc_a == rc_b == RXR_OK, (a.error(), b.error())
    assert acc_a.tobytes() == acc_b.tobytes() and (acc_a[..., :3] != 0).any()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def refused(b, cam, call, why):
    """`call()` is RXR_ERR_INVALID with `why` in the message, and B renders the RESIDENT frame, picks and is bounded as before"""
    before = snapshot(b, cam)
    rc = call()
    assert rc == RXR_ERR_INVALID, (rc, b.error())
    assert why in b.error(), b.error()
    rc, px = b.render()                      # (no upload in between: the frame must still be resident)
    assert rc == RXR_OK and px.tobytes() == before["frame"].tobytes()
    assert_same(snapshot(b, cam), before, why)


@pytest.mark.parametrize("form", FORMS)
def test_refusals_found_by_the_check_kernel_change_nothing(pair, form):
    _, b, cam = pair
    old = three()
    b.set_meshes(old)
    new = recount(old, [0, 1, 2], "grow", seed=800)
    bad = list(new)
    bad[2] = dict(new[2], indices=new[2]["indices"].copy())
    nt = len(new[2]["indices"])
    bad[2]["indices"][-1, 2] = len(new[2]["vertices"])          # == the new vertex count, the last word of the last named mesh
    refused(b, cam, lambda: b.resize([0, 1, 2], bad, form), f"mesh_indices[2] = 2: triangle {nt - 1} has a vertex index")
    # an index that the OLD vertex count would have allowed to be larger is judged against the NEW one
    shrunk = recount(old, [1], "shrink", seed=801)
    worse = dict(shrunk[1], indices=shrunk[1]["indices"].copy())
    worse["indices"][0, 0] = len(old[1]["vertices"]) - 1
    refused(b, cam, lambda: b.resize([1], [worse], form), "mesh_indices[0] = 1: triangle 0 has a vertex index")
    for col, k, msg in ((0, 0, "vertices exceed vertex_stride 80"), (1, 1, "triangles exceed triangle_stride 60")):
        counts, v, uv, i, nr = MR.pack(new, vstride=80, tstride=60, slack=True)
        counts[k, col] = (80, 60)[col] + 1
        refused(b, cam, lambda: b.resize_arrays([0, 1, 2], counts, v, uv, i, nr, form), f"mesh_indices[{k}] = {k}: its {(81, 61)[col]} {msg}")
    # ... and the same arrays, untouched, are accepted afterwards
    assert b.resize([0, 1, 2], new, form) == RXR_OK, b.error()


@pytest.mark.parametrize("form", FORMS)
def test_refusals_found_on_the_host_change_nothing(pair, form):
    _, b, cam = pair
    old = three()
    b.set_meshes(old)
    new = recount(old, [0, 1, 2], "grow", seed=810)
    refused(b, cam, lambda: b.resize([0, 1, 0], [new[0], new[1], new[0]], form), "named twice")
    refused(b, cam, lambda: b.resize([0, 3], [new[0], new[1]], form), "no such mesh")
    refused(b, cam, lambda: b.resize([0, 1, 2, 1], new + [new[1]], form), "4 meshes named, 3 are registered")
    counts, v, uv, i, nr = MR.pack(new)
    vs, ts = v.shape[1], i.shape[1]
    named = np.arange(3, dtype=np.uint32)
    huge = (named.ctypes.data, 1 << 31, counts.ctypes.data, v.ctypes.data, uv.ctypes.data, i.ctypes.data, nr.ctypes.data, 0xFFFFFFFF, 0xFFFFFFFF)
    if form == "host":
        refused(b, cam, lambda: b.rxr.rxr_resize_meshes(b.ctx, *huge), "sizes overflow")
        refused(b, cam, lambda: b.rxr.rxr_resize_meshes(b.ctx, None, 3, *huge[2:7], vs, ts), "NULL mesh_indices")
        for k in (2, 3, 5, 6):     # counts, vertices, indices, normals (uvs may be NULL)
            args = list(huge[:7]) + [vs, ts]
            args[1], args[k] = 3, None
            refused(b, cam, lambda: b.rxr.rxr_resize_meshes(b.ctx, *args), "NULL array")
    else:
        import torch

        refused(b, cam, lambda: b.rxr.rxr_resize_meshes_to(b.ctx, *huge, None), "sizes overflow")
        dev = [torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda() for a in (counts, v, uv, i, nr)]
        torch.cuda.synchronize()
        p = [d.data_ptr() for d in dev]
        host = [a.ctypes.data for a in (counts, v, uv, i, nr)]
        for k, name in enumerate(("dev_counts", "dev_vertices", "dev_uvs", "dev_indices", "dev_normals")):
            # a host pointer, an odd address, and -- but for the uvs, which may be absent -- a NULL pointer
            for q, why in ((host[k], f"{name} is not device memory"), (p[k] + 2, f"{name} must be 4-byte aligned")) + (() if k == 2 else ((None, f"{name} must be 4-byte aligned"),)):
                args = p[:k] + [q] + p[k + 1:]
                refused(b, cam, lambda: b.rxr.rxr_resize_meshes_to(b.ctx, named.ctypes.data, 3, *args, vs, ts, None), why)
        # too small: the strides claim more than the allocation holds
        refused(b, cam, lambda: b.rxr.rxr_resize_meshes_to(b.ctx, named.ctypes.data, 3, *p, vs + (1 << 22), ts, None), "is not device memory")
    assert b.resize([0, 1, 2], new, form) == RXR_OK, b.error()


def test_no_valid_registration_and_the_empty_call():
    with RCtx() as c:
        one = M.grid_mesh(3, 1, 1)
        assert c.resize([], [], "host") == RXR_OK                       # n == 0 does nothing, registration or not
        assert c.resize([0], [one], "host") == RXR_ERR_INVALID and "no such mesh" in c.error()
        broken = dict(one, indices=np.array([[0, 1, 3]], np.uint32))
        c.set_meshes([one, broken], expect=RXR_ERR_INVALID)             # (leaves the context without a valid registration)
        for form in FORMS:
            assert c.resize([0], [one], form) == RXR_ERR_INVALID and "no valid registration" in c.error()
        c.set_meshes([one])
        assert c.resize([0], [MR.resized(one, 5, 3, 2)], "host") == RXR_OK, c.error()


def test_a_group_of_one_device_takes_the_host_form_only(pair):
    a, _, cam = pair
    old = three()
    new = recount(old, [0, 2], "mixed", seed=820)
    g = RCtx()
    g.close()                                                            # (a handle of rxr_create_multi in the plain one's place)
    devs = (C.c_int * 1)(0)
    assert g.rxr.rxr_create_multi(C.byref(g.ctx), devs, 1) == RXR_OK
    try:
        g.set_meshes(old)
        assert g.resize([2, 0], [new[2], new[0]], "to") == RXR_ERR_UNSUPPORTED and "multi-device" in g.error()
        assert g.resize([2, 0], [new[2], new[0]], "host") == RXR_OK, g.error()
        a.set_meshes(new)
        for k in range(3):
            assert all((x == y).all() for x, y in zip(g.bounds(k), a.bounds(k)))
        g.meshes = list(new)
        assert g.frame(cam).tobytes() == a.frame(cam).tobytes()
        assert g.resize([1, 1], [new[1], new[1]], "host") == RXR_ERR_INVALID and "named twice" in g.error()
    finally:
        g.close()


# ---- the chain: tile meshes -> vertex normals -> resize of the registered meshes, on one stream ------------------------------------------
CHAIN_BOXES = [(0, 0, 8, 8), (8, 0, 16, 8), (0, 8, 8, 16), (8, 8, 16, 16)]      # 2 x 2 chunks of 8 x 8 cells
MG, VS, TS = 2, 6 * 64, 2 * 64                                                 # two tile slots; the strides of a box of 64 cells


def chain_lists():
    """generator, tiles (two slots in stripes of four cells: every chunk has two groups), and the excluded sector before and after it
    moves from chunk 0 into chunk 1: the counts of those two chunks change, no chunk's number of groups does"""
    from tests import terrain_tiles_ref as TT
    from tests.terrain_exclusion_ref import Exclusions, square
    from tests.terrain_gen_ref import Generator

    gen = Generator([(3.0, 2.0, 2.5, 1.5), (12.5, 5.0, 2.0, 2.0), (6.0, 12.0, 1.5, 3.0)], map_box=(-20, -20, 36, 36))
    tiles = TT.Tiles(TT.stripes(0, 16, 0, 16, 2, width=4))
    return gen, tiles, Exclusions([square(2.5, 2.5, 5.5, 5.5)]), Exclusions([square(10.5, 2.5, 13.5, 6.5)])


def chain_camera(product):
    return camera(product, position=(8.0, 16.0, 26.0), center=(8.0, 0.0, 8.0))


def host_tile_meshes(c):
    """the resident lists' tile meshes of CHAIN_BOXES through the blocking forms (rxr_generated_tile_meshes, rxr_vertex_normals), as
    rxr_set_meshes takes them in mesh-slot order; and the calls' counts"""
    n = len(CHAIN_BOXES)
    bx = np.ascontiguousarray(CHAIN_BOXES, F)
    box_counts, counts, group_tiles = np.zeros((n, 4), np.uint32), np.zeros((n * MG, 2), np.uint32), np.zeros(n * MG, np.uint32)
    v, uv, idx = np.zeros((n * MG, VS, 4), F), np.zeros((n * MG, VS, 2), F), np.zeros((n * MG, TS, 3), np.uint32)
    rc = c.rxr.rxr_generated_tile_meshes(c.ctx, bx.ctypes.data, n, 1, MG, VS, TS, box_counts.ctypes.data, counts.ctypes.data, group_tiles.ctypes.data, v.ctypes.data,
                                         uv.ctypes.data, idx.ctypes.data)
    assert rc == RXR_OK, c.error()
    nr = np.zeros((n * MG, VS, 3), F)
    assert c.rxr.rxr_vertex_normals(c.ctx, n * MG, counts.ctypes.data, v.ctypes.data, idx.ctypes.data, nr.ctypes.data, VS, TS) == RXR_OK, c.error()
    meshes = [dict(vertices=v[m, :nv].copy(), indices=idx[m, :nt].copy(), uvs=uv[m, :nv].copy(), normals=nr[m, :nv].copy(), list=3) for m, (nv, nt) in enumerate(counts)]
    return meshes, box_counts, counts


def test_the_chain_resizes_registered_meshes_without_the_host(product):
    import torch

    from tests.test_gpu_terrain_tiles import set_exclusions, set_generator, set_tiles

    gen, tiles, before, after = chain_lists()
    cam = chain_camera(product)
    n = len(CHAIN_BOXES)
    with RCtx() as a, RCtx() as b:
        assert set_generator(b.rxr, b.ctx, gen) == RXR_OK and set_tiles(b.rxr, b.ctx, tiles) == RXR_OK and set_exclusions(b.rxr, b.ctx, before) == RXR_OK, b.error()
        old, old_boxes, old_counts = host_tile_meshes(b)
        assert set_exclusions(b.rxr, b.ctx, after) == RXR_OK, b.error()                # the sector moves
        new, new_boxes, new_counts = host_tile_meshes(b)
        changed = [k for k in range(n) if not np.array_equal(old_counts[MG * k:MG * k + MG], new_counts[MG * k:MG * k + MG])]
        assert changed == [0, 1] and (old_boxes[:, 3] == MG).all() and (new_boxes[:, 3] == MG).all(), (changed, old_boxes, new_boxes)
        a.set_meshes(new)                                                              # registered from the host arrays of the new terrain
        want = snapshot(a, cam)
        b.set_meshes(old)
        first = snapshot(b, cam)
        assert first["frame"].tobytes() != want["frame"].tobytes()
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            d_box, d_counts, d_tiles = (torch.zeros(k, dtype=torch.int32, device="cuda") for k in (4 * n, 2 * n * MG, n * MG))
            d_v, d_uv, d_nr = (torch.full((n * MG * VS * k,), float("nan"), device="cuda") for k in (4, 2, 3))
            d_idx = torch.full((n * MG * TS * 3,), -1, dtype=torch.int32, device="cuda")
        bx = np.ascontiguousarray(CHAIN_BOXES, F)
        sp = C.c_void_p(s.cuda_stream)
        rc = b.rxr.rxr_generated_tile_meshes_to(b.ctx, bx.ctypes.data, n, 1, MG, VS, TS, d_box.data_ptr(), d_counts.data_ptr(), d_tiles.data_ptr(), d_v.data_ptr(),
                                                d_uv.data_ptr(), d_idx.data_ptr(), sp)
        assert rc == RXR_OK, b.error()
        assert b.rxr.rxr_vertex_normals_to(b.ctx, n * MG, d_counts.data_ptr(), d_v.data_ptr(), d_idx.data_ptr(), d_nr.data_ptr(), None, VS, TS, sp) == RXR_OK, b.error()
        named = np.arange(n * MG, dtype=np.uint32)
        # the in-place update refuses these counts and changes nothing ...
        rc = b.rxr.rxr_update_meshes_to(b.ctx, named.ctypes.data, n * MG, d_counts.data_ptr(), d_v.data_ptr(), d_idx.data_ptr(), d_nr.data_ptr(), VS, TS, sp)
        assert rc == RXR_ERR_INVALID and "count differs" in b.error()
        assert b.render()[1].tobytes() == first["frame"].tobytes()
        # ... the resize takes them, with the uvs, from the same arrays on the same stream
        rc = b.rxr.rxr_resize_meshes_to(b.ctx, named.ctypes.data, n * MG, d_counts.data_ptr(), d_v.data_ptr(), d_uv.data_ptr(), d_idx.data_ptr(), d_nr.data_ptr(), VS, TS, sp)
        assert rc == RXR_OK, b.error()
        torch.cuda.synchronize()
        b.meshes = list(new)
        got = snapshot(b, cam)
        assert_same(got, want, "chain")
        rng = np.random.default_rng(0x7E44EB)                                          # rays straight down onto the terrain
        o = np.column_stack([rng.uniform(0.5, 15.5, 48), np.full(48, 30.0), rng.uniform(0.5, 15.5, 48)]).astype(F)
        d = np.column_stack([rng.uniform(-0.02, 0.02, 48), np.full(48, -1.0), rng.uniform(-0.02, 0.02, 48)]).astype(F)
        hit_b, hit_a = b.intersect(o, d, full=True), a.intersect(o, d, full=True)
        assert (hit_a["mesh"] < n * MG).sum() >= 30 and len(set(hit_a["mesh"].tolist())) >= 6
        for key in hit_a:
            assert np.array_equal(hit_b[key].view(np.uint32), hit_a[key].view(np.uint32)), key


# ---- the same through the host mirror ----------------------------------------------------------------------------------------------------
def generated_scene(api, gen, tiles, excl):
    """CHAIN_BOXES as four chunks, their tile groups as the chunks' batches3d (the mirror's CPU partition); (scene, render)"""
    mirror = api.TerrainGenerator(**gen.args()).set_exclusions(**excl.args()).set_tiles(**tiles.args())
    box_counts, counts, group_tiles, v, uv, idx = mirror.generate_tile_meshes_cpu(CHAIN_BOXES, MG, VS, TS)
    scene = api.Scene.empty()
    for b in range(len(CHAIN_BOXES)):
        chunk = scene.add_chunk()
        for g in range(int(box_counts[b, 3])):
            nv, nt = (int(c) for c in counts[b, g])
            colour = (60 + 150 * g, 220 - 50 * b, 90 + 60 * g, 255)
            chunk.add_batch3d(api.Batch3D.new(v[b, g, :nv], idx[b, g, :nt], uv[b, g, :nv]).with_computed_normals().source(B.PixelSource.Pixel(colour)))
    scene.lights([B.Light(B.LIGHT_POINT).with_position((8.0, 12.0, 8.0)).with_color((1.0, 0.95, 0.8)).with_intensity(3.0).with_start_distance(2.0)
                  .with_end_distance(80.0).compile()])
    cam = api.D3OrbitCamera.new()
    cam.set_parameter_f32("distance", 24.0)
    cam.center = (8.0, 0.0, 8.0)
    cam.azimuth, cam.elevation = 0.9, 0.8
    assets = api.Assets.default()

    def render():
        vm, pm = cam.matrices(160.0, 96.0)
        out = np.zeros(160 * 96 * 4, np.uint8)
        api.Rasterizer.setup(None, vm, pm).ambient((0.5, 0.5, 0.5, 1.0)).rasterize(scene, out, 160, 96, 32, assets)
        return out.reshape(96, 160, 4)

    return scene, render


def test_a_moved_sector_through_the_mirror_is_resized_on_the_device(product):
    api = product
    gen, tiles, before, after = chain_lists()
    api.lib.rxh_set_device_projection(1)
    try:
        want = generated_scene(api, gen, tiles, after)[1]()                             # the host route: registered from the new host arrays
        moved = api.TerrainGenerator(**gen.args()).set_exclusions(**after.args()).set_tiles(**tiles.args())
        # off (the default): as before, 1 -- replaced on the host
        scene, render = generated_scene(api, gen, tiles, before)
        first = render()
        assert first.tobytes() != want.tobytes() and scene.resize_meshes is False
        assert scene.rebuild_generated_tile_meshes(moved, CHAIN_BOXES, [0, 1, 2, 3], MG) == 1
        assert render().tobytes() == want.tobytes()
        # on: 2 -- resized on the device
        scene, render = generated_scene(api, gen, tiles, before)
        scene.resize_meshes = True
        assert render().tobytes() == first.tobytes() and scene.resize_meshes is True
        assert scene.rebuild_generated_tile_meshes(moved, CHAIN_BOXES, [0, 1, 2, 3], MG) == 2
        got = render()
        assert got.tobytes() == want.tobytes(), int((got != want).any(axis=2).sum())
        # the batches took the new counts and the fingerprints followed: the same call again finds nothing to resize and updates in place
        assert scene.rebuild_generated_tile_meshes(moved, CHAIN_BOXES, [0, 1, 2, 3], MG) == 0
        assert render().tobytes() == want.tobytes()
        # a chunk whose number of groups changed is still refused
        from tests import terrain_tiles_ref as TT

        other = api.TerrainGenerator(**gen.args()).set_exclusions(**after.args()).set_tiles(**TT.Tiles({(0, 0): 1}).args())
        with pytest.raises(Exception, match="tile groups"):
            scene.rebuild_generated_tile_meshes(other, CHAIN_BOXES, [0, 1, 2, 3], MG)
    finally:
        api.lib.rxh_set_device_projection(0)


def test_a_removed_cell_through_the_mirror_is_resized_on_the_device(product):
    from tests.test_gpu_mesh_update import CELLS, height, terrain_scene

    api = product
    base = {(x, y): height(x, y) for y in range(CELLS) for x in range(CELLS)}
    gone = {k: h for k, h in base.items() if k != (20, 5)}                              # a cell of chunk (1, 0)
    api.lib.rxh_set_device_projection(1)
    try:
        want = terrain_scene(api, gone)[2]()
        for on, code in ((False, 1), (True, 2)):
            t, scene, render = terrain_scene(api, base)
            scene.resize_meshes = on
            first = render()
            t.remove_height(20, 5)
            assert scene.rebuild_terrain_meshes(t, [(1, 0)], [1]) == code
            got = render()
            assert got.tobytes() == want.tobytes() and got.tobytes() != first.tobytes(), (on, int((got != want).any(axis=2).sum()))
            if on:      # the counts were adopted: a height stroke afterwards takes the in-place path
                t.set_height(22, 6, 3.0)
                assert scene.rebuild_terrain_meshes(t, [(1, 0)], [1]) == 0
                assert render().tobytes() == terrain_scene(api, {**gone, (22, 6): 3.0})[2]().tobytes()
    finally:
        api.lib.rxh_set_device_projection(0)
