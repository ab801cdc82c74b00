"""What the four device queries share on the host (rusterix_amd/csrc/rxr_query.h): the lane that orders a query's calls across
streams, and the staging of the blocking form's host arrays.  The same five cases for ray picking (rxr_intersect), shader bakes
(rxr_bake_shaders), terrain bakes (rxr_bake_terrain) and terrain picks (rxr_terrain_hits), outcomes only: every result is its numpy
reference's (tests/intersect_ref.py, bake_ref.py, terrain_ref.py, terrain_hit_ref.py), bit for bit.

    cross-stream order    `_to` with inputs X on stream A, at once the blocking form with Y, at once `_to` with X on stream B
    replacement           `_to` on stream A, at once other resident data (rxr_set_*), then the blocking form
    io buffer growth      `_to` on stream A, at once a blocking call whose host arrays no longer fit the lane's io buffer
    destroy               `_to` on stream A, at once rxr_destroy: the outputs are complete and outlive the context
    multi-device handles  the blocking form answers as member 0 does, the `_to` form is refused

One small shape per query: 70 rays (more than a wave) at four triangles, two programs at 8 x 8, one chunk of size 8 at 2 pixels
per tile, 300 terrain rays.  Each query's `big` inputs need more than 1.25 times the bytes of X plus 4096, the room a first
allocation of the io buffer leaves."""
import ctypes as C

import numpy as np
import pytest

import rusterix_amd
from rusterix_amd.abi import RXR_ERR_UNSUPPORTED, RXR_OK
from tests import bake_ref
from tests import intersect_ref
from tests import pick_fuzz
from tests import terrain_hit_ref
from tests import terrain_ref

pytestmark = pytest.mark.gpu

F = np.float32


def device(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def empty(shape, dtype):
    import torch

    return torch.zeros(shape, dtype=getattr(torch, dtype), device="cuda")


class Query:
    """one device query: set(ctx, k) makes resident data k (0 or 1) resident, inputs(which) are its `x`, `y` and `big` arguments,
    want(k, which) their reference on data k (computed once), blocking() / to() the two forms, host() a `_to` call's outputs"""

    def __init__(self):
        self.rxr = rusterix_amd.rxr_abi()
        self._want = {}

    def want(self, k, which):
        if (k, which) not in self._want:
            self._want[k, which] = self.reference(k, self.inputs(which))
        return self._want[k, which]

    def error(self, ctx):
        return (self.rxr.rxr_last_error(ctx) or b"").decode()

    def check(self, got, want, label):
        assert set(got) == set(want), label
        for key in want:
            a, b = np.ascontiguousarray(got[key]), np.ascontiguousarray(want[key])
            assert a.shape == b.shape and a.dtype.itemsize == b.dtype.itemsize, f"{label}: {key}"
            assert a.tobytes() == b.tobytes(), f"{label}: {key} differs from the reference"


class Intersect(Query):
    name = "intersect"

    def quads(self, z, shift):
        v = np.array([(0, 0, z, 1), (1, 0, z, 1), (1, 1, z, 1), (0, 1, z, 1)], F) + np.array([shift, 0, 0, 0], F)
        return pick_fuzz.mesh(v, [(0, 1, 2), (0, 2, 3)])

    def data(self, k):   # four triangles: two quads, at other depths and places for k == 1
        return [self.quads(2.0 + k, 0.25 * k), self.quads(1.0 + k, 0.5 - 0.25 * k)]

    def set(self, ctx, k):
        arr, keep = pick_fuzz.mesh_array(self.data(k))
        assert self.rxr.rxr_set_meshes(ctx, C.cast(arr, C.c_void_p), 2) == RXR_OK, self.error(ctx)

    def inputs(self, which):
        n, seed = dict(x=(70, 1), y=(70, 2), big=(400, 3))[which]
        rng = np.random.default_rng(seed)
        o = np.concatenate([rng.uniform(-0.5, 2.0, (n, 2)), np.full((n, 1), -1.0)], axis=1).astype(F)
        d = np.concatenate([rng.uniform(-0.2, 0.2, (n, 2)), np.ones((n, 1))], axis=1).astype(F)
        return o, d

    def reference(self, k, inputs):
        ref = intersect_ref.intersect_many(self.data(k), *inputs, full=True)
        assert 0 < (ref["mesh"] != intersect_ref.MISS).sum() < len(ref["mesh"])
        return ref

    def outputs(self, n, make):
        return dict(t=make((n,), "float32"), mesh=make((n,), "int32"), triangle=make((n,), "int32"), hitpoint=make((n, 3), "float32"),
                    uv=make((n, 2), "float32"), normal=make((n, 3), "float32"))

    def blocking(self, ctx, inputs):
        o, d = inputs
        out = self.outputs(len(o), lambda shape, dtype: np.zeros(shape, dtype))
        rc = self.rxr.rxr_intersect(ctx, o.ctypes.data, d.ctypes.data, len(o), 1, *(a.ctypes.data for a in out.values()))
        return rc, {k: (v.view(np.uint32) if v.dtype == np.int32 else v) for k, v in out.items()}

    def to(self, ctx, inputs, stream):
        import torch

        o, d = device(inputs[0]), device(inputs[1])
        out = self.outputs(len(inputs[0]), empty)
        torch.cuda.synchronize()
        rc = self.rxr.rxr_intersect_to(ctx, o.data_ptr(), d.data_ptr(), len(inputs[0]), 1, *(a.data_ptr() for a in out.values()), stream)
        return rc, (out, o, d)

    def host(self, queued):
        return {k: (v.cpu().numpy().view(np.uint32) if k in ("mesh", "triangle") else v.cpu().numpy()) for k, v in queued[0].items()}

    def check(self, got, want, label):
        bad = pick_fuzz.differences(got, want, label)
        assert set(got) == set(want) and bad is None, bad


class ShaderBake(Query):
    name = "bake_shaders"
    W = H = 8

    def __init__(self, oracle):
        super().__init__()
        self.oracle = oracle

    def data(self, k):   # two programs of exactly rounded operations, without patterns or palette
        progs = bake_ref.exact_programs()
        return [progs["gradient"], progs["arith"]] if k == 0 else [progs["loop"], progs["written"]]

    def set(self, ctx, k):
        sset, keep = bake_ref.shader_set(self.data(k))
        assert self.rxr.rxr_set_shaders(ctx, C.cast(C.pointer(sset), C.c_void_p)) == RXR_OK, self.error(ctx)

    def inputs(self, which):
        return np.array(dict(x=[0, 1], y=[1, 0], big=[0, 1, 1, 0, 0, 1, 0, 1])[which], np.uint32)

    def reference(self, k, order):
        ref = bake_ref.Reference(self.oracle, self.data(k))
        each = [ref.pixels(p, self.W, self.H) for p in range(2)]
        return dict(pixels=np.stack([each[p] for p in order]))

    def blocking(self, ctx, order):
        px = np.zeros((len(order), self.H, self.W, 4), F)
        by = np.zeros((len(order), self.H, self.W, 4), np.uint8)
        rc = self.rxr.rxr_bake_shaders(ctx, order.ctypes.data, len(order), self.W, self.H, px.ctypes.data, by.ctypes.data)
        return rc, dict(pixels=px, rgba=by)

    def to(self, ctx, order, stream):
        import torch

        px, by = empty((len(order), self.H, self.W, 4), "float32"), empty((len(order), self.H, self.W, 4), "uint8")
        torch.cuda.synchronize()
        rc = self.rxr.rxr_bake_shaders_to(ctx, order.ctypes.data, len(order), self.W, self.H, px.data_ptr(), by.data_ptr(), stream)
        return rc, (px, by)

    def host(self, queued):
        return dict(pixels=queued[0].cpu().numpy(), rgba=queued[1].cpu().numpy())

    def check(self, got, want, label):
        """the float buffer bit for bit; the bytes as tests/bake_ref.py states them from those floats (exact outside the band where
        a 16-ulp powf may truncate to the neighbouring byte)"""
        assert np.array_equal(got["pixels"].view(np.uint32), want["pixels"].view(np.uint32)), f"{label}: float pixels differ from the reference"
        for j in range(len(want["pixels"])):
            bake_ref.check_bytes(got["rgba"][j], want["pixels"][j], f"{label} (bake {j})")


class TerrainBake(Query):
    name = "bake_terrain"
    PPT = 2

    def data(self, k):   # 2 x 2 chunks of size 8, every cell blended at radius 1
        if not hasattr(self, "_specs"):
            self._specs = [terrain_ref.uniform_scene(terrain_ref.RADIUS, 1, chunk_size=8, chunks=2, seed=9 + i) for i in range(2)]
        return self._specs[k]

    def set(self, ctx, k):
        keep, args = self.data(k).arrays()
        assert self.rxr.rxr_set_terrain(ctx, *args) == RXR_OK, self.error(ctx)

    def inputs(self, which):
        return np.array(dict(x=[(0, 0)], y=[(1, 1)], big=[(0, 0), (1, 0), (0, 1), (1, 1), (1, 1), (0, 0)])[which], np.int32)

    def reference(self, k, coords):
        each = {c: self.data(k).bake(c, self.PPT) for c in {tuple(int(v) for v in c) for c in coords}}
        return dict(rgba=np.stack([each[tuple(int(v) for v in c)] for c in coords]))

    def blocking(self, ctx, coords):
        out = np.zeros((len(coords), 16, 16, 4), np.uint8)
        return self.rxr.rxr_bake_terrain(ctx, coords.ctypes.data, len(coords), self.PPT, out.ctypes.data), dict(rgba=out)

    def to(self, ctx, coords, stream):
        import torch

        out = empty((len(coords), 16, 16, 4), "uint8")
        torch.cuda.synchronize()
        return self.rxr.rxr_bake_terrain_to(ctx, coords.ctypes.data, len(coords), self.PPT, out.data_ptr(), stream), (out,)

    def host(self, queued):
        return dict(rgba=queued[0].cpu().numpy())


class TerrainHits(Query):
    name = "terrain_hits"
    MD = 20.0

    def data(self, k):
        return terrain_hit_ref.fuzz_spec(1 + k)

    def set(self, ctx, k):
        keep, args = self.data(k).arrays()
        assert self.rxr.rxr_set_terrain_heights(ctx, *args) == RXR_OK, self.error(ctx)

    def inputs(self, which):
        n, seed = dict(x=(300, 1), y=(300, 2), big=(600, 3))[which]
        o, d, _ = terrain_hit_ref.fuzz_rays(seed, n)
        return o, d

    def reference(self, k, inputs):
        ref = self.data(k).hits(*inputs, self.MD)
        assert 0 < ref["hit"].sum() < len(ref["hit"])
        return {key: ref[key] for key in terrain_hit_ref.KEYS}

    def outputs(self, n, make):
        return dict(hit=make((n,), "int32"), t=make((n,), "float32"), world_pos=make((n, 3), "float32"), grid_pos=make((n, 2), "int32"))

    def blocking(self, ctx, inputs):
        o, d = inputs
        out = self.outputs(len(o), lambda shape, dtype: np.zeros(shape, dtype))
        rc = self.rxr.rxr_terrain_hits(ctx, o.ctypes.data, d.ctypes.data, len(o), self.MD, *(a.ctypes.data for a in out.values()))
        out["hit"] = out["hit"].view(np.uint32)
        return rc, out

    def to(self, ctx, inputs, stream):
        import torch

        o, d = device(inputs[0]), device(inputs[1])
        out = self.outputs(len(inputs[0]), empty)
        torch.cuda.synchronize()
        rc = self.rxr.rxr_terrain_hits_to(ctx, o.data_ptr(), d.data_ptr(), len(inputs[0]), self.MD, *(a.data_ptr() for a in out.values()), stream)
        return rc, (out, o, d)

    def host(self, queued):
        out = {k: v.cpu().numpy() for k, v in queued[0].items()}
        out["hit"] = out["hit"].view(np.uint32)
        return out

    def check(self, got, want, label):
        bad = terrain_hit_ref.first_difference(got, want)
        assert set(got) == set(want) and not bad, f"{label}: {bad}"


@pytest.fixture(scope="module")
def queries(oracle):
    """the four queries; their references are computed once, by the first case that needs them"""
    return {q.name: q for q in (Intersect(), ShaderBake(oracle), TerrainBake(), TerrainHits())}


@pytest.fixture(params=["intersect", "bake_shaders", "bake_terrain", "terrain_hits"])
def q(request, queries, product):
    return queries[request.param]


@pytest.fixture()
def ctx(q):
    """a context of the test's own with resident data 0"""
    handle = C.c_void_p()
    assert q.rxr.rxr_create(C.byref(handle), 0) == RXR_OK
    q.set(handle, 0)
    yield handle
    q.rxr.rxr_destroy(handle)


def streams(n):
    import torch

    made = [torch.cuda.Stream() for _ in range(n)]
    return made, [C.c_void_p(s.cuda_stream) for s in made]


def test_cross_stream_order(q, ctx):
    _, (a, b) = streams(2)
    x, y = q.inputs("x"), q.inputs("y")
    rc_a, on_a = q.to(ctx, x, a)
    rc_host, host = q.blocking(ctx, y)
    rc_b, on_b = q.to(ctx, x, b)
    assert (rc_a, rc_host, rc_b) == (RXR_OK,) * 3, q.error(ctx)
    assert q.rxr.rxr_synchronize(ctx) == RXR_OK, q.error(ctx)
    q.check(q.host(on_a), q.want(0, "x"), "`_to` on stream A")
    q.check(host, q.want(0, "y"), "the blocking form")
    q.check(q.host(on_b), q.want(0, "x"), "`_to` on stream B")


def test_replacement_while_a_query_is_queued(q, ctx):
    made, (a,) = streams(1)
    rc_a, on_a = q.to(ctx, q.inputs("x"), a)
    q.set(ctx, 1)
    rc_host, host = q.blocking(ctx, q.inputs("y"))
    assert (rc_a, rc_host) == (RXR_OK, RXR_OK), q.error(ctx)
    made[0].synchronize()
    q.check(q.host(on_a), q.want(0, "x"), "`_to` on stream A, the old data")
    q.check(host, q.want(1, "y"), "the blocking form, the new data")


def test_io_buffer_growth(q, ctx):
    made, (a,) = streams(1)
    rc_first, first = q.blocking(ctx, q.inputs("x"))            # (allocates the io buffer: what X needs, times 1.25, plus 4096)
    rc_a, on_a = q.to(ctx, q.inputs("y"), a)
    rc_big, big = q.blocking(ctx, q.inputs("big"))
    assert (rc_first, rc_a, rc_big) == (RXR_OK,) * 3, q.error(ctx)
    made[0].synchronize()
    q.check(first, q.want(0, "x"), "the first blocking call")
    q.check(q.host(on_a), q.want(0, "y"), "`_to` on stream A")
    q.check(big, q.want(0, "big"), "the blocking call that outgrew the io buffer")


def test_destroy_while_a_query_is_queued(q):
    made, (a,) = streams(1)
    handle = C.c_void_p()
    assert q.rxr.rxr_create(C.byref(handle), 0) == RXR_OK
    q.set(handle, 0)
    rc, on_a = q.to(handle, q.inputs("x"), a)
    message = q.error(handle)
    q.rxr.rxr_destroy(handle)
    assert rc == RXR_OK, message
    made[0].synchronize()
    q.check(q.host(on_a), q.want(0, "x"), "`_to` on stream A, the context destroyed behind it")


def test_multi_device_handles(q):
    multi = C.c_void_p()
    assert q.rxr.rxr_create_multi(C.byref(multi), (C.c_int * 2)(0, 0), 2) == RXR_OK
    try:
        q.set(multi, 0)
        rc, host = q.blocking(multi, q.inputs("x"))
        assert rc == RXR_OK, q.error(multi)
        q.check(host, q.want(0, "x"), "the blocking form on a two-member handle")
        rc, _ = q.to(multi, q.inputs("x"), None)
        assert rc == RXR_ERR_UNSUPPORTED and "multi-device" in q.error(multi)
    finally:
        q.rxr.rxr_destroy(multi)
