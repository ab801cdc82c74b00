"""A frame does not depend on the context's earlier frames.

A context carries state from one frame to the next: the bins and counter sets every launch hands back zeroed (rxr_device.h), the parities
of the alternating counter sets, scratch_dirty, blockscan_off and the rings of bad shapes, list_capacity, host_records, frame_uses_*,
the modules of the compiled program set, a dozen buffers that only grow -- and the host mirror its generation-keyed residency of
textures, program sets and meshes.  tests/test_gpu_routes.py gives every raster kernel ONE frame, compared with the oracle; the only
route-to-route transitions it exercises are those the file order happens to produce.

Here every state of STATES (the 21 routes that need no context of their own, and ten frames that move state the route scenes leave
alone) is drawn once by a context that has drawn nothing else: that frame is the reference, so the bar is bit-exact for relaxed lit frames
too.  test_walk_from(first) then alternates `first` with every other state on the host mirror's one context; over all parameters every
ordered pair of states is consecutive somewhere (schedule, checked without a GPU).  After EVERY frame: the bytes equal the reference's,
the kernel is the state's, the scratch words the next launch assumes zero are zero, the frame was not silently rendered again (a stale
count repaired by the second attempt would hide exactly there), and the run-time compiler says what the state expects.

Every state's cfg is built once per module and reused on every visit: coming back to a state meets the mirror's generation checks while
the context holds another state's textures, program set and meshes.  Nothing is compared with the oracle on the GPU (test_gpu_routes.py
and the builders' own tests do that); profiles/route_walk/README.md has the times and the two mutations the walk was tried against."""
import collections
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest

import rusterix_amd
from rusterix_amd import scenes
from tests.routes import assert_route
from tests.test_gpu_routes import ROUTES, SMALL, _oracle_frame, _recreate_context, cloud_scene, knobs

gpu = pytest.mark.gpu

# name: the test id; build(api) -> cfg; env: per-upload variables; device: device projection; kernel: what a fresh context reports for the
# frame; may_rerender: the frame may be drawn twice (history-dependent in HOW it is drawn, not in what); jit: RXR_SHADER_JIT of a program state
State = collections.namedtuple("State", "name build env device kernel may_rerender jit")

EXCLUDED = {name for name, r in ROUTES.items() if r["ctx_env"]}   # (a create-time variable: a context of its own, test_gpu_routes.py)


def _route_states():
    return [State(name, r["build"], r["env"], False, name, False, r["env"].get("RXR_SHADER_JIT") if r["kw"].get("prog") else None)
            for name, r in ROUTES.items() if not r["ctx_env"]]


def _extra(name, kernel, build, env=None, device=False, may_rerender=False, **kw):
    return State(name, functools.partial(build, **kw), env or {}, device, kernel, may_rerender, None)


# Every variable below is read per upload (rxr_upload.hip: RXR_LIGHT_MATH in the RasterParams phase, RXR_BLOCKSCAN and RXR_BLOCKSCAN2D where
# the scratch is sized), none by rxr_create.  The kernel names are what a fresh context reported on an MI355X, recorded once.
EXTRAS = [
    # rxr_set_meshes, frame_uses_meshes, k_proj*
    _extra("x_cloud_device", "k_raster_rows", cloud_scene, device=True),
    # k_raster's small scene without host records: the device counts the triangles, so the frame is binned
    _extra("x_small_device", "k_raster_rows", cloud_scene, device=True, **SMALL, width=171, height=107),
    # the scene of k_raster_rows_rl in the other arithmetic
    _extra("x_lit_exact", "k_raster_rows", cloud_scene, env={"RXR_LIGHT_MATH": "exact"}, lights=5),
    # a light beyond the 1e9 window: the FRAME demotes itself to the exact kernel (rxr_upload.hip), not the context
    _extra("x_huge_light", "k_raster_rows", cloud_scene, lights=5, huge_light=True),
    # count / scan / fill: `parity` flips
    _extra("x_blockscan_off", "k_raster_rows", cloud_scene, env={"RXR_BLOCKSCAN": "0"}),
    # the binned 2D pass through k_blockscan2d
    _extra("x_tilemap2d", "k_raster", scenes.tile_map_2d_scene, width=333, height=211, nx=17, ny=11),
    # 2D count / scan / fill: `parity2d` flips
    _extra("x_tilemap2d_general", "k_raster", scenes.tile_map_2d_scene, env={"RXR_BLOCKSCAN2D": "0"}, width=333, height=211, nx=17, ny=11),
    # the 2D bins overflow, the frame is rendered again and the shape is remembered (blockscan2d_bad)
    _extra("x_stacked2d", "k_raster", scenes.tile_map_2d_scene, may_rerender=True, stacked=600, nx=12, ny=8),
    # every buffer grows: the smaller frames that follow lie in front of this one's bytes
    _extra("x_map_room", "k_raster_rl", scenes.map_scene, width=640, height=400, logo_size=64, n_lights=2),
    # two tiles
    _extra("x_cube_two_tiles", "k_raster", scenes.cube_scene, width=17, height=15, tile_size=40, textured=True),
]
STATES = _route_states() + EXTRAS
BY_NAME = {s.name: s for s in STATES}
NAMES = [s.name for s in STATES]


def schedule(first):
    """the states test_walk_from(first) draws, in order: `first` twice (the pair (first, first)), then every other state of the table, each
    behind `first`"""
    order = [first, first]
    for name in NAMES:
        if name != first:
            order += [name] if order[-1] == first else [first, name]
    return order


# ---- without a GPU --------------------------------------------------------------------------------------------------------------
def test_state_names_are_unique():
    assert len(set(NAMES)) == len(NAMES) == 31, NAMES


def test_the_state_table_has_every_route_but_the_fused_one():
    """a new route cannot silently drop out: the only one left out is the one that needs RXR_SMALL_MODE at rxr_create"""
    assert EXCLUDED == {"k_raster_fused"}
    assert set(ROUTES) - set(NAMES) == EXCLUDED
    for name in set(ROUTES) - EXCLUDED:
        s, r = BY_NAME[name], ROUTES[name]
        assert s.kernel == name and s.env is r["env"] and s.build is r["build"] and not s.device and not s.may_rerender
    assert [s.name for s in STATES if s.may_rerender] == ["x_stacked2d"]
    assert {s.name: s.jit for s in STATES if s.jit is not None} == {
        "k_raster_vm": "0", "k_raster_vm_s": "0", "k_raster_vm_sv": "0", "k_raster_vm_p": "0", "k_raster_vm_v": "0", "k_raster_jit": "1", "k_raster_jit_cut": "1"}


def test_the_schedule_alone_covers_every_ordered_pair():
    pairs = set()
    for first in NAMES:
        order = schedule(first)
        assert len(order) == 2 * len(NAMES) - 1 and set(order) == set(NAMES)
        pairs.update(zip(order, order[1:]))   # (pairs across the end of one test and the start of the next are not counted)
    assert pairs == {(a, b) for a in NAMES for b in NAMES}, f"{len(pairs)} of {len(NAMES) ** 2} ordered pairs"


def test_states_the_mutations_rely_on_differ(oracle):
    """On the oracle's frames.  A context that kept a predecessor's textures must change the frame: the cut-out scene with the textures of
    its twin without holes (and the other way round), and the sparse scene with the cloud's, differ from their own frames -- the texels
    that differ are on screen.  And the exact-lit state is the relaxed-lit route's scene: a context demoted for good would draw
    k_raster_rows_rl's frame with x_lit_exact's kernel."""
    def with_assets_of(name, other):
        cfg, donor = BY_NAME[name].build(oracle), BY_NAME[other].build(oracle)
        cfg.assets = donor.assets
        return scenes.render(cfg).copy()

    solid, holes, sparse = "k_raster_rows", "k_raster_pair", "k_raster_rows_sp"
    assert ROUTES[holes]["kw"].get("holes") and not ROUTES[solid]["kw"].get("holes")
    for name, other in ((holes, solid), (solid, holes), (sparse, solid)):
        own = _oracle_frame(name)
        changed = (with_assets_of(name, other) != own).any(axis=2).mean()
        assert changed > 0.01, f"{name} with the textures of {other}: {changed:.2%} of the pixels change"
    exact, relaxed = BY_NAME["x_lit_exact"], ROUTES["k_raster_rows_rl"]
    assert exact.build.func is relaxed["build"].func and exact.build.keywords == relaxed["kw"] and not relaxed["env"]
    assert np.array_equal(scenes.render(exact.build(oracle)), _oracle_frame("k_raster_rows_rl"))
    lit = (_oracle_frame("k_raster_rows_rl") != _oracle_frame("k_raster_rows")).any(axis=2).mean()
    assert lit > 0.01, "the lights change nothing"


# ---- on the GPU -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cfg_of(name):
    """the state's scene, built once per process and reused on every visit"""
    return BY_NAME[name].build(rusterix_amd.load())


def rerenders(product):
    return rusterix_amd.rxr_abi().rxr_debug_rerenders(C.c_void_p(product.lib.rxh_context()))


def jit_info(product):
    return rusterix_amd.rxr_abi().rxr_debug_jit_info(C.c_void_p(product.lib.rxh_context())).decode()


VISITS = collections.Counter()   # per process, as g_code_objects of rxr_jit.hip is


@contextlib.contextmanager
def visiting(product, monkeypatch, s):
    """the state's variables and projection mode for one frame; RXR_LIGHT_MATH is deleted for every state that does not set it"""
    with knobs(product, monkeypatch, s.env), monkeypatch.context() as m:
        if "RXR_LIGHT_MATH" not in s.env:
            m.delenv("RXR_LIGHT_MATH", raising=False)
        product.lib.rxh_set_device_projection(1 if s.device else 0)
        try:
            yield
        finally:
            product.lib.rxh_set_device_projection(0)


def assert_same_bytes(got, ref, what):
    if np.array_equal(got, ref):
        return
    d = np.argwhere((got != ref).any(axis=2))
    y, x = d[0]
    raise AssertionError(f"{what}: {len(d)} pixels differ from the frame of a fresh context; first at (x={x}, y={y}): got {got[y, x].tolist()}, "
                         f"fresh {ref[y, x].tolist()}")


def assert_jit_info(product, s, what):
    info = jit_info(product)
    if s.jit == "0":
        assert info == "", f"{what}: interpreted, but the run-time compiler says {info!r}"
    elif s.jit == "1":
        assert info.startswith("compiled:"), f"{what}: {info!r}"
        assert VISITS[s.name] == 1 or "(cached)" in info, f"{what}: visit {VISITS[s.name]} compiled the set again: {info!r}"


def visit(product, monkeypatch, s, what, ref=None):
    """draws the state's frame on the context as it is; every check of the visit is made before any of them fails the test, so that one
    message says all that is wrong with the frame (bytes against `ref`, kernel, scratch, silent re-render, run-time compiler)"""
    from tests.test_gpu_sparse_frames import assert_scratch_clean

    wrong = []

    def check(assertion, *args):
        try:
            assertion(*args)
        except AssertionError as e:
            wrong.append(str(e))

    with visiting(product, monkeypatch, s):
        before = rerenders(product)
        frame = scenes.render(cfg_of(s.name)).copy()
        VISITS[s.name] += 1
        if ref is not None:
            check(assert_same_bytes, frame, ref, what)
        check(assert_route, product, s.kernel, what)
        check(assert_scratch_clean, product, what)
        again = rerenders(product) - before
        if again and not s.may_rerender:
            wrong.append(f"{what}: the frame was rendered {again} more time(s) behind the caller's back (rxr_debug_rerenders)")
        check(assert_jit_info, product, s, what)
    assert not wrong, "\n".join(wrong)
    return frame


@pytest.fixture(scope="module")
def reference_frames(product):
    """every state drawn once by a context that has drawn nothing else"""
    frames = {}
    with pytest.MonkeyPatch.context() as monkeypatch:
        try:
            for s in STATES:
                _recreate_context(product)
                frames[s.name] = visit(product, monkeypatch, s, f"fresh context -> {s.name}")
                frames[s.name].setflags(write=False)
        finally:
            _recreate_context(product)
    return frames


@gpu
@pytest.mark.parametrize("first", NAMES)
def test_walk_from(product, monkeypatch, reference_frames, first):
    previous = "(the context as the test found it)"
    for name in schedule(first):
        visit(product, monkeypatch, BY_NAME[name], f"{previous} -> {name}", reference_frames[name])
        previous = name
