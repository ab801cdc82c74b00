"""The wave walk of the ray box tree without a device (rxr_set_ray_wave; k_accel_by_wave, rusterix_amd/csrc/rxr_ray_accel.hip):
tests/ray_wave_ref.py restates its visit rule, held here to the thread walk's (tests/ray_accel_ref.py: walk) at every tree shape; the
route rule rxr_ray_wave_takes is called in the built library against the header's constants; the ABI carries the three calls."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from tests import intersect_ref as R
from tests import ray_accel_ref as A
from tests import ray_wave_ref as V

F = np.float32
ROOT = Path(__file__).resolve().parent.parent
L, W = A.LEAF, A.WIDTH
NTRI = (1, 7, 8, 9, 63, 64, 65, 511, 512, 513, 4095, 4096, 4097, 32769)


def check_walk(ntri, passes):
    """the properties every walk must have; returns (positions, nodes tested)"""
    cnt = A.levels(ntri)
    positions, tested, steps, deepest = V.wave_walk(ntri, passes)
    for level, idx in tested:
        assert 0 <= level < len(cnt) and 0 <= idx < cnt[level], (level, idx)          # no node index out of its level
    assert len(tested) == len(set(tested))
    assert steps <= sum(cnt) + 1 and deepest <= V.STACK
    assert positions == sorted(positions) and len(positions) == len(set(positions))   # increasing: segment order
    assert all(0 <= p < ntri for p in positions)
    leaves, thread_tested = A.walk(ntri, passes)
    thread = {p for leaf in leaves for p in range(leaf * L, min(leaf * L + L, ntri))}
    assert thread <= set(positions), f"{ntri} triangles: the wave walk skips {sorted(thread - set(positions))[:5]} that the thread walk tests"
    # ... because it tests a subset of the boxes the thread walk may test: the odd levels below the root, never the leaves
    assert all(level % 2 == 1 and level < len(cnt) - 1 for level, _ in tested)
    return positions, tested


def test_tops_zero_to_five_and_both_parities():
    assert sorted({len(A.levels(n)) - 1 for n in NTRI}) == [0, 1, 2, 3, 4, 5]


@pytest.mark.parametrize("ntri", NTRI)
def test_every_box_passes_every_position_once(ntri):
    positions, tested = check_walk(ntri, lambda level, idx: True)
    assert positions == list(range(ntri))


@pytest.mark.parametrize("ntri", NTRI)
def test_no_box_passes(ntri):
    """The shipped rule tests neither the root's box nor (RXR_RAY_WAVE_LEAF_BOXES 0) the leaves', so a tree of one level (one leaf)
    or two (up to 64 triangles) has no box left to test: every position is tested whatever the boxes say.  From three levels on
    nothing is."""
    assert V.LEAF_BOXES is False
    positions, tested = check_walk(ntri, lambda level, idx: False)
    cnt = A.levels(ntri)
    if len(cnt) <= 2:
        assert positions == list(range(ntri)) and tested == []
    else:
        assert positions == []
        top = len(cnt) - 1
        below = top - 1 if top % 2 == 0 else top - 2     # an even top takes one level first
        assert tested == [(below, i) for i in range(cnt[below])]


@pytest.mark.parametrize("ntri", NTRI)
@pytest.mark.parametrize("seed,share", [(0, 0.7), (1, 0.95), (2, 0.3)])
def test_seeded_coins(ntri, seed, share):
    rng = np.random.default_rng(1000 * seed + ntri)
    ok = [rng.random(c) < share for c in A.levels(ntri)]
    positions, _ = check_walk(ntri, lambda level, idx: bool(ok[level][idx]))
    # exactly the positions whose tested ancestors all pass
    cnt = A.levels(ntri)
    top = len(cnt) - 1
    levels_tested = [l for l in range(1, top) if l % 2 == 1]
    want = [p for p in range(ntri) if all(ok[l][p // (L * W ** l)] for l in levels_tested)]
    assert positions == want


@pytest.mark.parametrize("ntri", NTRI[:-1] + (6000,))
def test_box_pass_over_the_adversarial_generators_scenes(ntri):
    """the passes come from the shipped box test over a tree of the generator's triangles, for rays aimed at them and rays anywhere"""
    rng = np.random.default_rng(ntri)
    per = -(-ntri // len(A.KINDS))
    tri = [A.triangles(rng, per, kind) for kind in A.KINDS]
    v0, v1, v2 = (np.concatenate([t[k] for t in tri])[:ntri] for k in range(3))
    # (any order does for the duty; sorting by a centroid coordinate gives boxes that cull)
    order = np.argsort((v0[:, 0] + v1[:, 0] + v2[:, 0]), kind="stable")
    v0, v1, v2 = v0[order], v1[order], v2[order]
    nodes = V.build_nodes(v0, v1, v2)
    assert [len(lv["kappa"]) for lv in nodes] == A.levels(ntri)
    pick = rng.integers(0, ntri, 6)
    o, d = A.aimed_rays(rng, v0[pick], v1[pick], v2[pick])
    o = np.concatenate([o, rng.standard_normal((2, 3)).astype(F) * F(50)])
    d = np.concatenate([d, rng.standard_normal((2, 3)).astype(F)])
    with np.errstate(all="ignore"):
        d = R.normalized(d)
    p0, e1, e2 = A.records(v0, v1, v2)
    culled = 0
    for r in range(len(o)):
        if A.ray_dead(o[r], d[r]):
            continue
        positions, _ = check_walk(ntri, V.passes_of(nodes, o[r], d[r]))
        culled += ntri - len(positions)
        # the duty itself, on this scene: what mt accepts is among the positions tested
        ok, _, _, _ = R.mt(o[r], d[r], p0, e1, e2)
        assert set(np.nonzero(ok)[0].tolist()) <= set(positions)
    if ntri >= 4095:
        assert culled > 0


# ---- the route rule ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def takes():
    from rusterix_amd import libs

    fn = libs.rxr_abi().rxr_ray_wave_takes
    return lambda n_rays, n_triangles: int(fn(n_rays, n_triangles))


RAYS = (0, 1, 2, 7, 8, 9, 63, 64, 65, 255, 256, 1023, 1024, 4095, 4096, 4097, 16383, 16384, 16385, 65535, 65536, 1920 * 1080, 2 ** 32 - 1)
TRIS = (0, 1, 12, 2255, 2256, 2257, 12288, 100000, 524288, 1048576, 2 ** 24, 2 ** 32 - 1)


def test_the_rule_is_the_closed_form_over_the_headers_constants(takes):
    lo, hi, triangles = V.route_constants()
    assert 1 < lo <= hi and triangles > 2256             # a single click and the teapot's scene are outside whatever else holds
    for n in RAYS + (lo - 1, lo, hi, hi + 1):
        for t in TRIS + (triangles - 1, triangles, triangles + 1):
            assert takes(n, t) == int(V.takes(n, t)) and takes(n, t) in (0, 1), (n, t)
    assert takes(lo, triangles) == 1 and takes(hi, 2 ** 32 - 1) == 1


def test_the_rule_is_monotone_in_the_triangles_and_an_interval_in_the_rays(takes):
    for n in RAYS:
        col = [takes(n, t) for t in TRIS]
        assert col == sorted(col), (n, col)              # more triangles never leave the route
    for t in TRIS:
        row = [takes(n, t) for n in RAYS]
        on = [i for i, x in enumerate(row) if x]
        assert not on or on == list(range(on[0], on[-1] + 1)), (t, row)   # one interval of ray counts


def test_a_single_click_and_small_scenes_stay_on_the_existing_routes(takes):
    for t in TRIS:
        assert takes(1, t) == 0 and takes(0, t) == 0
    for n in RAYS:
        assert takes(n, 2256) == 0 and takes(n, 0) == 0


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------
def test_the_abi_carries_the_three_calls_at_version_5():
    from rusterix_amd import abi

    hdr = (ROOT / "include" / "rxr.h").read_text()
    ffi = (ROOT / "shim" / "rusterix-hip-shim" / "src" / "ffi.rs").read_text()
    assert re.search(r"#define RXR_ABI_VERSION 5u", hdr) and re.search(r"RXR_ABI_VERSION: u32 = 5;", ffi) and abi.RXR_ABI_VERSION == 5
    for name in ("rxr_set_ray_wave", "rxr_ray_wave_takes", "rxr_ray_wave_info"):
        assert re.search(r"\bint " + name + r"\(", hdr), name
        assert re.search(r"pub fn " + name + r"\(", ffi), name
        assert name in abi.SIGNATURES, name
    assert (abi.RXR_RAY_WAVE_OFF, abi.RXR_RAY_WAVE_ON, abi.RXR_RAY_WAVE_FORCE) == (0, 1, 2)
    assert (abi.RXR_RAY_WAVE_INFO_MODE, abi.RXR_RAY_WAVE_INFO_BATCHES, abi.RXR_RAY_WAVE_INFO_RAYS, abi.RXR_RAY_WAVE_INFO_WORDS) == (0, 1, 2, 3)
    assert abi.SIGNATURES["rxr_ray_wave_takes"] == (C.c_int, [C.c_uint32, C.c_uint32])
    assert "pub fn set_ray_wave(" in (ROOT / "shim" / "rusterix-hip-shim" / "src" / "lib.rs").read_text()
    from rusterix_amd import binding, trace
    for mod in (binding, trace):
        assert (mod.RAY_WAVE_OFF, mod.RAY_WAVE_ON, mod.RAY_WAVE_FORCE) == (0, 1, 2) and len(mod.RAY_WAVE_INFO) == abi.RXR_RAY_WAVE_INFO_WORDS
