"""The ray box tree's cull without a device (tests/ray_accel_ref.py restates rxr_ray_accel.hip's box test, wild rule and walk in numpy
float32): the shipped pad keeps every hit the committed adversarial generator produces, with a factor of four to spare; triangles
without a usable box are wild; rays the walk drops are rays every triangle test rejects; the stackless walk enters every leaf
exactly once when every box passes and only the root when none does."""
import re
from pathlib import Path

import numpy as np
import pytest

from tests import intersect_ref as R
from tests import ray_accel_ref as A

F = np.float32
ROOT = Path(__file__).resolve().parent.parent


def test_constants_are_the_headers_and_the_recorded_measurement():
    assert (A.LEAF, A.WIDTH, A.KAPPA_CAP) == (8, 8, 4096.0)
    c = A.C_SHIPPED
    assert c >= 1 and c == 2.0 ** round(np.log2(c))      # a power of two
    text = (ROOT / "profiles" / "ray_accel" / "README.md").read_text()
    measured = float(re.search(r"smallest C at which no accepted pair is culled: \*\*([0-9.]+)\*\*", text).group(1))
    shipped = float(re.search(r"shipped `RXR_RAY_ACCEL_C`: \*\*([0-9.]+)\*\*", text).group(1))
    assert shipped == c and shipped == 8 * measured


def test_mt_pairs_is_intersect_refs_mt():
    P = A.adversarial_pairs(5, 500)
    p0, e1, e2 = A.records(P["v0"], P["v1"], P["v2"])
    ok, t = A.mt_pairs(P["o"], P["d"], p0, e1, e2)
    for i in range(0, len(ok), 7):
        ok1, t1, _, _ = R.mt(P["o"][i], P["d"][i], p0[i:i + 1], e1[i:i + 1], e2[i:i + 1])
        assert bool(ok1[0]) == bool(ok[i]) and R.same(t1, t[i:i + 1])


def test_a_quarter_of_the_shipped_pad_culls_no_accepted_hit():
    """seeds that the measurement of profiles/ray_accel/README.md did not draw"""
    hits = 0
    per_kind = {k: 0 for k in A.KINDS}
    for seed in (1001, 1002, 1003):
        P = A.adversarial_pairs(seed, 50000)
        bad, acc = A.culled(P, A.C_SHIPPED / 4)
        for ki, k in enumerate(A.KINDS):
            per_kind[k] += int(acc[P["kind"] == ki].sum())
        assert not bad.any(), f"seed {seed}: {int(bad.sum())} accepted hits culled, the first of kind {A.KINDS[P['kind'][np.nonzero(bad)[0][0]]]}"
        hits += int(acc.sum())
    assert hits >= 200_000, hits
    assert min(per_kind.values()) >= 20_000, per_kind      # every kind takes part


def test_the_generator_is_adversarial():
    """without a pad the exact box culls accepted hits of every kind but the axis-aligned one: the pad is needed"""
    P = A.adversarial_pairs(1001, 50000)
    bad, _ = A.culled(P, 0.0)
    kinds = {A.KINDS[k] for k in np.unique(P["kind"][bad])}
    assert {"sliver", "random_box", "random_edges"} <= kinds


def test_wild_classification():
    v0 = np.zeros((8, 3), F)
    v1 = np.tile(np.array([1, 0, 0], F), (8, 1))
    v2 = np.tile(np.array([0, 1, 0], F), (8, 1))
    v1[1, 0] = np.nan                      # a NaN vertex
    v2[2, 1] = np.inf                      # an infinite one
    v0[3] = (3e38, 0, 0)
    v1[3] = (-3e38, 0, 0)                  # finite vertices, an edge that overflows
    v2[4] = v1[4]                          # zero area: 0 / 0
    v2[5] = (2, 0, 0)                      # zero area, collinear
    v2[6] = (1, 1.0 / 4100, 0)             # kappa just above the cap ...
    v2[7] = (0, 1.0 / 4095, 0)             # ... and a thin but well-conditioned right triangle (kappa 1)
    p0, e1, e2 = A.records(v0, v1, v2)
    assert A.wild(p0, e1, e2).tolist() == [False, True, True, True, True, True, True, False]
    k = A.kappa(e1[6:7], e2[6:7])[0]
    assert 4096 < k < 4200
    # at the cap itself a triangle is still tame: kappa <= cap
    e = np.array([[1, 0, 0]], F)
    assert not A.wild(np.zeros((1, 3), F), e, np.array([[1, 1, 0]], F), cap=float(A.kappa(e, np.array([[1, 1, 0]], F))[0]))[0]
    assert A.wild(np.zeros((1, 3), F), e, np.array([[1, 1, 0]], F), cap=1.0)[0]


def test_a_wild_node_always_passes_and_a_dead_ray_hits_nothing():
    inf = F(np.inf)
    o = np.array([[5, 5, 5]], F)
    d = R.normalized(np.array([[1, 1, 1]], F))
    assert A.box_pass(np.full((1, 3), -inf), np.full((1, 3), inf), F(1), inf, o, d)[0]
    # a box behind the ray, then ahead of it
    lo, hi = np.array([[0, 0, 0]], F), np.array([[1, 1, 1]], F)
    assert not A.box_pass(lo, hi, F(1.2), F(1), o, d)[0]
    assert A.box_pass(lo, hi, F(1.2), F(1), o, -d)[0]
    # a zero component of the direction: the slab it is inside of does not constrain it
    assert A.box_pass(lo, hi, F(1.2), F(1), np.array([[0.5, 0.5, -3]], F), np.array([[0, 0, 1]], F))[0]
    assert not A.box_pass(lo, hi, F(1.2), F(1), np.array([[1.5, 0.5, -3]], F), np.array([[0, 0, 1]], F))[0]


def test_rays_the_walk_drops_are_rejected_by_every_triangle():
    rng = np.random.default_rng(3)
    P = A.adversarial_pairs(9, 2000)
    p0, e1, e2 = A.records(P["v0"], P["v1"], P["v2"])
    specials = [np.nan, np.inf, -np.inf]
    rays = []
    for i in range(3):
        for s in specials:
            o, d = np.array([0.3, 0.2, -4.0], F), np.array([0.1, 0.2, 1.0], F)
            o[i] = s
            rays.append((o, np.array([0.1, 0.2, 1.0], F)))
            d[i] = s
            rays.append((np.array([0.3, 0.2, -4.0], F), d))
    rays.append((np.array([0.3, 0.2, -4.0], F), np.zeros(3, F)))                  # zero direction
    rays.append((np.array([0.3, 0.2, -4.0], F), np.array([1e-40, 0, 1e-40], F)))  # its length underflows
    rays.append((np.array([0.3, 0.2, -4.0], F), np.array([1e-30, 1e-30, 1e-30], F)))
    rays.append((np.array([0.3, 0.2, -4.0], F), np.array([3e38, 3e38, 0], F)))    # its length overflows
    n_dead = 0
    for o, dir_ in rays:
        with np.errstate(all="ignore"):
            d = R.normalized(dir_)
        if not A.ray_dead(o, d):
            continue
        n_dead += 1
        ok, _, _, _ = R.mt(o, d, p0, e1, e2)
        assert not ok.any(), (o, dir_)
        # ... and against triangles aimed at: the unit quad's, hit squarely by the finite part of the ray
        q0 = np.array([[0, 0, 0]], F)
        ok, _, _, _ = R.mt(o, d, q0, np.array([[1, 0, 0]], F), np.array([[0, 1, 0]], F))
        assert not ok.any()
    assert n_dead >= 20
    del rng


COUNTS = (1, A.LEAF - 1, A.LEAF, A.LEAF + 1, A.LEAF * A.WIDTH - 1, A.LEAF * A.WIDTH, A.LEAF * A.WIDTH + 1, A.LEAF * A.WIDTH ** 2 + 1)


@pytest.mark.parametrize("ntri", COUNTS + (5000, 12288))
@pytest.mark.parametrize("leaf,width", [(A.LEAF, A.WIDTH), (4, 4), (16, 16), (3, 5)])
def test_the_walk_enters_every_leaf_once_when_every_box_passes(ntri, leaf, width):
    cnt = A.levels(ntri, leaf, width)
    assert cnt[-1] == 1 and cnt[0] == -(-ntri // leaf)
    entered, tested = A.walk(ntri, lambda level, idx: True, leaf, width)
    assert entered == list(range(cnt[0]))
    assert len(tested) == len(set(tested)) == sum(cnt)          # every node once


@pytest.mark.parametrize("ntri", COUNTS)
def test_the_walk_tests_only_the_root_when_nothing_passes(ntri):
    entered, tested = A.walk(ntri, lambda level, idx: False)
    assert entered == [] and tested == [(len(A.levels(ntri)) - 1, 0)]


@pytest.mark.parametrize("seed", range(6))
def test_the_walk_enters_exactly_the_leaves_whose_ancestors_all_pass(seed):
    rng = np.random.default_rng(seed)
    ntri = int(rng.integers(1, 6000))
    cnt = A.levels(ntri)
    ok = [rng.random(c) < 0.7 for c in cnt]
    entered, tested = A.walk(ntri, lambda level, idx: bool(ok[level][idx]))
    want = []
    for leaf in range(cnt[0]):
        idx, good = leaf, True
        for level in range(len(cnt)):
            good &= bool(ok[level][idx])
            idx //= A.WIDTH
        if good:
            want.append(leaf)
    assert entered == want
    assert len(tested) <= sum(cnt) and len(tested) == len(set(tested))
    # the position only moves forward: leaves-first order of the nodes' first positions never decreases
    first = [idx * A.LEAF * A.WIDTH ** level for level, idx in tested]
    assert first == sorted(first)
