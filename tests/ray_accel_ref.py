"""numpy float32 restatement of the box tree's cull (rusterix_amd/csrc/rxr_ray_accel.hip): the padded slab test `box_pass`, the wild
rule, the implicit tree's levels and its stackless walk -- and the adversarial generator that decides the pad's constant C.

The tree may skip a triangle only if Batch3D::intersect's float32 test (tests/intersect_ref.py: mt) rejects the ray.  That test
accepts rays whose line misses a thin triangle's exact box by far, so the box is grown by

    pad = C * eps32 * kappa * (max|o_i| + max|box coordinate|),      kappa = |e1| |e2| / |e1 x e2|  (the largest below the node)

`measure_C` finds the smallest power of two C at which no accepted (ray, triangle) pair of `adversarial_pairs` is culled by that
triangle's own box; the library ships 8 x that (RXR_RAY_ACCEL_C, rxr_isect.h).  tools/ray_accel_margin.py runs the measurement;
profiles/ray_accel/README.md records it.  Every operation below is one IEEE float32 operation in the device's order."""
import re
from pathlib import Path

import numpy as np

from tests import intersect_ref as R

F = np.float32
EPS32 = F(2.0 ** -23)
INF = F(np.inf)


def _header_constants():
    text = (Path(__file__).resolve().parent.parent / "rusterix_amd" / "csrc" / "rxr_isect.h").read_text()
    get = lambda name: re.search(r"#define\s+" + name + r"\s+([0-9.]+)", text).group(1)
    return int(get("RXR_RAY_ACCEL_LEAF")), int(get("RXR_RAY_ACCEL_WIDTH")), float(get("RXR_RAY_ACCEL_KAPPA_CAP")), float(get("RXR_RAY_ACCEL_C"))


LEAF, WIDTH, KAPPA_CAP, C_SHIPPED = _header_constants()


# ---- the triangle's side -----------------------------------------------------------------------------------------------------------
def records(v0, v1, v2):
    """(p0, e1, e2) as k_isect_prep writes them: [n][3] float32 each"""
    v0, v1, v2 = (np.asarray(x, F) for x in (v0, v1, v2))
    with np.errstate(all="ignore"):
        return v0, v1 - v0, v2 - v0


def kappa(e1, e2):
    with np.errstate(all="ignore"):
        n = R.cross(e1, e2)
        return (np.sqrt(R.dot(e1, e1)) * np.sqrt(R.dot(e2, e2))) / np.sqrt(R.dot(n, n))


def wild(p0, e1, e2, cap=KAPPA_CAP):
    """always tested: a value of the record is not finite, or kappa is not finite or above the cap"""
    fin = np.isfinite(p0).all(axis=-1) & np.isfinite(e1).all(axis=-1) & np.isfinite(e2).all(axis=-1)
    with np.errstate(all="ignore"):
        return ~fin | ~(kappa(e1, e2) <= F(cap))


def own_box(v0, v1, v2):
    """(lo, hi, maxabs) of one triangle's vertices, as a leaf of one triangle would hold them"""
    lo = np.fmin(np.fmin(v0, v1), v2)
    hi = np.fmax(np.fmax(v0, v1), v2)
    return lo, hi, np.fmax(np.abs(lo), np.abs(hi)).max(axis=-1)


# ---- the ray's side ----------------------------------------------------------------------------------------------------------------
def ray_dead(o, d):
    """a ray the walk drops outright: a component of the origin or of the NORMALISED direction is not finite"""
    return ~(np.isfinite(o).all(axis=-1) & np.isfinite(d).all(axis=-1))


def box_pass(lo, hi, kap, maxabs, o, d, C=C_SHIPPED):
    """the device's box_pass, elementwise over [n] nodes and [n] rays (d normalised): True = enter the node"""
    lo, hi, o, d = (np.asarray(x, F) for x in (lo, hi, o, d))
    kap, maxabs = np.asarray(kap, F), np.asarray(maxabs, F)
    with np.errstate(all="ignore"):
        inv = F(1.0) / d
        omax = np.fmax(np.fmax(np.abs(o[..., 0]), np.abs(o[..., 1])), np.abs(o[..., 2]))
        pad = ((F(C) * EPS32) * kap) * (omax + maxabs)
        tn = np.full(pad.shape, -INF, F)
        tf = np.full(pad.shape, INF, F)
        for i in range(3):
            a = ((lo[..., i] - pad) - o[..., i]) * inv[..., i]
            b = ((hi[..., i] + pad) - o[..., i]) * inv[..., i]
            tn = np.fmax(tn, np.fmin(a, b))
            tf = np.fmin(tf, np.fmax(a, b))
        return ~(maxabs < INF) | ((tn <= tf) & (tf >= F(0.0)))


def mt_pairs(o, d, p0, e1, e2):
    """intersect_ref.mt, ray i against triangle i: (accepted, t)"""
    with np.errstate(all="ignore"):
        h = R.cross(d, e2)
        a = R.dot(e1, h)
        ok = ~(np.abs(a) < F(1e-6))
        f = F(1.0) / a
        s = o - p0
        u = f * R.dot(s, h)
        ok &= (u >= F(0.0)) & (u <= F(1.0))
        q = R.cross(s, e1)
        v = f * R.dot(d, q)
        ok &= ~((v < F(0.0)) | (u + v > F(1.0)))
        t = f * R.dot(e2, q)
        ok &= t > F(1e-4)
    return ok, t


# ---- the adversarial generator -----------------------------------------------------------------------------------------------------
KINDS = ("axis_right", "sliver", "random_box", "random_edges")


def _unit(rng, n):
    v = rng.standard_normal((n, 3))
    return v / np.linalg.norm(v, axis=1)[:, None]


def triangles(rng, n, kind):
    """n triangles of one kind: (v0, v1, v2) float32.  Sizes 1e-3 .. 1e3, centres up to 1e3 away from the world's origin."""
    size = 10.0 ** rng.uniform(-3, 3, n)
    centre = rng.standard_normal((n, 3)) * (10.0 ** rng.uniform(-1, 3, n))[:, None]
    if kind == "axis_right":
        a = rng.integers(0, 3, n)
        b = (a + rng.integers(1, 3, n)) % 3   # (another axis)
        e1 = np.zeros((n, 3))
        e2 = np.zeros((n, 3))
        e1[np.arange(n), a] = size * rng.choice([-1.0, 1.0], n)
        e2[np.arange(n), b] = size * rng.uniform(0.25, 1.0, n) * rng.choice([-1.0, 1.0], n)
    elif kind == "sliver":
        u = _unit(rng, n)
        w = np.cross(u, _unit(rng, n))
        w /= np.linalg.norm(w, axis=1)[:, None]
        e1 = u * size[:, None]
        e2 = u * (size * rng.uniform(0.05, 0.95, n))[:, None] + w * (size * 10.0 ** rng.uniform(-4, -1.5, n))[:, None]
    elif kind == "random_box":
        e1 = rng.uniform(-1, 1, (n, 3)) * size[:, None]
        e2 = rng.uniform(-1, 1, (n, 3)) * size[:, None]
    elif kind == "random_edges":
        e1 = rng.standard_normal((n, 3)) * size[:, None]
        e2 = rng.standard_normal((n, 3)) * (size * 10.0 ** rng.uniform(-1.5, 1.5, n))[:, None]
    else:
        raise ValueError(kind)
    v0 = centre.astype(F)
    return v0, (centre + e1).astype(F), (centre + e2).astype(F)


def aimed_rays(rng, v0, v1, v2, graze_share=0.5):
    """one ray per triangle, from 1e-2 .. 1e5 away, through a vertex, a point on an edge, a point just off an edge or an inner point;
    `graze_share` of them graze the plane: the
    direction's component along the normal is 1e-5 .. 0.3 of its length"""
    n = len(v0)
    V = np.stack([v0, v1, v2], axis=1).astype(np.float64)
    what = rng.integers(0, 4, n)
    i = rng.integers(0, 3, n)
    a, b, c = V[np.arange(n), i], V[np.arange(n), (i + 1) % 3], V[np.arange(n), (i + 2) % 3]
    s = rng.uniform(0, 1, n)[:, None]
    edge = a + (b - a) * s
    inner = edge + (c - edge) * rng.uniform(0, 1, n)[:, None]
    off = edge + (c - edge) * (rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-7, -3, n))[:, None]
    target = np.where((what == 0)[:, None], a, np.where((what == 1)[:, None], edge, np.where((what == 2)[:, None], off, inner)))
    dist = 10.0 ** rng.uniform(-2, 5, n)
    # half of the rays at a random incidence, half grazing the triangle's plane (where the test's 1 / a amplifies its rounding most)
    way = _unit(rng, n)
    nrm = np.cross(V[:, 1] - V[:, 0], V[:, 2] - V[:, 0])
    nlen = np.linalg.norm(nrm, axis=1)
    graze = (rng.uniform(0, 1, n) < graze_share) & (nlen > 0)
    nrm = nrm / np.where(nlen > 0, nlen, 1.0)[:, None]
    flat = way - nrm * np.sum(way * nrm, axis=1)[:, None]
    flat /= np.maximum(np.linalg.norm(flat, axis=1), 1e-300)[:, None]
    lift = (rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-5, -0.5, n))[:, None]
    way = np.where(graze[:, None], flat + nrm * lift, way)
    way /= np.maximum(np.linalg.norm(way, axis=1), 1e-300)[:, None]
    o = (target + way * dist[:, None]).astype(F)
    d = target.astype(F) - o
    return o, d


def adversarial_pairs(seed, n_per_kind, graze_share=0.5):
    """the committed generator: for each kind n_per_kind (ray, triangle) pairs.  Returns a dict of float32 arrays: v0, v1, v2, o and the
    NORMALISED d, plus `kind` (index into KINDS)."""
    rng = np.random.default_rng(seed)
    out = {k: [] for k in ("v0", "v1", "v2", "o", "d", "kind")}
    for ki, kind in enumerate(KINDS):
        v0, v1, v2 = triangles(rng, n_per_kind, kind)
        o, d = aimed_rays(rng, v0, v1, v2, graze_share)
        with np.errstate(all="ignore"):
            d = R.normalized(d)
        for k, x in zip(("v0", "v1", "v2", "o", "d"), (v0, v1, v2, o, d)):
            out[k].append(x)
        out["kind"].append(np.full(n_per_kind, ki))
    return {k: np.concatenate(v) for k, v in out.items()}


def accepted_tame(P):
    """(mask of the pairs mt accepts whose triangle is not wild, p0, e1, e2)"""
    p0, e1, e2 = records(P["v0"], P["v1"], P["v2"])
    ok, _ = mt_pairs(P["o"], P["d"], p0, e1, e2)
    return ok & ~wild(p0, e1, e2), p0, e1, e2


def culled(P, C):
    """mask of accepted, tame pairs that the triangle's own box would cull at the constant C"""
    acc, p0, e1, e2 = accepted_tame(P)
    lo, hi, maxabs = own_box(P["v0"], P["v1"], P["v2"])
    return acc & ~box_pass(lo, hi, kappa(e1, e2), maxabs, P["o"], P["d"], C), acc


def measure_C(seeds, n_per_kind, powers=range(-8, 24), graze_share=0.5):
    """(smallest power of two C that culls no accepted pair, accepted hits, {kind: its smallest C})"""
    need = {k: 2.0 ** min(powers) for k in KINDS}
    hits = 0
    for seed in seeds:
        P = adversarial_pairs(seed, n_per_kind, graze_share)
        acc = None
        for p in powers:
            bad, acc = culled(P, 2.0 ** p)
            if not bad.any():
                break
            for ki, k in enumerate(KINDS):
                if bad[P["kind"] == ki].any():
                    need[k] = max(need[k], 2.0 ** (p + 1))
        hits += int(acc.sum())
    return max(need.values()), hits, need


# ---- the implicit tree -------------------------------------------------------------------------------------------------------------
def levels(ntri, leaf=LEAF, width=WIDTH):
    """nodes per level, leaves first, up to one root"""
    cnt = [(ntri + leaf - 1) // leaf]
    while cnt[-1] > 1:
        cnt.append((cnt[-1] + width - 1) // width)
    return cnt


def walk(ntri, passes, leaf=LEAF, width=WIDTH):
    """k_accel_by_ray's walk: passes(level, index) -> bool.  Returns (leaves entered, nodes tested), both in visiting order."""
    cnt = levels(ntri, leaf, width)
    top = len(cnt) - 1
    level, idx = top, 0
    entered, tested = [], []
    while True:
        assert 0 <= idx < cnt[level]
        tested.append((level, idx))
        ok = passes(level, idx)
        if ok and level > 0:
            level -= 1
            idx *= width
            continue
        if ok:
            entered.append(idx)
        idx += 1
        while level < top and (idx % width == 0 or idx == cnt[level]):
            idx = (idx - 1) // width + 1
            level += 1
        if level == top:
            break
    return entered, tested
