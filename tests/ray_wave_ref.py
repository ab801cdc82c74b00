"""Restatement of the wave walk's visit rule (k_accel_by_wave, rusterix_amd/csrc/rxr_ray_accel.hip) over the
implicit levels of tests/ray_accel_ref.py, and the constants of its route rule (rxr_ray_wave_takes, rxr_isect.h).

A wave walks one ray.  Entering node (l, i):
    l odd, >= 3    the 64 nodes i * 64 .. of level l - 2 (clipped to that level) are tested; the passing ones are a frame, entered lowest
                   first
    l even, >= 2   (only the root of a tree whose top level is even) one level: the 8 children i * 8 .. of level l - 1
    l == 1         the node's sorted positions [i * 64, min(i * 64 + 64, ntri)) are tested
    l == 0         (a tree of one leaf) its up to 8 positions
The root's box is never tested, and -- the shipped choice, LEAF_BOXES False -- neither are the leaves': a tree of one or two levels
tests every position whatever the boxes say."""
import re
from pathlib import Path

import numpy as np

from tests import ray_accel_ref as A

LEAF_BOXES = False   # RXR_RAY_WAVE_LEAF_BOXES of the shipped build
STACK = 12           # ACCEL_WAVE_STACK


def route_constants():
    """(RXR_RAY_WAVE_MIN_RAYS, RXR_RAY_WAVE_MAX_RAYS, RXR_RAY_WAVE_MIN_TRIANGLES) as rxr_isect.h defines them"""
    text = (Path(__file__).resolve().parent.parent / "rusterix_amd" / "csrc" / "rxr_isect.h").read_text()
    get = lambda name: int(re.search(r"#define\s+" + name + r"\s+(\d+)u", text).group(1))
    return get("RXR_RAY_WAVE_MIN_RAYS"), get("RXR_RAY_WAVE_MAX_RAYS"), get("RXR_RAY_WAVE_MIN_TRIANGLES")


def takes(n_rays, n_triangles):
    lo, hi, triangles = route_constants()
    return lo <= n_rays <= hi and n_triangles >= triangles


def wave_walk(ntri, passes, leaf_boxes=LEAF_BOXES):
    """k_accel_by_wave's walk: passes(level, index) -> bool.  Returns (positions tested, nodes tested, steps, deepest stack), the first
    two in visiting order; a step is one entered node."""
    L, W = A.LEAF, A.WIDTH
    cnt = A.levels(ntri)
    top = len(cnt) - 1
    positions, tested = [], []
    steps = deepest = 0
    stack = [(top, 0, [0])]   # frames: (level of the nodes, parent's index, bits still set); the root is a frame of one bit
    while stack:
        deepest = max(deepest, len(stack))
        assert len(stack) <= STACK
        level, pidx, bits = stack[-1]
        if not bits:
            stack.pop()
            continue
        idx = (pidx << 6) + bits.pop(0)
        assert 0 <= idx < cnt[level]
        steps += 1
        if level >= 2:
            down, fan = (2, W * W) if level & 1 else (1, W)
            mask = []
            for j in range(fan):
                c = idx * fan + j
                if c < cnt[level - down]:
                    tested.append((level - down, c))
                    if passes(level - down, c):
                        mask.append(j)
            if mask:
                stack.append((level - down, idx, mask))
            continue
        n = L * W if level else L
        p0, p1 = idx * n, min(idx * n + n, ntri)
        take = list(range(p0, p1))
        if leaf_boxes:
            keep = set()
            for j in range(W if level else 1):
                leaf = p0 // L + j
                if leaf < cnt[0]:
                    tested.append((0, leaf))
                    if passes(0, leaf):
                        keep.add(leaf)
            take = [p for p in take if p // L in keep]
        positions += take
    return positions, tested, steps, deepest


# ---- nodes: from triangles in their sorted order (the build's arithmetic), or from the device's own array ---------------------------
def build_nodes(v0, v1, v2):
    """the levels of the tree over triangles already in sorted order, leaves first: per level a dict of lo, hi [n][3], kappa, maxabs [n]
    (k_accel_leaves / k_accel_level: a wild triangle makes its leaf and every ancestor wild)"""
    F, INF = A.F, A.INF
    p0, e1, e2 = A.records(v0, v1, v2)
    wild = A.wild(p0, e1, e2)
    with np.errstate(all="ignore"):
        kap = A.kappa(e1, e2)
    tlo, thi, _ = A.own_box(*(np.asarray(x, F) for x in (v0, v1, v2)))
    items = dict(lo=tlo, hi=thi, kappa=kap.astype(F), wild=wild)
    out = []
    for group in [A.LEAF] + [A.WIDTH] * (len(A.levels(len(p0))) - 1):
        n = -(-len(items["wild"]) // group)
        lo, hi = np.full((n, 3), INF, F), np.full((n, 3), -INF, F)
        kappa, w = np.zeros(n, F), np.zeros(n, bool)
        for i in range(n):
            sl = slice(i * group, (i + 1) * group)
            tame = ~items["wild"][sl]
            w[i] = items["wild"][sl].any()
            if tame.any():
                lo[i], hi[i] = items["lo"][sl][tame].min(axis=0), items["hi"][sl][tame].max(axis=0)
                kappa[i] = items["kappa"][sl][tame].max()
        maxabs = np.fmax(np.abs(lo), np.abs(hi)).max(axis=1)
        lo[w], hi[w], kappa[w], maxabs[w] = -INF, INF, F(1), INF
        out.append(dict(lo=lo, hi=hi, kappa=kappa, maxabs=maxabs))
        items = dict(lo=lo, hi=hi, kappa=kappa, wild=w)
    return out


def split_nodes(flat, ntri):
    """rxr_debug_ray_accel_nodes' [n][8] floats (lo[3], kappa, hi[3], maxabs) as the levels of build_nodes"""
    out, off = [], 0
    for n in A.levels(ntri):
        x = flat[off:off + n]
        out.append(dict(lo=x[:, 0:3], kappa=x[:, 3], hi=x[:, 4:7], maxabs=x[:, 7]))
        off += n
    assert off == len(flat)
    return out


def passes_of(nodes, o, d):
    """box_pass of one ray (d normalised) against every node: a function (level, index) -> bool for wave_walk and ray_accel_ref.walk"""
    table = []
    for lv in nodes:
        n = len(lv["kappa"])
        table.append(A.box_pass(lv["lo"], lv["hi"], lv["kappa"], lv["maxabs"], np.tile(o, (n, 1)), np.tile(d, (n, 1))))
    return lambda level, idx: bool(table[level][idx])
