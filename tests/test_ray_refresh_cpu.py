"""The ranged refit's host side without a device (rusterix_amd/csrc/rxr_ray_refresh.h through tests/ray_refresh_walk.cpp): the dirty
node intervals of every level against a brute-force statement of the rule -- a node is dirty iff a dirty sorted position lies below
it -- over the shapes of tests/test_gpu_ray_refresh.py and seeded random dirty sets, the same program under AddressSanitizer and
UBSan, and the new symbols in the generated Rust mirror."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import ray_accel_ref as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "ray_refresh_walk.cpp")
L, W = A.LEAF, A.WIDTH


def brute(ntri, ranges, leaf=L, width=W):
    """per level (nodes of the level, the maximal runs [lo, hi] of dirty nodes)"""
    cnt = A.levels(ntri, leaf, width) if ntri else []
    mask = np.zeros(ntri, bool)
    for b, e in ranges:
        mask[b:e] = True
    nodes = np.unique(np.nonzero(mask)[0] // leaf)
    out = []
    for k, n in enumerate(cnt):
        if k:
            nodes = np.unique(nodes // width)
        assert not len(nodes) or nodes[-1] < n
        cut = np.nonzero(np.diff(nodes) > 1)[0] + 1
        runs = [(int(r[0]), int(r[-1])) for r in np.split(nodes, cut)] if len(nodes) else []
        out.append((n, runs))
    return out


def parse(text):
    cases, cur = [], None
    for line in text.splitlines():
        w = line.split()
        if w[0] == "case":
            cur = dict(ntri=int(w[1]), n_levels=int(w[2]), levels=[])
            cases.append(cur)
        else:
            runs = [tuple(int(x) for x in r.split("-")) for r in w[3:]]
            assert int(w[0]) == len(cur["levels"])
            cur["levels"].append((int(w[1]), int(w[2]), runs))
    return cases


def shaped_cases():
    """the shapes of the device tests: a leaf across two meshes, totals where a level fills with the dirty mesh first, in the middle
    and last, adjacent and distant meshes, everything, nothing, 257 one-triangle meshes"""
    out = [(24, [(0, 13)]), (24, [(13, 24)]), (24, [(0, 13), (13, 24)]), (24, []), (1, [(0, 1)]), (0, [])]
    for total in (64, 65, 512, 513, 4097):
        third = total // 3
        out += [(total, [(0, third)]), (total, [(third, 2 * third)]), (total, [(2 * third, total)]), (total, [(0, total)]),
                (total, [(third - 1, third), (third, third + 1)]), (total, [(0, 1), (total - 1, total)]), (total, [(5, 5)])]
    out.append((300, [(i, i + 1) for i in range(257)]))
    out.append((1 << 20, [(0, 1 << 20)]))
    out.append((1 << 20, [((1 << 20) - 512, 1 << 20)]))
    return out


def random_cases(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        ntri = int(2 ** rng.uniform(0, 20))
        k = int(rng.integers(0, 12))
        cuts = np.sort(rng.integers(0, ntri + 1, 2 * k))
        if rng.random() < 0.5 and ntri > 600:      # chunk-sized ranges far apart, as a stroke leaves them
            starts = np.sort(rng.integers(0, ntri - 512, k))
            cuts = np.sort(np.concatenate([starts, np.minimum(starts + 512, ntri)]))
        out.append((ntri, [(int(cuts[2 * i]), int(cuts[2 * i + 1])) for i in range(k)]))
    return out


def run_cases(exe, cases, tmp_path, env=None, leaf=L, width=W):
    path = tmp_path / "cases.txt"
    path.write_text("".join(" ".join(str(x) for x in [ntri] + [v for r in ranges for v in r]) + "\n" for ntri, ranges in cases))
    pr = subprocess.run([exe, str(leaf), str(width), "@" + str(path)], capture_output=True, text=True, timeout=300, env=env)
    assert pr.returncode == 0, (pr.stdout + pr.stderr)[-4000:]
    return parse(pr.stdout)


def check(got, cases, leaf=L, width=W):
    assert len(got) == len(cases)
    for g, (ntri, ranges) in zip(got, cases):
        # (ranges that overlap after sorting are still a union of positions: the brute force does not care)
        want = brute(ntri, ranges, leaf, width)
        assert g["ntri"] == ntri and g["n_levels"] == len(want), (ntri, ranges, g)
        for k, (n, runs) in enumerate(want):
            assert g["levels"][k] == (n, sum(hi - lo + 1 for lo, hi in runs), runs), (ntri, ranges, k, g["levels"][k], runs)


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("walk") / "ray_refresh_walk")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-o", exe, SRC], check=True)
    return exe


def test_the_shapes_of_the_device_tests(walk, tmp_path):
    cases = shaped_cases()
    check(run_cases(walk, cases, tmp_path), cases)


def test_random_dirty_sets_up_to_two_to_the_twenty(walk, tmp_path):
    cases = random_cases(3000, 20261020)
    assert max(c[0] for c in cases) > 1 << 19 and any(len(c[1]) == 0 for c in cases)
    check(run_cases(walk, cases, tmp_path), cases)


@pytest.mark.parametrize("leaf,width", [(1, 2), (4, 2), (16, 4)])
def test_other_leaf_sizes_and_widths(walk, tmp_path, leaf, width):
    cases = [c for c in random_cases(400, leaf * 100 + width) if c[0] <= 1 << 16]
    check(run_cases(walk, cases, tmp_path, leaf=leaf, width=width), cases, leaf, width)


def test_a_case_on_the_command_line(walk):
    pr = subprocess.run([walk, str(L), str(W), "24", "0", "13"], capture_output=True, text=True)
    assert pr.returncode == 0
    check(parse(pr.stdout), [(24, [(0, 13)])])


def test_the_walk_is_clean_under_asan_and_ubsan(tmp_path):
    for lib in ("libasan.a", "libubsan.a"):
        found = subprocess.run(["g++", "-print-file-name=" + lib], capture_output=True, text=True).stdout.strip()
        if not os.path.isabs(found) or not os.path.exists(found):
            pytest.skip(f"this g++ has no static {lib}")
    exe = str(tmp_path / "ray_refresh_walk_asan")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-static-libasan", "-static-libubsan", "-o", exe, SRC]
    pr = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert pr.returncode == 0, pr.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    cases = shaped_cases() + random_cases(500, 7)
    check(run_cases(exe, cases, tmp_path, env=env), cases)


def test_the_generated_ffi_and_the_layout_asserts(tmp_path):
    pr = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_ffi.py"), "--check"], capture_output=True, text=True)
    assert pr.returncode == 0, pr.stdout + pr.stderr
    ffi = open(os.path.join(ROOT, "shim", "rusterix-hip-shim", "src", "ffi.rs")).read()
    for name in ("rxr_set_ray_refresh", "rxr_ray_refresh_info", "rxr_ray_refresh_verify", "rxr_ray_accel_invalidate", "RXR_RAY_REFRESH_FULL",
                 "RXR_RAY_REFRESH_RANGED", "RXR_RAY_REFIT_SMALL_MAX", "RXR_RAY_REFRESH_INFO_WORDS", "RXR_RAY_REFRESH_VERIFY_WORDS"):
        assert name in ffi, name
    hdr = open(os.path.join(ROOT, "include", "rxr.h")).read()
    words = {k: int(v) for k, v in re.findall(r"#define (RXR_RAY_REFRESH_(?:INFO|VERIFY)_\w+) (\d+)u", hdr)}
    assert words["RXR_RAY_REFRESH_INFO_WORDS"] == 8 and words["RXR_RAY_REFRESH_VERIFY_WORDS"] == 5
    # the header as C11 with the generated layout asserts (tests/abi_host.c includes both): syntax and asserts only, nothing is linked
    pr = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only", os.path.join(ROOT, "tests", "abi_host.c")],
                        capture_output=True, text=True)
    assert pr.returncode == 0, pr.stderr[-4000:]
