"""Which raster kernel a launch gets (rusterix_amd/csrc/rxr_route.h), over the whole fact space, on the CPU.

The cases below ARE the specification -- the table that used to sit above the launcher as a comment, written as Python; none of them
reads the decision code.  tests/raster_route_walk.cpp prints the function's answer for all 6 x 2 x 3 x 2^8 = 18 432 combinations of
(kernel_level, plain_programs, fused_small, 3D pass active, split_rounds, span table attached, relaxed lights with lights, opacity pass,
tile_stride 1 / 2, RXR_NO_ROWS, RXR_PAIR_TILES=1).  tests/test_gpu_routes.py pins the same names to scenes on the device."""
import collections
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Row = collections.namedtuple("Row", "level plain fused d3 split spans rl opacity stride no_rows pairs name takes pair_grid")

# the kernels that look RasterParams.row_spans up (raster_tile's SPANS): every feature level >= 1, the two _sp kernels, rows_cut
READS_SPANS = {"k_raster_vm", "k_raster_vm_s", "k_raster_vm_sv", "k_raster_vm_p", "k_raster_vm_v", "k_raster_chunk", "k_raster_chunk_rl",
               "k_raster_chunk_cut", "k_raster_chunk_cut_rl", "k_raster_rows_sp", "k_raster_rows_rl_sp", "k_raster_rows_cut", "k_raster_rows_cut_rl"}
ALL = READS_SPANS | {"k_raster", "k_raster_rl", "k_raster_fused", "k_raster_rows", "k_raster_rows_rl", "k_raster_pair", "k_raster_pair_rl"}


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    exe = tmp_path_factory.mktemp("route") / "walk"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "rusterix_amd", "csrc"),
                    os.path.join(ROOT, "tests", "raster_route_walk.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    rows = [Row(*(f if i == 11 else int(f) for i, f in enumerate(line.split()))) for line in out.splitlines()]
    assert len(rows) == 6 * 2 * 3 * 2 ** 8 and len({r[:11] for r in rows}) == len(rows)
    return rows


def binned_rows(r):  # a binned 3D frame that may run rounds in row mode
    return r.level == 0 and r.fused == 0 and r.d3 and not r.no_rows


def pair(r):
    return binned_rows(r) and r.pairs and not r.opacity and r.stride == 1


def rl(r):  # frames without a 3D light loop: one kernel for both light modes
    return "_rl" if r.rl and r.d3 else ""


def takes_spans_answer(r):
    """rxr_raster_takes_spans: would the kernel of this launch look the span table up if it were attached?"""
    if r.level >= 1:
        return 1
    if r.fused != 0 or not r.d3 or r.no_rows:
        return 0
    if r.pairs and not r.opacity and r.stride == 1:
        return 0
    return 1


# (case, its rows of the walk, the kernel each of them gets)
CASES = [
    ("interpreter levels", lambda r: r.level >= 2,
     lambda r: {5: "k_raster_vm_v", 4: "k_raster_vm_p" if r.plain else "k_raster_vm_sv", 3: "k_raster_vm_s", 2: "k_raster_vm"}[r.level]),
    ("chunk", lambda r: r.level == 1,
     lambda r: "k_raster_chunk" + ("_cut" if r.split and r.fused == 0 and r.d3 else "") + rl(r)),
    ("fused", lambda r: r.level == 0 and r.fused == 1, lambda r: "k_raster_fused"),
    ("pair", pair, lambda r: "k_raster_pair" + rl(r)),
    ("rows_cut", lambda r: binned_rows(r) and not pair(r) and r.split, lambda r: "k_raster_rows_cut" + rl(r)),
    ("rows_sp and rows", lambda r: binned_rows(r) and not pair(r) and not r.split,
     lambda r: "k_raster_rows" + rl(r) + ("_sp" if r.spans else "")),
    ("plain", lambda r: r.level == 0 and r.fused != 1 and not binned_rows(r), lambda r: "k_raster" + rl(r)),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_route_table(walk, case):
    _, select, kernel = case
    mine = [r for r in walk if select(r)]
    assert mine
    attached = {r[:11]: r for r in walk if r.spans}  # the same launch with the span table attached
    for r in mine:
        assert r.name == kernel(r), r
        assert r.takes == (r.name in READS_SPANS), r
        assert r.pair_grid == (r.name in ("k_raster_pair", "k_raster_pair_rl")), r
        assert attached[r[:5] + (1,) + r[6:11]].takes == takes_spans_answer(r), r


def test_every_kernel_is_reached_and_every_launch_is_some_case(walk):
    assert {r.name for r in walk} == ALL and len(ALL) == 20
    assert all(sum(1 for _, select, _ in CASES if select(r)) == 1 for r in walk)
