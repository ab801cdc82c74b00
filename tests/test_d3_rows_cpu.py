"""The tile rows a triangle can reach (rxr_tri_tile_rows, rusterix_amd/csrc/rxr_device.h), without a GPU: tests/d3_rows_main.cpp is built
with g++ -O2 -ffp-contract=off, and once more with -fsanitize=address,undefined, and run directly.  Its fuzz mode makes seeded records at
16x16, 48x64 and 333x187 -- ordinary triangles, slivers, triangles far larger than the frame (coefficients up to 1e30), walls whose
pixel box is clamped to the full height, zero-area triangles and all-zero records, NaN and +-inf in each coefficient -- and checks for
each that (1) every pixel centre that passes the pixel box and the three !(r < 0) tests, in visit()'s float expressions and by brute
force, lies in a tile row inside the range, and (2) the binary search returns the range of a linear scan over all tile rows."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "d3_rows_main.cpp")
# 21 cases are one round of 3 frame sizes x 7 kinds; 27 rounds put each of NaN, +inf, -inf into each of the nine coefficients at each
# frame size
CASES = 21 * 400


def compiled(tmp_path_factory, name, *flags):
    exe = str(tmp_path_factory.mktemp("d3_rows") / name)
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", *flags, SRC, "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return compiled(tmp_path_factory, "d3_rows")


@pytest.fixture(scope="module")
def program_sanitized(tmp_path_factory):
    return compiled(tmp_path_factory, "d3_rows_san", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")


def fuzz(exe, seed, cases):
    pr = subprocess.run([exe, "fuzz", str(seed), str(cases)], capture_output=True, text=True)
    assert pr.returncode == 0, (pr.stdout + pr.stderr)[-3000:]
    words = pr.stdout.split()
    return {k: int(v) for k, v in zip(words[0::2], words[1::2])}


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_covered_pixels_lie_inside_the_range_and_the_search_equals_the_scan(program, seed):
    got = fuzz(program, seed, CASES)
    assert got["records"] == CASES
    # the cases are not vacuous: records with rows and without, ranges that the edges narrowed below the pixel box's, covered pixels
    assert got["with_rows"] > CASES // 4 and got["empty"] > CASES // 20, got
    assert got["narrowed_by_edges"] > CASES // 20 and got["covered_pixels"] > 100 * CASES, got


def test_the_same_under_the_sanitizers(program, program_sanitized):
    """AddressSanitizer and UndefinedBehaviorSanitizer: no report, and the same counts"""
    assert fuzz(program_sanitized, 4, CASES // 4) == fuzz(program, 4, CASES // 4)


def test_all_zero_records_reach_nothing(program, tmp_path):
    """an invisible edge record or a skipped batch leaves an all-zero record: the union over such a frame is the empty range"""
    recs = tmp_path / "zeros.bin"
    recs.write_bytes(bytes(96 * 5))
    pr = subprocess.run([program, "time", str(recs), "64", "1"], capture_output=True, text=True)
    assert pr.returncode == 0, pr.stderr
    words = pr.stdout.split()
    assert words[:5] == ["records", "5", "range", "0", "0"], pr.stdout
