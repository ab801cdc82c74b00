"""The rectangle geometry of the banded rxr_render_download (rusterix_amd/csrc/rxr_download_plan.h), without a GPU:
tests/download_plan_main.cpp is built with g++ -O2, and once more with -fsanitize=address,undefined, and run directly.  Its fuzz mode
draws seeded frames up to 300x300 -- content rows on tile rows or none, row_of as render_impl derives it for four bands, a span table (or
none) whose spans lie in content tile rows only, some rows empty, min_tiles zero or small -- and asserts for each that
 1. every pixel of the frame lies in exactly one rectangle of fills and copies,
 2. the copies are in ascending rows and each lies inside one band (the copy loop relies on it),
 3. every pixel inside a tile row's span lies in a copy, never in a fill,
 4. link bytes plus host bytes are W * H * 4,
 5. without a table there is exactly one whole-width copy per non-empty band,
 6. when the trimmed pixels fall under min_tiles * 256 all copies are whole-width and the fills are only the rows outside the content."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "download_plan_main.cpp")
CASES = 20000


def compiled(tmp_path_factory, name, *flags):
    exe = str(tmp_path_factory.mktemp("download_plan") / name)
    subprocess.run(["g++", "-O2", "-std=c++17", *flags, SRC, "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return compiled(tmp_path_factory, "download_plan")


@pytest.fixture(scope="module")
def program_sanitized(tmp_path_factory):
    return compiled(tmp_path_factory, "download_plan_san", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")


def run(exe, *args):
    pr = subprocess.run([exe, *args], capture_output=True, text=True)
    assert pr.returncode == 0, (pr.stdout + pr.stderr)[-3000:]
    return pr.stdout


def fuzz(exe, seed, cases):
    words = run(exe, "fuzz", str(seed), str(cases)).split()
    return {k: int(v) for k, v in zip(words[0::2], words[1::2])}


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_fills_and_copies_tile_the_frame_and_spans_travel(program, seed):
    got = fuzz(program, seed, CASES)
    assert got["cases"] == CASES
    # the cases are not vacuous: strided copies, wholly filled strips, the whole-row fallback (with something trimmed), the nine-tenths rule
    assert got["strided"] > CASES // 10 and got["filled_strips"] > CASES // 10, got
    assert got["fallback"] > CASES // 40 and got["nine_tenths"] > CASES // 100, got
    assert got["no_table"] > CASES // 10 and got["clipped"] > CASES // 2, got


def test_the_plan_worked_out_by_hand_and_a_frame_without_content(program):
    """160x128, bands of 32 rows, every tile row's span [2, 5): eight copies {16k, 16k + 16, 32, 80}, sixteen side fills, 24 576 bytes
    over the link and 57 344 from the host; c0 == c1: no copies, two fills that cover everything"""
    assert run(program, "known").strip() == "ok"


def test_the_fill_writer_writes_the_fill_pixels_and_nothing_else(program):
    """aligned and at base + 1, across 1, 4 and 8 workers: 00 00 00 FF in every fill pixel, the sentinel everywhere else"""
    assert run(program, "fills").strip() == "ok"


def test_the_same_under_the_sanitizers(program, program_sanitized):
    """AddressSanitizer and UndefinedBehaviorSanitizer: no report, and the same counts"""
    assert fuzz(program_sanitized, 4, CASES // 4) == fuzz(program, 4, CASES // 4)
    assert run(program_sanitized, "known").strip() == "ok"
    assert run(program_sanitized, "fills").strip() == "ok"
