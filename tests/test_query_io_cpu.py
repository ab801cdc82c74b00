"""Where the blocking device queries put their host arrays inside their lane's io buffer (rusterix_amd/csrc/rxr_query_layout.h), on
the CPU.

tests/query_layout_walk.cpp prints the layout for the array lists of the four entry points (rxr_intersect, rxr_terrain_hits,
rxr_bake_shaders, rxr_bake_terrain), every subset of their optional outputs, at 1, 63, 64, 65 and 1000 rays / texels.  The table
below states the lists again, in Python; the properties: a present array has its bytes, starts on a 16-byte boundary (the shader
bake stores float4 texels) and overlaps no other; an absent array takes no room; the total is the end of the last array."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = (1, 63, 64, 65, 1000)
# per query: (bytes per ray or texel, optional) in the entry point's order
QUERIES = {
    "intersect": [(12, False), (12, False), (4, False), (4, False), (4, False), (12, True), (8, True), (12, True)],
    "terrain_hits": [(12, False), (12, False), (4, False), (4, True), (12, True), (8, True)],
    "bake_shaders": [(16, True), (4, True)],
    "bake_terrain": [(4, False)],
}


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    exe = tmp_path_factory.mktemp("query_io") / "walk"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "rusterix_amd", "csrc"),
                    os.path.join(ROOT, "tests", "query_layout_walk.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    rows = {}
    for line in out.splitlines():
        f = line.split()
        key = (f[0], int(f[1]), int(f[2]))
        assert key not in rows
        rows[key] = (int(f[3]), [tuple(int(v) for v in s.split(":")) for s in f[4:]])
    return rows


@pytest.mark.parametrize("query", sorted(QUERIES))
def test_layout(walk, query):
    arrays = QUERIES[query]
    n_opt = sum(1 for _, optional in arrays if optional)
    mine = {k: v for k, v in walk.items() if k[0] == query}
    assert sorted(mine) == sorted((query, n, s) for n in COUNTS for s in range(1 << n_opt))     # every subset at every count
    for (_, n, subset), (total, sections) in mine.items():
        assert len(sections) == len(arrays)
        opt, end = 0, 0
        for (unit, optional), (off, size) in zip(arrays, sections):
            present = True
            if optional:
                present = bool((subset >> opt) & 1)
                opt += 1
            label = f"{query}, n = {n}, subset {subset:b}: section at {off} of {size} bytes"
            if not present:
                assert size == 0, label         # (it takes no room: the next section starts where this one would have)
                continue
            assert size == n * unit, label
            assert off % 16 == 0, label
            assert off >= end, label            # in order and disjoint: it starts behind every earlier section's end
            assert off - end < 16, label        # ... with no more than the alignment's padding in between
            end = off + size
        assert total == end, f"{query}, n = {n}, subset {subset:b}: total {total}, last section ends at {end}"


def test_the_walk_covers_the_four_entry_points(walk):
    assert {k[0] for k in walk} == set(QUERIES) and len(walk) == len(COUNTS) * (8 + 8 + 4 + 1)
