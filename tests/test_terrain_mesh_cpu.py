"""The terrain chunk mesh without a GPU: the host mirror's CPU Terrain::build_mesh against the dictionary transcription of
tests/terrain_mesh_ref.py (every bit, normals from the oracle), the closed form the kernel computes against that transcription on
seeded random presence masks, and hand-computed pins of the reference's behaviour."""
import numpy as np
import pytest

import rusterix_amd
from tests import terrain_mesh_ref as M
from tests.terrain_mesh_ref import F, HeightSpec


@pytest.fixture(scope="module")
def api():
    return rusterix_amd.load()


def mirror(api, spec, coord):
    v, i, uv, n = spec.product(api).build_mesh(coord).geometry()
    assert not uv.any() and uv.shape == (len(v), 2)
    return dict(vertices=v, indices=i, normals=n)


def both(api, oracle, spec, coord):
    """the reference's mesh, after checking that the mirror's CPU build_mesh equals it in every bit"""
    want = M.build_mesh(spec, coord, oracle)
    got = mirror(api, spec, coord)
    assert not M.first_difference(got, want), M.first_difference(got, want)
    return want


# ---- the closed form ---------------------------------------------------------------------------------------------------------------------
def test_the_closed_form_is_the_transcription_on_random_masks():
    rng = np.random.default_rng(13)
    for case in range(300):
        cs = int(rng.integers(1, 17))
        mask = rng.random((cs, cs)) < rng.choice([0.0, 0.1, 0.3, 0.5, 0.7, 0.9, 1.0])
        assert M.closed_form(mask) == M.transcription(mask), (case, cs)
    for cs in (1, 2, 3, 8, 9):
        for name, mask in M.masks(cs).items():
            assert M.closed_form(mask) == M.transcription(mask), (cs, name)


def test_incident_triangles_ascend_and_number_at_most_six():
    _, triangles, incident = M.transcription(np.ones((5, 5), bool))
    assert max(len(i) for i in incident) == 6 and min(len(i) for i in incident) == 1
    assert all(i == sorted(i) for i in incident) and len(triangles) == 50


# ---- hand-pinned ------------------------------------------------------------------------------------------------------------------------
def test_a_single_cell(api, oracle):
    spec = HeightSpec((1.0, 1.0), 4).height(1, 2, 3.0)
    m = both(api, oracle, spec, (0, 0))
    assert m["vertices"].tolist() == [[1, 3, 2, 1], [2, 0, 2, 1], [1, 0, 3, 1], [2, 0, 3, 1]]     # (0,0), (1,0), (0,1), (1,1); only the cell itself has a height
    assert m["indices"].tolist() == [[0, 2, 1], [1, 2, 3]]
    # triangle 0 = (p0, p2, p1): cross((0,-3,1), (1,-3,0)) = (3, 1, 3) / sqrt(19); triangle 1 is flat: (0, 1, 0)
    n0 = np.array([3, 1, 3], F) / np.sqrt(F(19))
    assert np.array_equal(m["normals"][3], np.array([0, 1, 0], F))
    assert np.allclose(m["normals"][0], n0, atol=1e-6)


def test_two_cells_side_by_side_share_two_corners(api, oracle):
    spec = HeightSpec((1.0, 1.0), 4).height(0, 0, 1.0).height(1, 0, 2.0)
    m = both(api, oracle, spec, (0, 0))
    assert len(m["vertices"]) == 6
    assert m["vertices"][:, [0, 2]].tolist() == [[0, 0], [1, 0], [0, 1], [1, 1], [2, 0], [2, 1]]     # the second cell adds (2,0) and (2,1)
    assert m["indices"].tolist() == [[0, 2, 1], [1, 2, 3], [1, 3, 4], [4, 3, 5]]


def test_an_l_of_three_cells(api, oracle):
    spec = HeightSpec((1.0, 1.0), 4).height(0, 0, 1.0).height(0, 1, 2.0).height(1, 1, 3.0)
    m = both(api, oracle, spec, (0, 0))
    # row 0: cell (0,0) makes (0,0) (1,0) (0,1) (1,1); row 1: cell (0,1) adds (0,2) (1,2); cell (1,1) adds (2,1) (2,2)
    assert m["vertices"][:, [0, 2]].tolist() == [[0, 0], [1, 0], [0, 1], [1, 1], [0, 2], [1, 2], [2, 1], [2, 2]]
    assert m["indices"].tolist() == [[0, 2, 1], [1, 2, 3], [2, 4, 3], [3, 4, 5], [3, 5, 6], [6, 5, 7]]
    _, _, incident = M.transcription(M.present_mask(spec, (0, 0), 4))
    assert incident[3] == [1, 2, 3, 4]                       # corner (1,1): cell (0,0) triangle 1, cell (0,1) both, cell (1,1) triangle 0


def test_a_chunk_at_negative_coordinates(api, oracle):
    spec = HeightSpec((0.75, 1.5), 3)
    for x, y in ((-3, -6), (-1, -6), (-2, -5), (-1, -4)):
        spec.height(x, y, M.height_at(x, y))
    m = both(api, oracle, spec, (-1, -2))
    assert len(m["indices"]) == 8
    assert m["vertices"][0].tolist() == [F(-3) * F(0.75), M.height_at(-3, -6), F(-6) * F(1.5), 1.0]
    assert len(both(api, oracle, spec, (-2, -2))["vertices"]) == 0 and len(both(api, oracle, spec, (0, 0))["indices"]) == 0


def test_the_rim_reads_the_neighbour_chunk_or_zero(api, oracle):
    spec = HeightSpec((1.0, 1.0), 2)
    for y in range(2):
        for x in range(2):
            spec.height(x, y, 5.0)
    spec.height(2, 0, 7.0).height(2, 1, 8.0)                  # the chunk to the right; none below
    m = both(api, oracle, spec, (0, 0))
    at = {(int(v[0]), int(v[2])): float(v[1]) for v in m["vertices"]}
    assert len(at) == 9 and at[(2, 0)] == 7.0 and at[(2, 1)] == 8.0     # its heights, though its cells are not cells of this mesh
    assert at[(0, 2)] == 0.0 and at[(1, 2)] == 0.0 and at[(2, 2)] == 0.0
    assert len(m["indices"]) == 8


def test_flat_terrain_has_normals_exactly_up(api, oracle):
    for h, scale in ((0.0, (1.0, 1.0)), (2.5, (0.75, 1.5))):
        spec = HeightSpec(scale, 3)
        for y in range(4):
            for x in range(4):
                spec.height(x, y, h)
        m = both(api, oracle, spec, (0, 0))
        assert len(m["normals"]) == 16
        assert (M.bits(m["normals"]) == M.bits(np.array([0.0, 1.0, 0.0], F))).all()      # +0.0, not -0.0


def test_a_listed_zero_is_a_cell_and_an_unlisted_cell_is_not(api, oracle):
    spec = HeightSpec((1.0, 1.0), 2).height(0, 0, 0.0)
    assert len(both(api, oracle, spec, (0, 0))["indices"]) == 2
    assert len(both(api, oracle, HeightSpec((1.0, 1.0), 2).height(5, 5, 1.0), (0, 0))["indices"]) == 0


@pytest.mark.parametrize("cs", [1, 3, 8, 9])
def test_the_mirror_on_every_mask(api, oracle, cs):
    for name, mask in M.masks(cs).items():
        for coord, scale in (((0, 0), (1.0, 1.0)), ((-2, 1), (0.75, 1.5))):
            spec = M.masked_spec(mask, coord, scale, seed=cs, neighbours=name != "hole")
            m = both(api, oracle, spec, coord)
            assert len(m["indices"]) == 2 * int(mask.sum()), (cs, name)


def test_the_mesh_goes_in_as_a_chunks_terrain_batch(api):
    mesh = M.masked_spec(np.ones((2, 2), bool)).product(api).build_mesh((0, 0))
    assert mesh.counts() == (9, 8)
    api.Scene.empty().add_chunk().terrain_batch3d(mesh)      # (asserts that the scene took it)
