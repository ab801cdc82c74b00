"""Vertex normals without a GPU: the numpy transcription of tests/vertex_normals_ref.py against the oracle (every bit), the host
mirror's Scene::compute_static_normals / compute_dynamic_normals on the CPU against the oracle, rxr_check_vertex_normals' verdicts and
messages, and the generator's conditions for every seed the GPU tests use."""
import ctypes as C

import numpy as np
import pytest

import rusterix_amd
from rusterix_amd import binding as B
from rusterix_amd.abi import RXR_ERR_INVALID, RXR_OK
from tests import vertex_normals_ref as R
from tests.vertex_normals_ref import F

ORDER_SEEDS = (11, 12, 13, 14)          # tests/test_gpu_vertex_normals.py uses the same


@pytest.fixture(scope="module")
def api():
    return rusterix_amd.load()


# ---- the ground truth agrees with itself ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", ORDER_SEEDS + (21, 22))
def test_the_transcription_is_the_oracle_bit_for_bit(oracle, seed):
    for nv, nt, deg in ((40, 120, 0), (40, 120, 3), (7, 1, 0), (3, 50, 0), (64, 10, 1)):
        v, i = R.generated(seed, nv, nt, deg)
        assert R.same_bits(R.transcribed_normals(v, i), R.oracle_normals(oracle, v, i)), (seed, nv, nt, deg)


def test_the_transcription_is_the_oracle_on_fans_boxes_and_special_values(oracle):
    for valence in (1, 63, 64, 65, 257):
        v, i = R.fan(valence)
        assert R.same_bits(R.transcribed_normals(v, i), R.oracle_normals(oracle, v, i)), valence
    bv, bi, _, _ = oracle.Batch3D.from_box(-1.0, 0.5, 2.0, 2.0, 1.0, 3.0).geometry()
    assert bv.shape == (24, 4) and bi.shape == (12, 3)
    assert R.same_bits(R.transcribed_normals(bv, bi), R.oracle_normals(oracle, bv, bi))
    v, i = R.generated(5, 12, 30)
    v[3, 0], v[7, 2] = np.nan, np.inf
    assert R.same_bits(R.transcribed_normals(v, i), R.oracle_normals(oracle, v, i))


def test_a_lone_negative_zero_component_comes_out_positive(oracle):
    v, i = R.negative_zero_triangle()
    fn = R.face_normals(v, i)
    assert np.signbit(fn[0, 0]) and fn[0, 0] == 0 and fn[0, 1] == 1.0, fn
    want = R.oracle_normals(oracle, v, i)
    assert (want.view(np.uint32) == np.array([0, 0x3F800000, 0], np.uint32)).all(), want      # +0.0 + -0.0 = +0.0
    assert R.same_bits(R.transcribed_normals(v, i), want)


@pytest.mark.parametrize("seed", ORDER_SEEDS)
def test_the_order_seeds_meet_their_conditions(seed):
    """conditions of the GPU order test, not measurements: reversing the triangles changes the bits of at least a quarter of the
    vertices, and at most a quarter are NaN"""
    v, i = R.generated(seed, 40, 120)
    forward, backward = R.transcribed_normals(v, i), R.transcribed_normals(v, i, reverse=True)
    assert R.differing_vertices(forward, backward) >= 10, R.differing_vertices(forward, backward)
    assert int(np.isnan(forward).any(axis=1).sum()) <= 10
    assert all(len(set(t)) == 3 for t in i.tolist())


def test_the_generator_states_its_degenerate_triangles():
    v, i = R.generated(3, 40, 120, degenerate=4)
    assert [len(set(t)) for t in i.tolist()].count(2) == 4 and all(len(set(t)) == 3 for t in i[4:].tolist())
    assert (np.abs(v[:, :3]) <= 4).all() and (v[:, 3] == 1).all()


# ---- the mirror on the CPU -------------------------------------------------------------------------------------------------------------
def boxes_and_meshes(api):
    """a few batches: boxes and generated meshes, WITHOUT normals"""
    out = [api.Batch3D.from_box(-1.0 + k, 0.0, -5.0, 1.0, 1.0 + 0.25 * k, 1.0) for k in range(3)]
    for seed in (31, 32):
        v, i = R.generated(seed, 30, 70, degenerate=1)
        out.append(api.Batch3D.new(v, i, np.zeros((len(v), 2), F)))
    return out


@pytest.mark.parametrize("which", ["static", "dynamic"])
@pytest.mark.parametrize("threads", [False, True])
def test_the_mirrors_scene_normals_on_the_cpu_are_the_oracles(api, oracle, which, threads):
    scene = api.Scene.empty()
    batches = boxes_and_meshes(api)
    for b in batches:
        (scene.add_d3_static if which == "static" else scene.add_d3_dynamic)(b)
    kind = B.LIST_STATIC if which == "static" else B.LIST_DYNAMIC
    assert scene.batch3d_normals(kind, 0).shape == (0, 3)
    (scene.compute_static_normals if which == "static" else scene.compute_dynamic_normals)(threads=threads)
    other = scene.add_d3_dynamic if which == "static" else scene.add_d3_static      # (the other list is not touched)
    other(batches[0])
    assert scene.batch3d_normals(B.LIST_DYNAMIC if which == "static" else B.LIST_STATIC, 0).shape == (0, 3)
    for k, b in enumerate(batches):
        v, i, _, _ = b.geometry()
        assert R.same_bits(scene.batch3d_normals(kind, k), R.oracle_normals(oracle, v, i)), k


# ---- rxr_check_vertex_normals ---------------------------------------------------------------------------------------------------------------
def check(counts, indices, n, vs, ts):
    rxr = rusterix_amd.rxr_abi()
    msg = C.create_string_buffer(256)
    p = lambda a: None if a is None else a.ctypes.data
    rc = rxr.rxr_check_vertex_normals(p(counts), p(indices), n, vs, ts, msg, 256)
    return rc, msg.value.decode()


def test_check_vertex_normals_verdicts_and_messages():
    meshes = [R.generated(1, 9, 12), R.generated(2, 5, 3), R.generated(3, 9, 12)]
    counts, _, indices, _ = R.pack(meshes, vstride=10, tstride=14)
    assert check(counts, indices, 3, 10, 14) == (RXR_OK, "")
    assert check(None, None, 0, 10, 14) == (RXR_OK, "")                       # n == 0 does nothing
    bad = indices.copy()
    bad[1, 2, 1] = 5                                                          # == the mesh's vertex count
    rc, msg = check(counts, bad, 3, 10, 14)
    assert rc == RXR_ERR_INVALID and msg == "mesh 1: triangle 2 has a vertex index 5 that is not below its 5 vertices", msg
    bad = indices.copy()
    bad[2, 13, 0] = 0xFFFFFFFF                                                # past the mesh's triangle count: never read
    assert check(counts, bad, 3, 10, 14)[0] == RXR_OK
    c = counts.copy()
    c[2, 0] = 11
    rc, msg = check(c, indices, 3, 10, 14)
    assert rc == RXR_ERR_INVALID and msg == "mesh 2: its 11 vertices exceed vertex_stride 10", msg
    c = counts.copy()
    c[0, 1] = 15
    c[2, 0] = 11                                                              # (the FIRST offending mesh is named)
    rc, msg = check(c, indices, 3, 10, 14)
    assert rc == RXR_ERR_INVALID and msg == "mesh 0: its 15 triangles exceed triangle_stride 14", msg
    rc, msg = check(None, indices, 3, 10, 14)
    assert rc == RXR_ERR_INVALID and "NULL counts" in msg
    rc, msg = check(counts, None, 3, 10, 14)
    assert rc == RXR_ERR_INVALID and "NULL indices" in msg
    assert check(np.zeros((3, 2), np.uint32), None, 3, 10, 0)[0] == RXR_OK    # (an array of 0 bytes is not looked at)
    rc, msg = check(counts, indices, 1 << 31, 0xFFFFFFFF, 0xFFFFFFFF)
    assert rc == RXR_ERR_INVALID and "overflow" in msg
    # the message is cut to the caller's capacity
    rxr = rusterix_amd.rxr_abi()
    small = C.create_string_buffer(8)
    assert rxr.rxr_check_vertex_normals(None, indices.ctypes.data, 3, 10, 14, small, 8) == RXR_ERR_INVALID and small.value == b"NULL co"
