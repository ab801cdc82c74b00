"""The in-place mesh update's ABI without a GPU: rxr_update_meshes, rxr_update_meshes_to and rxr_mesh_bounds are declared with the
same arity in include/rxr.h, the generated Rust mirror and rusterix_amd.libs.rxr_abi(), the library exports them, a NULL context is
RXR_ERR_INVALID, and the numpy reference of the box (tests/mesh_update_ref.py) agrees with hand-computed boxes."""
import ctypes as C
import os
import re

import numpy as np

import rusterix_amd
from rusterix_amd import binding as B
from tests import mesh_update_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARITY = {"rxr_update_meshes": 9, "rxr_update_meshes_to": 10, "rxr_mesh_bounds": 4}


def _arguments(text, pattern):
    m = re.search(pattern, text, flags=re.S)
    assert m, pattern
    return [a for a in m.group(1).split(",") if a.strip()]


def test_the_three_prototypes_agree_in_header_mirror_and_python():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rxr.h")).read(), flags=re.S)
    rs = open(os.path.join(ROOT, "shim", "rusterix-hip-shim", "src", "ffi.rs")).read()
    lib = rusterix_amd.rxr_abi()
    for name, arity in ARITY.items():
        assert len(_arguments(hdr, rf"\bint\s+{name}\s*\((.*?)\)\s*;")) == arity, name
        assert len(_arguments(rs, rf"pub fn {name}\((.*?)\)\s*->\s*c_int;")) == arity, name
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == arity, name


def test_the_library_exports_them():
    lib = rusterix_amd.load_rxr()
    for name in ARITY:
        assert hasattr(lib, name), f"librxr_hip.so does not export {name}"
    assert hasattr(rusterix_amd.load().lib, "rxh_scene_rebuild_terrain_meshes")


def test_a_null_context_is_invalid():
    lib = rusterix_amd.rxr_abi()
    one = np.zeros(16, np.uint32)
    assert lib.rxr_update_meshes(None, one.ctypes.data, 1, one.ctypes.data, one.ctypes.data, one.ctypes.data, one.ctypes.data, 1, 1) == B.RXR_ERR_INVALID
    assert lib.rxr_update_meshes_to(None, one.ctypes.data, 1, one.ctypes.data, one.ctypes.data, one.ctypes.data, one.ctypes.data, 1, 1, None) == B.RXR_ERR_INVALID
    lo = (C.c_float * 3)()
    assert lib.rxr_mesh_bounds(None, 0, lo, lo) == B.RXR_ERR_INVALID


def test_the_reference_box_on_three_tiny_meshes():
    nan, inf = np.nan, np.inf
    # finite: w is not part of the box
    lo, hi = M.box([[1, 2, 3, 100], [-1, 5, 0, -100], [0, 0, 7, 1]])
    assert lo.tolist() == [-1, 0, 0] and hi.tolist() == [1, 5, 7]
    # a NaN coordinate is ignored, per coordinate: the vertex's other coordinates still count
    lo, hi = M.box([[nan, 2, 3, 1], [4, nan, -3, 1], [5, 1, nan, 1]])
    assert lo.tolist() == [4, 1, -3] and hi.tolist() == [5, 2, 3]
    # nothing but NaN, and no vertex at all: +inf / -inf
    for v in ([[nan, nan, nan, 1]] * 3, np.zeros((0, 4), np.float32)):
        lo, hi = M.box(v)
        assert lo.tolist() == [inf] * 3 and hi.tolist() == [-inf] * 3
    # ... and the vectorised form is the loop
    rng = np.random.default_rng(5)
    v = rng.standard_normal((300, 4)).astype(np.float32)
    v[rng.random((300, 4)) < 0.2] = nan
    for a, b in zip(M.box(v), M.box_fast(v)):
        assert np.array_equal(a, b)
    # -0.0 and +0.0 bounds compare equal (the sign of a zero bound is not specified)
    lo, hi = M.box([[-0.0, 0.0, 0.0, 1], [0.0, -0.0, -0.0, 1]])
    assert (lo == 0).all() and (hi == 0).all()


def test_pack_leaves_the_slack_poisoned():
    a = M.grid_mesh(3, 1, seed=1)
    b = M.grid_mesh(1, 2, seed=2)
    counts, v, i, nr = M.pack([a, b], vstride=5, tstride=4, slack=True)
    assert counts.tolist() == [[3, 1], [1, 2]] and v.shape == (2, 5, 4) and i.shape == (2, 4, 3) and nr.shape == (2, 5, 3)
    assert np.array_equal(v[0, :3], a["vertices"]) and np.isnan(v[0, 3:, 0]).all() and (i[1, 2:] == 0xFFFFFFFF).all()
    pv, pi, pn = M.expected_pools([a, b])
    assert pv.shape == (4, 4) and pi.shape == (3, 3) and np.array_equal(pn[3], b["normals"][0])
