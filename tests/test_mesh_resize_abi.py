"""rxr_resize_meshes' ABI and host arithmetic without a GPU: both prototypes are declared with the same arity in include/rxr.h, the
generated Rust mirror and rusterix_amd.rxr_abi(), the library exports them, the refusals that need no device answer RXR_ERR_INVALID, and
the new-base arithmetic (rusterix_amd/csrc/rxr_mesh_resize.h: prefix sums and the 2^31 output-slot limit) is held to a numpy
restatement over seeded count vectors, 0 and 2^31 - 1 included -- through the library and through tests/mesh_resize_bases_main.cpp, a
program of its own that is also built with -fsanitize=address,undefined and run directly."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import rusterix_amd
from rusterix_amd import binding as B
from tests import mesh_resize_ref as MR
from tests import mesh_update_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARITY = {"rxr_resize_meshes": 10, "rxr_resize_meshes_to": 11}
U31 = (1 << 31) - 1


def _arguments(text, pattern):
    m = re.search(pattern, text, flags=re.S)
    assert m, pattern
    return [a.strip() for a in m.group(1).split(",") if a.strip()]


def test_both_prototypes_agree_in_header_mirror_and_python():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rxr.h")).read(), flags=re.S)
    rs = open(os.path.join(ROOT, "shim", "rusterix-hip-shim", "src", "ffi.rs")).read()
    lib = rusterix_amd.rxr_abi()
    for name, arity in ARITY.items():
        c_args = _arguments(hdr, rf"\bint\s+{name}\s*\((.*?)\)\s*;")
        rs_args = _arguments(rs, rf"pub fn {name}\((.*?)\)\s*->\s*c_int;")
        fn = getattr(lib, name)
        assert len(c_args) == len(rs_args) == len(fn.argtypes) == arity and fn.restype is C.c_int, name
        # argument by argument: a pointer in one is a pointer in all, a u32 a u32
        for c_arg, rs_arg, py in zip(c_args, rs_args, fn.argtypes):
            pointer = "*" in c_arg
            assert pointer == ("*const" in rs_arg or "*mut" in rs_arg) == (py is C.c_void_p), (name, c_arg, rs_arg, py)
            if not pointer:
                assert c_arg.startswith("uint32_t") and rs_arg.endswith("u32") and py is C.c_uint32, (name, c_arg, rs_arg, py)
    # the uv array sits between the vertices and the indices in both
    for name in ARITY:
        names = [a.split()[-1].lstrip("*") for a in _arguments(hdr, rf"\bint\s+{name}\s*\((.*?)\)\s*;")]
        assert [n.replace("dev_", "") for n in names[:8]] == ["ctx", "mesh_indices", "n", "counts", "vertices", "uvs", "indices", "normals"], names


def test_the_library_exports_them():
    lib = rusterix_amd.load_rxr()
    for name in list(ARITY) + ["rxr_debug_resize_bases"]:
        assert hasattr(lib, name), f"librxr_hip.so does not export {name}"


def test_refusals_that_need_no_device():
    lib = rusterix_amd.rxr_abi()
    one = np.zeros(16, np.uint32)
    p = one.ctypes.data
    assert lib.rxr_resize_meshes(None, p, 1, p, p, p, p, p, 1, 1) == B.RXR_ERR_INVALID
    assert lib.rxr_resize_meshes_to(None, p, 1, p, p, None, p, p, 1, 1, None) == B.RXR_ERR_INVALID
    assert lib.rxr_resize_meshes(None, None, 0, None, None, None, None, None, 0, 0) == B.RXR_ERR_INVALID     # (a NULL context even with n == 0)


# ---- the new-base arithmetic ------------------------------------------------------------------------------------------------------------------
def library_bases(counts):
    lib = rusterix_amd.rxr_abi()
    c = np.ascontiguousarray(counts, np.uint32).reshape(-1, 2)
    bases = np.full((len(c), 4), 0xABABABAB, np.uint32)
    totals = np.zeros(4, np.uint64)
    reached = lib.rxr_debug_resize_bases(c.ctypes.data, len(c), bases.ctypes.data, totals.ctypes.data)
    return int(reached), bases, tuple(int(t) for t in totals)


def count_vectors():
    """seeded count vectors: small scenes, scenes with empty meshes, scenes that end just below, at and above the limit in either pool"""
    rng = np.random.default_rng(11)
    out = [np.zeros((0, 2), np.uint32), np.zeros((5, 2), np.uint32), np.array([[U31, 0]], np.uint32), np.array([[0, U31]], np.uint32),
           np.array([[U31, 0], [1, 0]], np.uint32), np.array([[0, 0], [U31 - 4, 1]], np.uint32), np.array([[3, (1 << 31) // 3]], np.uint32),
           np.array([[3, (1 << 31) // 3 + 1]], np.uint32), np.array([[0xFFFFFFFF, 0xFFFFFFFF]] * 4, np.uint32)]
    for _ in range(40):
        n = int(rng.integers(1, 400))
        c = rng.integers(0, 5000, (n, 2)).astype(np.uint32)
        c[rng.random(n) < 0.2] = 0
        out.append(c)
    for _ in range(20):     # around the limit: a few large meshes among small ones
        n = int(rng.integers(2, 30))
        c = rng.integers(0, 1 << 12, (n, 2)).astype(np.uint32)
        k = int(rng.integers(0, n))
        c[k] = (rng.integers(0, 1 << 31), rng.integers(0, 1 << 29))
        out.append(c)
    return out


def test_the_bases_equal_the_numpy_prefix_sums_and_the_limit_is_2_to_the_31_output_slots():
    fitted = refused = 0
    for c in count_vectors():
        reached, bases, totals = library_bases(c)
        want_reached, want_bases, want_totals = MR.bases(c)
        assert reached == want_reached and totals == want_totals, (c[:4], reached, want_reached)
        written = min(reached + 1, len(c))
        assert np.array_equal(bases[:written], want_bases[:written]) and (bases[written:] == 0xABABABAB).all()
        if reached == len(c):     # fits: the restatement as numpy prefix sums in 64 bits
            excl, total = MR.bases_numpy(c)
            assert np.array_equal(bases.astype(np.uint64), excl) and tuple(int(t) for t in total) == totals
            assert totals[2] < MR.SLOT_LIMIT and totals[3] < MR.SLOT_LIMIT
            fitted += 1
        else:
            assert totals[2] >= MR.SLOT_LIMIT or totals[3] >= MR.SLOT_LIMIT
            refused += 1
    assert fitted > 40 and refused > 5, (fitted, refused)
    # exactly at the edge: 2^31 - 1 output vertices fit, one more does not
    assert library_bases([[U31, 0]])[0] == 1 and library_bases([[U31, 0], [1, 0]])[0] == 1
    assert library_bases([[0, 0], [U31 - 4, 1]])[0] == 2 and library_bases([[0, 0], [U31 - 3, 1]])[0] == 1
    # triangles: 4 output vertices and 3 output slots each, so the vertex pool is the one that fills: 3 + 4 * (2^29 - 1) = 2^31 - 1 fits
    assert library_bases([[3, (1 << 29) - 1]])[0] == 1 and library_bases([[4, (1 << 29) - 1]])[0] == 0 and library_bases([[0, 1 << 29]])[0] == 0


def compiled(tmp_path_factory, name, *flags):
    exe = str(tmp_path_factory.mktemp("mesh_resize") / name)
    subprocess.run(["g++", "-O2", "-std=c++17", *flags, os.path.join(ROOT, "tests", "mesh_resize_bases_main.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    return compiled(tmp_path_factory, "bases"), compiled(tmp_path_factory, "bases_san", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")


def test_the_program_of_its_own_agrees_plain_and_under_the_sanitizers(programs, tmp_path):
    for k, c in enumerate(count_vectors()[:30]):
        path = tmp_path / f"counts{k}.bin"
        path.write_bytes(np.ascontiguousarray(c, np.uint32).tobytes())
        want_reached, want_bases, want_totals = MR.bases(c)
        outs = []
        for exe in programs:
            pr = subprocess.run([exe, str(path)], capture_output=True, text=True)
            assert pr.returncode == 0, (pr.stdout + pr.stderr)[-3000:]
            outs.append(pr.stdout)
        assert outs[0] == outs[1]
        lines = outs[0].splitlines()
        head = lines[0].split()
        assert int(head[1]) == want_reached and tuple(int(x) for x in head[3:7]) == want_totals
        got = np.array([[int(x) for x in ln.split()] for ln in lines[1:]], np.uint32).reshape(-1, 4)
        assert np.array_equal(got, want_bases[:min(want_reached + 1, len(c))])


def test_pack_with_uvs_leaves_the_slack_poisoned():
    a, b = M.grid_mesh(3, 1, seed=1), M.grid_mesh(1, 2, seed=2)
    counts, v, uv, i, nr = MR.pack([a, b], vstride=5, tstride=4, slack=True)
    assert counts.tolist() == [[3, 1], [1, 2]] and uv.shape == (2, 5, 2) and np.array_equal(uv[0, :3], a["uvs"]) and np.array_equal(uv[1, :1], b["uvs"])
    assert (uv.view(np.uint32)[0, 3:] == 0x7FC0BEEF).all() and (uv.view(np.uint32)[1, 1:] == 0x7FC0BEEF).all()
    grown = MR.resized(a, 7, 4, seed=3)
    assert len(grown["vertices"]) == 7 and len(grown["indices"]) == 4 and grown["list"] == a["list"] and (grown["indices"] < 7).all()
