"""Ray picking without a GPU: the ABI of rxr_intersect / rxr_intersect_to / rxr_screen_rays_to, the generated mirror, the
numpy restatement of Scene::intersect (tests/intersect_ref.py) on hand-computed cases, and the intersect kernels' code object."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import rusterix_amd
from tests import intersect_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NEW = ("rxr_intersect", "rxr_intersect_to", "rxr_screen_rays_to")
RXR_ERR_INVALID = -1


def test_entry_points_are_declared_and_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rxr.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(rf"\bint {name}\(", hdr), name
    assert re.search(r"#define RXR_INTERSECT_FULL \(1u << 0\)", hdr)
    assert re.search(r"#define RXR_ABI_VERSION 5u", hdr)
    lib = rusterix_amd.load_rxr()
    for name in NEW:
        assert hasattr(lib, name), name
    host = C.CDLL(rusterix_amd.lib_paths()["host"])
    for name in ("rxh_scene_intersect", "rxh_rasterizer_screen_ray"):
        assert hasattr(host, name), name
    rs = open(os.path.join(ROOT, "shim", "rusterix-hip-shim", "src", "ffi.rs")).read()
    for name in NEW:
        assert f"pub fn {name}(" in rs, name


def test_null_context_and_null_arrays_are_invalid():
    L = rusterix_amd.rxr_abi()
    buf = np.zeros(16, np.float32)
    p = buf.ctypes.data
    assert L.rxr_intersect(None, p, p, 1, 0, p, p, p, None, None, None) == RXR_ERR_INVALID
    assert L.rxr_intersect(None, None, None, 1, 0, None, None, None, None, None, None) == RXR_ERR_INVALID
    assert L.rxr_intersect_to(None, p, p, 1, 0, p, p, p, None, None, None, None) == RXR_ERR_INVALID
    assert L.rxr_screen_rays_to(None, p, p, 4.0, 4.0, 0, 0, 2, 2, p, p, None) == RXR_ERR_INVALID


def test_generated_files_stay_current_and_the_layout_asserts_untouched():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_ffi.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout
    if os.path.isdir(os.path.join(ROOT, ".git")):
        r = subprocess.run(["git", "-C", ROOT, "diff", "--quiet", "HEAD", "--", "tests/abi_layout_asserts.h"], capture_output=True)
        # (1: the file differs; other codes: git could not look, e.g. a checkout owned by another user -- --check above still holds)
        assert r.returncode != 1, "tests/abi_layout_asserts.h changed: the intersect ABI must add functions only"


def quad(z, normal=(0.0, 0.0, -1.0), **kw):
    v = np.array([(0, 0, z, 1), (1, 0, z, 1), (1, 1, z, 1), (0, 1, z, 1)], np.float32)
    m = dict(vertices=v, indices=np.array([(0, 1, 2), (0, 2, 3)], np.uint32), uvs=v[:, :2].copy(),
             normals=np.array([normal] * 4, np.float32), list=R.LIST_STATIC, has_pid=False, pid=0)
    m.update(kw)
    return m


O = np.array([[0.25, 0.75, -1.0]], np.float32)
D = np.array([[0.0, 0.0, 2.0]], np.float32)   # (un-normalised: t is measured along the normalised direction, the hit point is not)


def test_unit_quad():
    out = R.intersect([quad(0.0)], O, D, full=True)
    assert out["t"][0] == 1.0 and out["mesh"][0] == 0 and out["triangle"][0] == 1
    assert out["hitpoint"][0].tolist() == [0.25, 0.75, 1.0]   # origin + dir * t with the caller's dir (tracer/mod.rs:30-32)
    assert out["uv"][0].tolist() == [0.25, 0.75]
    assert out["normal"][0].tolist() == [0.0, 0.0, -1.0]
    flipped = R.intersect([quad(0.0, normal=(0.0, 0.0, 1.0))], O, D, full=True)
    assert flipped["normal"][0].tolist() == [-0.0, -0.0, -1.0]   # faces against the ray
    miss = R.intersect([quad(0.0)], O, -D, full=True)
    assert miss["t"][0] == R.FLT_MAX and miss["mesh"][0] == R.MISS and miss["triangle"][0] == 0
    assert miss["hitpoint"][0].tolist() == [0.0, 0.0, 0.0]


def test_coplanar_duplicates_the_earliest_wins():
    out = R.intersect([quad(0.0), quad(0.0)], O, D)
    assert out["mesh"][0] == 0 and out["triangle"][0] == 1
    m = quad(0.0)
    m["indices"] = np.array([(0, 1, 2), (0, 2, 3), (0, 2, 3)], np.uint32)
    assert R.intersect([m], O, D)["triangle"][0] == 1


def test_overlay_behind_a_static_mesh_wins():
    out = R.intersect([quad(0.0), quad(5.0, list=R.LIST_OVERLAY)], O, D)
    assert out["mesh"][0] == 1 and out["t"][0] == 6.0
    # ... while a farther static mesh does not
    assert R.intersect([quad(0.0), quad(5.0)], O, D)["mesh"][0] == 0


def test_chunk_profile_id_rule_changes_the_winner():
    far = quad(5.0, list=R.LIST_CHUNK, has_pid=True, pid=7)
    near_same = quad(0.0, list=R.LIST_CHUNK, has_pid=True, pid=7)
    near_other = quad(0.0, list=R.LIST_CHUNK, has_pid=True, pid=8)
    near_none = quad(0.0, list=R.LIST_CHUNK)
    assert R.intersect([far, near_same], O, D)["mesh"][0] == 0     # same profile id as the best: the farther hit stays
    assert R.intersect([far, near_other], O, D)["mesh"][0] == 1
    assert R.intersect([far, near_none], O, D)["mesh"][0] == 1
    # the rule applies to RXR_LIST_CHUNK only
    assert R.intersect([far, dict(near_same, list=R.LIST_STATIC)], O, D)["mesh"][0] == 1


def test_intersect_kernels_do_not_spill(tmp_path):
    import __graft_entry__ as G

    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out = tmp_path / "rxr_intersect.s"
    flags = [f for f in G.HIP_FLAGS if f not in ("-shared", "-fPIC")]
    subprocess.run([hipcc] + flags + ["--cuda-device-only", "-S", "-o", str(out), os.path.join(G.CSRC, "rxr_intersect.hip")],
                   check=True, stderr=subprocess.DEVNULL)
    isa = open(out).read()
    kernels = re.findall(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", isa, flags=re.S)
    names = [k for k, _ in kernels]
    for k in ("k_isect_prep", "k_isect_by_tri", "k_isect_by_ray", "k_isect_fold", "k_screen_rays"):
        assert any(k in n for n in names), k
    for name, body in kernels:
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1)) == 0, f"{name} uses scratch"
        assert int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", body).group(1)) <= 64, f"{name}: more than 64 VGPRs"
    assert not re.search(r"^\s+scratch_\w+", isa, flags=re.M), "scratch instructions in the intersect kernels"
