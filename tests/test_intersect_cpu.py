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
from rusterix_amd.abi import RXR_ERR_INVALID
from tests import intersect_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NEW = ("rxr_intersect", "rxr_intersect_to", "rxr_screen_rays_to")


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


# ---- the vectorised reference and the seeded generator (tests/pick_fuzz.py) -------------------------------------------------------

from tests import pick_fuzz as P  # noqa: E402


def assert_bits(got, ref, label):
    assert set(got) == set(ref), label
    bad = P.differences(got, ref, label)
    assert bad is None, bad


@pytest.mark.parametrize("seed", P.SEEDS)
def test_intersect_many_equals_intersect(seed):
    """every output of both modes, bit for bit, on the generator's scenes and rays (the per-ray side sets the ray count: the whole
    parametrised test takes about a minute); a small max_pairs makes several ray blocks"""
    meshes = P.random_pick_scene(seed)
    o, d = P.random_rays(meshes, seed, 3000)
    o, d = o[:240], d[:240]
    recs = [R.tri_records(m) for m in meshes]
    for full in (False, True):
        ref = R.intersect(meshes, o, d, full=full, records=recs)
        assert_bits(R.intersect_many(meshes, o, d, full=full), ref, f"seed {seed} full={full}")
        assert_bits(R.intersect_many(meshes, o, d, full=full, max_pairs=50_000), ref, f"seed {seed} full={full} (small blocks)")


def test_intersect_many_on_the_adversarial_rays_and_hand_cases():
    from tests.test_gpu_intersect import adversarial_rays

    api = rusterix_amd.load()
    v, i, uv, n = api.Batch3D.from_box(3, 3, 3, 1, 1, 1).with_computed_normals().geometry()
    box = dict(vertices=v, indices=i, uvs=uv, normals=n, list=R.LIST_STATIC, has_pid=False, pid=0)
    o, d = adversarial_rays(np.random.default_rng(5))
    for meshes in ([quad(0.0), box],
                   [quad(0.0), quad(5.0, list=R.LIST_OVERLAY), quad(2.0), quad(3.0, list=R.LIST_OVERLAY), quad(-0.5, list=R.LIST_DYNAMIC)],
                   [quad(5.0, list=R.LIST_CHUNK, has_pid=True, pid=7), quad(0.0, list=R.LIST_CHUNK, has_pid=True, pid=7)],
                   [quad(0.0), quad(0.0)], []):
        for full in (False, True):
            assert_bits(R.intersect_many(meshes, o, d, full=full), R.intersect(meshes, o, d, full=full), f"{len(meshes)} meshes full={full}")
    # an accepted t of +inf beats a rejected triangle and loses to every finite t (huge coordinates)
    far = [quad(0.0), quad(1.0)]
    oo = np.array([[0.5, 0.25, -3e38]], np.float32)
    dd = np.array([[0.0, 0.0, 1.0]], np.float32)
    assert_bits(R.intersect_many(far, oo, dd, full=True), R.intersect(far, oo, dd, full=True), "huge")
    empty = R.intersect_many([quad(0.0)], np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), full=True)
    assert empty["t"].shape == (0,) and empty["normal"].shape == (0, 3)


def _empty_meshes_around_a_plain_run(meshes):
    """a plain run with a mesh without triangles right before it, inside it and right after it"""
    n = [len(m["indices"]) for m in meshes]
    for _, _, m0, m1, rule in P.segments(meshes):
        if rule == "plain" and m0 > 0 and n[m0 - 1] == 0 and 0 in n[m0:m1] and m1 < len(meshes) and n[m1] == 0:
            return True
    return False


def test_generator_gives_the_device_something_to_decide():
    """tests/test_gpu_intersect_fuzz.py compares the device with intersect_many on these seeds: here the reference alone shows that
    the scenes and rays exercise hits, many winners, the overlay rule, the profile-id rule, ties, meshes without triangles and
    segment ends on 1024-triangle boundaries"""
    overlay_behind = pid_decided = ties = 0
    holes = aligned = False
    for seed in P.SEEDS:
        meshes = P.random_pick_scene(seed)
        assert 5 <= len(meshes) <= 60 and sum(len(m["indices"]) for m in meshes) <= P.MAX_TRIANGLES + 300, seed
        for a, b in zip(meshes, meshes[1:]):   # rxr_set_meshes order: chunks (opacity, batches, terrain), static, dynamic, overlay
            key = lambda m: (0, m["chunk"], m["list"]) if m["list"] <= R.LIST_CHUNK_TERRAIN else (1, m["list"], 0)
            assert key(a) <= key(b), seed
        o, d = P.random_rays(meshes, seed, 3000)
        ref = R.intersect_many(meshes, o, d)
        hit = ref["mesh"] != R.MISS
        assert hit.mean() >= 0.30, (seed, hit.mean())
        assert len(np.unique(ref["mesh"][hit])) >= min(5, len(meshes)), (seed, np.unique(ref["mesh"][hit]))
        # every mesh alone: its own closest t per ray
        alone = [R.intersect_many([dict(m, list=R.LIST_STATIC)], o, d) for m in meshes]
        t_alone = np.stack([np.where(a["mesh"] != R.MISS, a["t"], np.float32(np.inf)) for a in alone])     # [mesh, ray]
        hit_alone = np.stack([a["mesh"] != R.MISS for a in alone])
        is_overlay = np.array([m["list"] == R.LIST_OVERLAY for m in meshes])
        win = np.where(hit, ref["mesh"], 0).astype(np.int64)
        overlay_behind += int((hit & is_overlay[win] & ((t_alone < ref["t"][None, :]) & hit_alone).any(axis=0)).sum())
        ties += int((hit & (((t_alone == ref["t"][None, :]) & hit_alone).sum(axis=0) >= 2)).sum())
        no_pid = R.intersect_many([dict(m, has_pid=False) for m in meshes], o, d)
        pid_decided += int((no_pid["mesh"] != ref["mesh"]).sum())
        holes |= _empty_meshes_around_a_plain_run(meshes)
        aligned |= any(end % 1024 == 0 for _, end, _, _, _ in P.segments(meshes)[:-1])
    assert overlay_behind >= 20 and pid_decided >= 20 and ties >= 20, (overlay_behind, pid_decided, ties)
    assert holes and aligned, (holes, aligned)


def test_segments_and_batches_restate_the_kernel_file():
    k = P.kernel_constants()
    assert k == dict(ISECT_WG=256, ISECT_FEW_RAYS=64, ISECT_RAYS_PER_Y=8, ISECT_KEYS_MAX=8 << 20), k
    assert P.expected_batches(32768, 300, k) == [27904, 4864]
    assert P.expected_batches(600, 33000, k) == [256, 256, 88]
    assert P.expected_batches(64000, 5, k) == [64000]
    ms = [quad(0.0), dict(quad(0.0), indices=np.zeros((0, 3), np.uint32)), quad(1.0, list=R.LIST_CHUNK),
          quad(2.0, list=R.LIST_CHUNK, has_pid=True, pid=3), quad(3.0, list=R.LIST_OVERLAY), quad(4.0, has_pid=True, pid=3)]
    assert P.segments(ms) == [(0, 4, 0, 3, "plain"), (4, 6, 3, 4, "pid"), (6, 8, 4, 5, "overlay"), (8, 10, 5, 6, "plain")]
