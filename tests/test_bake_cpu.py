"""The shader-texture bake without a GPU: rxr_check_bake (the acceptance rule of include/rxr.h), the ABI additions and the generated
mirrors, the bake kernels' code object, and the reference of tests/bake_ref.py on hand-computed cases -- including that the byte
comparison tests/test_gpu_bake.py makes with it is not vacuous for the programs it uses."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import rusterix_amd
from rusterix_amd import binding as B
from rusterix_amd.binding import Program
from tests import bake_ref as R
from tests.bake_ref import P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rxr_check_bake", "rxr_bake_shaders", "rxr_bake_shaders_to")
CARRIED = ["Roughness", "Metallic", "Opacity", "Normal", "Bump"]


def check_bake(programs, index):
    lib = rusterix_amd.rxr_abi()
    s, keep = R.shader_set(programs)
    msg = C.create_string_buffer(512)
    rc = lib.rxr_check_bake(C.cast(C.byref(s), C.c_void_p), index, msg, 512)
    return rc, msg.value.decode()


# ---- rxr_check_bake ----------------------------------------------------------------------------------------------------------------
def test_accepts_colour_only_programs_and_programs_that_only_read_a_carried_field():
    progs = list(R.exact_programs().values()) + list(R.special_programs().values()) + list(R.libm_programs().values())
    for i in range(len(progs)):
        rc, msg = check_bake(progs, i)
        assert rc == 0 and msg == "", (i, msg)
    for field in CARRIED:
        rc, msg = check_bake([P([field, "SetColor"])], 0)
        assert rc == 0, (field, msg)
        # written first, then read: the same invocation's value
        rc, msg = check_bake([P([("Push", 0.3, 0.4, 0.5), "Set" + field, field, "SetColor"])], 0)
        assert rc == 0, (field, msg)
        # written and never read
        rc, msg = check_bake([P(["UV", "SetColor", ("Push", 0.3, 0.4, 0.5), "Set" + field])], 0)
        assert rc == 0, (field, msg)


@pytest.mark.parametrize("field", CARRIED)
def test_refuses_read_before_write_of_a_carried_field(field):
    """Rusteria::shade resets only uv and color between texels: the read would see what the previous texel wrote"""
    for prog in (P([field, "SetColor", ("Push", 0.3, 0.4, 0.5), "Set" + field]),
                 # written on one path only
                 P(["UV", ("GetComponents", [0]), ("Push", 0.5), "Lt", ("If", [("Push", 0.3, 0.4, 0.5), "Set" + field], None), field, "SetColor"]),
                 # read in a callee before shade writes it
                 P([("FunctionCall", 0, 0, 1), "SetColor", ("Push", 0.3, 0.4, 0.5), "Set" + field], [field])):
        rc, msg = check_bake([P(["UV", "SetColor"]), prog], 1)
        assert rc == B.RXR_ERR_UNSUPPORTED and field.lower() in msg, (field, rc, msg)
    if field == "Normal":   # the raster loops assign `normal` before every call: for frames this program is fine, for a bake it is not
        lib = rusterix_amd.rxr_abi()
        s, keep = R.shader_set([P([field, "SetColor", ("Push", 0.3, 0.4, 0.5), "Set" + field])])
        assert lib.rxr_check_shaders(C.byref(s), None, None, 0) == 0
        assert check_bake([P(["UV", "SetColor"]), P([field, "SetColor", ("Push", 0.3, 0.4, 0.5), "Set" + field])], 0)[0] == 0   # the OTHER program of the set bakes


@pytest.mark.parametrize("prog, expect", [
    (P([("Push", 4.0), ("Push", 4.0), "Alloc"]), "Alloc"),
    (P([("For", [], [("Push", 0.0)], [], ["Return"])]), "Return inside For"),
    (P([("LoadGlobal", 0), "SetColor"], globals=1), "read before"),
    (P([("LoadLocal", 0), "SetColor"], shade_locals=1), "read before"),
    (P(["UV", "SetColor", ("Push", 1.0, 2.0, 3.0), "SetUV"]), "reads uv"),
    (P(["Emissive", "SetColor", ("Push", 0.5), "SetEmissive"]), "emissive"),
    (P([], globals=17), "globals"),
])
def test_refuses_everything_rxr_check_shaders_refuses(prog, expect):
    """... wherever in the set the refused program sits: a bake is defined for a program of a set rxr_set_shaders accepts"""
    for progs, index in (([prog], 0), ([P(["UV", "SetColor"]), prog], 0)):
        rc, msg = check_bake(progs, index)
        assert rc == B.RXR_ERR_UNSUPPORTED and expect in msg, (rc, msg)


def test_invalid_indices_and_programs_without_shade():
    plain, none = P(["UV", "SetColor"]), Program([[("Push", 0.5), "SetColor"]], shade_index=None)
    assert check_bake([plain, none], 1)[0] == B.RXR_ERR_INVALID          # shade_index -1: add_shader pushes None, nothing is baked
    assert check_bake([plain, none], 0)[0] == 0
    assert check_bake([plain, none], 2)[0] == B.RXR_ERR_INVALID          # out of range
    assert check_bake([], 0)[0] == B.RXR_ERR_INVALID
    assert check_bake([Program([[]], shade_index=3)], 0)[0] == B.RXR_ERR_INVALID   # (rxr_check_shaders' own)
    lib = rusterix_amd.rxr_abi()
    assert lib.rxr_check_bake(None, 0, None, 0) == B.RXR_ERR_INVALID
    msg = C.create_string_buffer(8)       # a short buffer is filled and terminated
    s, keep = R.shader_set([plain])
    assert lib.rxr_check_bake(C.cast(C.byref(s), C.c_void_p), 5, msg, 8) == B.RXR_ERR_INVALID and len(msg.value) == 7


# ---- the ABI -----------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_mirrored():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rxr.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(rf"\bint {name}\(", hdr), name
    assert re.search(r"#define RXR_ABI_VERSION 5u", hdr)
    m = re.search(r"#define RXR_BAKE_MAX_TEXELS \(1u << (\d+)\)", hdr)
    assert m and int(m.group(1)) <= 31, "n * width * height must fit in 32 bits"
    lib = rusterix_amd.load_rxr()
    for name in NEW:
        assert hasattr(lib, name), name
    host = C.CDLL(rusterix_amd.lib_paths()["host"])
    for name in ("rxh_scene_bake_shaders", "rxh_chunk_add_shader_baked", "rxh_chunk_shader_texture"):
        assert hasattr(host, name), name
    rs = open(os.path.join(ROOT, "shim", "rusterix-hip-shim", "src", "ffi.rs")).read()
    for name in NEW:
        assert f"pub fn {name}(" in rs, name
    import __graft_entry__ as G

    assert "rxr_bake.hip" in open(G.__file__).read()


def test_null_context_is_invalid():
    L = rusterix_amd.rxr_abi()
    progs = np.zeros(1, np.uint32)
    out = np.zeros(64, np.float32)
    assert L.rxr_bake_shaders(None, progs.ctypes.data, 1, 2, 2, out.ctypes.data, None) == B.RXR_ERR_INVALID
    assert L.rxr_bake_shaders_to(None, progs.ctypes.data, 1, 2, 2, out.ctypes.data, None, None) == B.RXR_ERR_INVALID


def test_generated_files_stay_current_and_the_layout_asserts_untouched():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_ffi.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout
    if os.path.isdir(os.path.join(ROOT, ".git")):
        r = subprocess.run(["git", "-C", ROOT, "diff", "--quiet", "HEAD", "--", "tests/abi_layout_asserts.h"], capture_output=True)
        # (1: the file differs; other codes: git could not look -- --check above still holds)
        assert r.returncode != 1, "tests/abi_layout_asserts.h changed: the bake ABI must add functions only"


# ---- the code object ---------------------------------------------------------------------------------------------------------------
def kernel_metadata(tmp_path):
    """{kernel name: {key: value}} of every gfx950 kernel in the built device library (its code objects' metadata notes)"""
    import __graft_entry__ as G

    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    llvm = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "llvm", "bin")
    if not os.path.exists(os.path.join(llvm, "llvm-objdump")):
        llvm = "/opt/rocm/llvm/bin"
    so = tmp_path / "librxr_hip.so"
    shutil.copy(os.path.join(G.CSRC, "librxr_hip.so"), so)
    subprocess.run([os.path.join(llvm, "llvm-objdump"), "--offloading", str(so)], check=True, cwd=tmp_path, capture_output=True)   # unbundles next to the file
    kernels = {}
    for f in sorted(os.listdir(tmp_path)):
        if "gfx950" not in f:
            continue
        notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", str(tmp_path / f)], check=True, capture_output=True, text=True).stdout
        for block in notes.split("- .agpr_count")[1:]:
            name = re.search(r"^    \.name:\s+(\S+)", block, flags=re.M).group(1)   # (four spaces: the kernel's own keys, not its arguments')
            kernels[name] = {k: v for k, v in re.findall(r"^    \.(private_segment_fixed_size|group_segment_fixed_size|uses_dynamic_stack|vgpr_count):\s+(\S+)", block, flags=re.M)}
    return kernels


def test_bake_kernels_have_no_dynamic_stack_and_no_more_scratch_than_the_programmed_raster_kernels(tmp_path):
    """the interpreter's deep stack slots, locals, globals and call frames are scratch by design (rxr_vm.h); the bake adds nothing to
    them, and its LDS is exactly the value-stack block the programmed raster kernels size for themselves"""
    k = kernel_metadata(tmp_path)
    raster = [n for n in k if n.startswith("k_raster_vm")]
    assert len(raster) >= 4 and "k_bake" in k and "k_bake_s" in k, sorted(k)
    most = max(int(k[n]["private_segment_fixed_size"]) for n in raster)
    for n in ("k_bake", "k_bake_s"):
        assert k[n]["uses_dynamic_stack"] == "false", n
        assert int(k[n]["private_segment_fixed_size"]) <= most, (n, k[n], most)
        assert int(k[n]["group_segment_fixed_size"]) <= min(int(k[r]["group_segment_fixed_size"]) for r in raster), n
    src = open(os.path.join(ROOT, "rusterix_amd", "csrc", "rxr_vm.h")).read()
    slots = int(re.search(r"#define RXR_VM_LDS_STACK (\d+)", src).group(1))
    assert int(k["k_bake_s"]["group_segment_fixed_size"]) == slots * 3 * 256 * 4


# ---- the reference -----------------------------------------------------------------------------------------------------------------
def test_reference_on_hand_computed_cases(oracle):
    progs = R.exact_programs()
    names = list(progs)
    ref = R.Reference(oracle, [progs[n] for n in names])
    g = ref.pixels(names.index("gradient"), 4, 2)
    assert g.shape == (2, 4, 4)
    assert g[0, 0].tolist() == [0.0, 1.0, 0.0, 1.0] and g[1, 3].tolist() == [0.75, 0.5, 0.0, 1.0]    # top row first: uv.y = 1 - y / H
    assert (ref.pixels(names.index("addition"), 3, 3)[..., :3] == 0.5).all()                           # (2 + 2) / 8
    f = ref.pixels(names.index("fib"), 6, 1)[0, :, 0] * 8
    assert f.tolist() == [0.0, 1.0, 1.0, 2.0, 3.0, 5.0]
    fields = ref.pixels(names.index("fields"), 2, 2)
    assert np.array_equal(fields[..., :3], R.uv_of(2, 2) * np.float32(0.5))                            # roughness 0.5, every other field 0
    # bytes: the cast saturates, truncates, maps NaN to 0; -0.0 was +0.0 already in the float buffer
    px = np.array([[[0.0, 1.0, 2.0, 1.0], [-1.0, np.nan, np.inf, 1.0], [-np.inf, 0.25, 1e-30, 1.0]]], np.float32)
    want = [[0, 255, 255, 255], [0, 0, 255, 255], [255, int(0.25 ** R.GAMMA * 255), 0, 255]]   # (powf(-inf, 0.4545) is +inf)
    assert R.expected_bytes(px)[0].tolist() == want
    assert not R.boundary_band(px).any()
    mz = R.Reference(oracle, [R.special_programs()["minus_zero_above_one"]]).pixels(0, 2, 1)
    assert not np.signbit(mz[..., 0]).any() and (mz[..., 1] >= 2).all()


def test_the_byte_comparison_is_not_vacuous(oracle):
    """fewer than 1 % of the colour channels of the programs the GPU test bakes lie in the boundary band (where a byte may differ by
    one), per program and overall; and the programs produce every special class of value"""
    total = in_band = 0
    for group in (R.exact_programs(), R.special_programs(), R.libm_programs()):
        names = list(group)
        ref = R.Reference(oracle, [group[n] for n in names])
        for i, n in enumerate(names):
            px = ref.pixels(i, 64, 64)
            band = R.boundary_band(px)
            assert band.mean() < 0.01, (n, float(band.mean()))
            total += band.size
            in_band += int(band.sum())
            if n == "arith":
                assert len(np.unique(R.expected_bytes(px).reshape(-1, 4), axis=0)) > 500   # a real image
    assert in_band / total < 0.01
    sp = R.special_programs()
    ref = R.Reference(oracle, list(sp.values()))
    c = np.concatenate([ref.pixels(i, 64, 64)[..., :3].reshape(-1) for i in range(len(sp))])
    assert (c < 0).any() and (c == 0).any() and (c == 1).any() and (c > 1).any() and np.isposinf(c).any() and np.isneginf(c).any() and np.isnan(c).any()
