"""tests/abi_no_normals.c: a C ABI caller hands over a small frame with a 3D batch WITHOUT normals (the host mirror refuses such batches,
the C ABI takes them).  The set-up records rxr_upload_frame makes on the host equal k_setup3d's byte for byte -- zero normals for that
batch although the staging blob's normals pool holds an earlier frame's values there -- and the frame rendered from them equals the frame
of a context created under RXR_HOST_SETUP=0 (tests/test_gpu_host_setup.py has the cases that go through the mirror)."""
import os
import subprocess

import pytest

import rusterix_amd

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_a_batch_without_normals_gets_the_device_s_records(tmp_path):
    lib = rusterix_amd.lib_paths()["rxr"]
    exe = str(tmp_path / "abi_no_normals")
    cc = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "abi_no_normals.c"),
                         "-o", exe, "-L" + os.path.dirname(lib), "-lrxr_hip", "-Wl,-rpath," + os.path.dirname(lib)], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok (0 failures)"), run.stdout[-6000:] + run.stderr[-2000:]
