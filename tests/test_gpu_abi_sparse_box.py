"""tests/abi_sparse_box.c: a C ABI caller whose batch box ends a few pixels short of its triangle, in a sparse frame under row spans.  The
frame must leave every scratch word that the next launch assumes zero at zero, and a dense frame behind it on the same context must equal
the same dense frame on a fresh context -- with k_blockscan and with the general count / scan / fill pipeline."""
import os
import subprocess

import pytest

import rusterix_amd

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("blockscan", ["default", "0"])
def test_undersized_batch_box_leaves_clean_scratch(tmp_path, blockscan):
    lib = rusterix_amd.lib_paths()["rxr"]
    exe = str(tmp_path / "abi_sparse_box")
    cc = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "abi_sparse_box.c"),
                         "-o", exe, "-L" + os.path.dirname(lib), "-lrxr_hip", "-Wl,-rpath," + os.path.dirname(lib)], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    env = dict(os.environ, RXR_CONTENT_MIN_TILES="0")   # (row spans only pay from 8192 empty tiles on: this frame is small)
    if blockscan == "0":
        env["RXR_BLOCKSCAN"] = "0"
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok (0 failures)"), run.stdout[-6000:] + run.stderr[-2000:]
