"""bench.py without --full: the headline only (exactly --steps timed steps, nothing measured beside them), and --dump-outputs: the
frame of the last timed step as float32, the same bytes whether one GPU renders it or the N > 1 path (rehearsed on this one GPU,
RXR_BENCH_REHEARSAL=1) assembles it from its ranks' stripes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bench(world, out, **env):
    e = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    e.update(env)
    pr = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(world), "--steps", "3", "--warmup", "1",
                         "--width", "1280", "--height", "720", "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600, env=e, cwd=ROOT)
    assert pr.returncode == 0, pr.stdout[-2000:] + pr.stderr[-4000:]
    lines = [l for l in pr.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, pr.stdout
    return json.loads(lines[0])


def test_plain_run_times_the_steps_and_dumps_the_last_frame(tmp_path):
    d = bench(1, tmp_path / "one")
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["warmup_steps_run"] >= 1
    assert d["unit"] == "Mpixels/s" and d["higher_is_better"] is True and d["dtype"] == "f32" and d["value_semantics"] == "device-resident"
    assert d["ms_per_step"] > 0 and abs(d["value"] - 1280 * 720 / d["ms_per_step"] / 1e3) <= 0.01 * d["value"]
    assert not {"roofline", "cpu_baseline", "e2e_ms", "other_light_math", "two_frames_in_flight"} & set(d), sorted(d)
    one = np.load(tmp_path / "one" / "frame.npy")
    assert one.dtype == np.float32 and one.shape == (720, 1280, 4) and d["outputs"]["frame"] == [720, 1280, 4]
    assert (one[..., 3] == 255).all() and one[..., :3].max() > 0
    d2 = bench(2, tmp_path / "two", RXR_BENCH_REHEARSAL="1")
    assert d2["n_gpus"] == 2 and d2["steps"] == 3 and "exchange_variants" not in d2 and "per_rank" not in d2
    assert np.array_equal(np.load(tmp_path / "two" / "frame.npy"), one)
