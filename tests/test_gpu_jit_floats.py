"""Run-time compiled Rusteria programs (rxr_jit.hip: the generator, rxr_jit_ops.h's copies of the interpreter's handlers, the hiprtc
option list) against the interpreter and the oracle FLOAT FOR FLOAT, in frames: every program of tests/jit_floats.py ends in
`Time Mul Fract SetColor`, its set is uploaded once per mode and rendered once per window with time = 2^k, and the windows together show
every bit of the value (tests/test_jit_floats_cpu.py proves that, and that the material is not vacuous).  Oracle, interpreted frame
(RXR_SHADER_JIT=0) and compiled frame (RXR_SHADER_JIT=1, `rxr_debug_jit_info` says `compiled:`) must be equal byte for byte in every
window: a last-ulp difference in any exact opcode, a fused multiply-add, or a folded constant that rounds differently fails here.

One set per test: the compilation is the cost (printed with -s; profiles/jit_floats/README.md keeps the figures)."""
import numpy as np
import pytest

from tests import jit_floats as J
from tests.test_gpu_shader_jit import jit_info

pytestmark = pytest.mark.gpu

SETS = {fs.name: fs for fs in J.all_sets()}


def three_ways(oracle, product, monkeypatch, fs, frame_of, want):
    monkeypatch.setenv("RXR_SHADER_JIT", "0")
    interpreted = frame_of(product).windows()
    assert jit_info(product) == ""
    monkeypatch.setenv("RXR_SHADER_JIT", "1")
    compiled = frame_of(product).windows()
    info = jit_info(product)
    monkeypatch.setenv("RXR_SHADER_JIT", "0")
    assert info.startswith("compiled:"), f"{fs.name}: {info}"
    print(f"\n{fs.name}: {info}")
    return interpreted, compiled, info


@pytest.mark.parametrize("name", list(SETS))
def test_compiled_interpreted_and_oracle_frames_are_equal_in_every_window(oracle, product, monkeypatch, name):
    fs = SETS[name]
    want = J.reference_windows(oracle, fs)
    interpreted, compiled, info = three_ways(oracle, product, monkeypatch, fs, fs.frame, want)
    J.assert_same_frames(fs, want, interpreted, compiled, note=f" [{info}]")
    assert len(np.unique(want[1].reshape(-1, 4), axis=0)) > 1, "the frame shows nothing"


@pytest.mark.parametrize("site", J.SITES)
@pytest.mark.parametrize("name", ["random-static-0.0", "grid-binary"])
def test_the_same_at_the_3d_call_sites(oracle, product, monkeypatch, name, site):
    """the opaque pass of an unlit box and a chunk's opacity-list pane run the programs too (k_raster_jit at other template levels);
    equality of the three frames is all that is asserted: the sRGB encode there is not linear"""
    fs = SETS[name]
    frame_of = lambda api: J.SiteFrame(api, fs.programs, fs.assets_of, site)   # noqa: E731
    want = frame_of(oracle).windows()
    interpreted, compiled, info = three_ways(oracle, product, monkeypatch, fs, frame_of, want)
    bad = ((want != interpreted) | (want != compiled)).any(axis=3)
    if bad.any():
        k, y, x = (int(v) for v in np.argwhere(bad)[0])
        raise AssertionError(f"{name} at the {site} site [{info}]: {int(bad.sum())} pixels differ (per window "
                             f"{dict(zip(J.WINDOWS, bad.reshape(len(bad), -1).sum(axis=1).tolist()))}); first in window 2^{J.WINDOWS[k]} at pixel (x {x}, y {y}): "
                             f"oracle {want[k, y, x].tolist()}, interpreted {interpreted[k, y, x].tolist()}, compiled {compiled[k, y, x].tolist()}")
    assert (want[1] != want[2]).any(), "the windows change nothing: the programs are not drawn"
