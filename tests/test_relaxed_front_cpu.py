"""The alpha byte of a 3D fragment at the levels without chunk paths and programs is the texel's alpha byte (shade3d_end,
rusterix_amd/csrc/rxr_kernels.hip): the reference forms opacity = a / 255 (a correctly rounded float32 division, rasterizer.rs:1313)
and encodes it as trunc(clamp(opacity, 0, 1) * 255 + 0.5); the kernels used to do the same with one fused multiply-add.  Both round
trips return `a` for every byte, so the kernels now keep the byte."""
import numpy as np


def test_the_alpha_byte_survives_the_round_trip_through_opacity():
    a = np.arange(256, dtype=np.float32)
    opacity = a / np.float32(255.0)                      # numpy's float32 division is correctly rounded, like the reference's
    assert opacity.dtype == np.float32
    clamped = np.minimum(np.maximum(opacity, np.float32(0.0)), np.float32(1.0))
    # the kernel's fma(x, 255, 0.5): the float64 product of two float32 numbers is exact and 0.5 adds exactly at these magnitudes
    # (below 2^9 with 53 bits): one rounding, to float32
    fused = (clamped.astype(np.float64) * 255.0 + 0.5).astype(np.float32)
    assert np.array_equal(fused.astype(np.int32) & 0xFF, np.arange(256)), "fma form (the kernels)"
    # the reference's own form: product rounded to float32, then the sum rounded
    unfused = (clamped * np.float32(255.0)) + np.float32(0.5)
    assert unfused.dtype == np.float32
    assert np.array_equal(unfused.astype(np.int32) & 0xFF, np.arange(256)), "mul + add form (the reference)"
    # ... and the alpha test around it (`alpha == 255`, :1408) sees the same byte
    assert np.array_equal((fused.astype(np.int32) & 0xFF) == 255, np.arange(256) == 255)
