"""The ulp harness of tests/libm_ref.py checked without a GPU, on the CPU oracle (orc_vm_shade on glibc, through
tests/bake_ref.Reference): the texel-to-operand map, the operand sets, the oracle's own error against the float64 reference, and
that the checker has teeth -- a sine with a careless range reduction fails it where it should.

The oracle's measured maxima are printed (pytest -s) and recorded in profiles/libm_ulp/README.md; they are not asserted: what is
asserted is the bound tests/test_gpu_libm_ulp.py holds the device to."""
import numpy as np
import pytest

from tests import libm_ref as L

W, H = L.W, L.H


def test_pass_through_returns_every_operand_and_visits_every_texel_once(oracle):
    o = L.oracle_results(oracle)
    index = np.zeros((H, W, 3), np.float32)
    index[..., 0] = np.arange(W)[None, :]
    index[..., 1] = np.arange(H)[:, None]
    index[..., 2] = np.arange(W * H).reshape(H, W)
    got = L.by_operand(o.bake(L.PASS_THROUGH, [index]))
    assert np.array_equal(got, index), "the texel-to-operand map of by_operand is not the bake's"
    assert np.array_equal(np.sort(got[..., 2].reshape(-1)), np.arange(W * H))          # every pattern texel exactly once
    for op in ("Sin", "Atan", "Log", "Pow"):
        a = L.operand_set(op).a
        got = L.by_operand(o.bake(L.PASS_THROUGH, [a]))
        plain = np.isfinite(a) & (a != 0)
        assert plain.sum() > 9000 and np.array_equal(got[plain].view(np.uint32), a[plain].view(np.uint32)), op   # denormals included
        assert np.array_equal(np.isnan(got), np.isnan(a)) and np.array_equal(got == 0, a == 0), op            # (+-0 comes back as a zero)
        assert np.array_equal(got[np.isinf(a)], a[np.isinf(a)]), op
        assert (np.abs(a[plain]) < 2.0 ** -126).any() and np.isnan(a).any() and (a == 0).any(), op


def test_operand_sets_hold_what_they_are_meant_to():
    for op in L.OPS:
        s = L.operand_set(op)
        assert s.a.shape == (H, W, 3) and s.a.dtype == np.float32 and (s.b is None) == (op in L.UNARY), op
        assert s.part.shape == (H, W, 3)
        again = L.operand_set.__wrapped__(op)
        assert np.array_equal(again.a.view(np.uint32), s.a.view(np.uint32)), f"{op}: the set is not reproducible"
    t = L.operand_set("Sin")
    big = np.abs(t.a[np.isfinite(t.a)])
    assert (big > 1e30).sum() > 500 and (t.part == "k pi/2 +- 8 ulp").sum() > 2000
    k = np.rint(t.a[t.part == "k pi/2 +- 8 ulp"].astype(np.float64) / (np.pi / 2))
    assert k.max() >= 2 ** 22 - 1 and k.min() < -1000
    # every part of a set reaches the x component, the only one Sin1 / Cos1 compute
    assert set(np.unique(t.part[..., 0])) == set(np.unique(t.part))
    lg = L.operand_set("Log").a
    assert ((lg > 0) & (lg < 2.0 ** -126)).sum() > 500 and (lg < 0).sum() > 300 and (np.abs(lg - 1) < 1e-5).sum() >= 129
    pw = L.operand_set("Pow")
    assert ((np.abs(pw.a - 1) < 2.0 ** -10) & (np.abs(pw.b) > 2.0 ** 10)).sum() > 500 and (pw.b == np.float32(0.4545)).sum() >= 3000
    at = L.operand_set("Atan2")
    with np.errstate(all="ignore"):
        r = np.log2(np.abs(at.a.astype(np.float64) / at.b.astype(np.float64)))
    assert (r[np.isfinite(r)] > 100).any() and (r[np.isfinite(r)] < -100).any()
    for sy in (False, True):       # every quadrant, every +-0 / +-inf combination
        for sx in (False, True):
            assert ((np.signbit(at.a) == sy) & (np.signbit(at.b) == sx) & np.isfinite(at.a) & (at.a != 0) & (at.b != 0)).sum() > 1000
            for ky in (0.0, np.inf):
                for kx in (0.0, np.inf):
                    assert ((np.abs(at.a) == ky) & (np.abs(at.b) == kx) & (np.signbit(at.a) == sy) & (np.signbit(at.b) == sx)).any()
    ro = L.operand_set("Rotate2D")
    assert (np.abs(ro.b) > 1e5).sum() > 100 and ((ro.b % 90 == 0) & (ro.b != 0)).sum() > 1000


@pytest.mark.parametrize("op", L.OPS)
def test_the_oracle_meets_the_class_rule_and_the_bound(oracle, op):
    """glibc through the oracle's interpreter: class rule and OpenCL bound on every set; the measured maximum is printed"""
    v = L.judge(op, L.oracle_results(oracle).results(op))
    print("\noracle " + v.line())
    assert not v.failures, v.message()
    if op != "Rotate2D":
        assert v.n_band < 0.01 * v.n_judged, f"{op}: {v.n_band} of {v.n_judged} operands in the exemption band"


@pytest.mark.parametrize("op", L.OPS)
def test_exemption_band_and_frame_window_on_the_reference_alone(op):
    """fewer than 1 % of a set is exempt; at least half of it has results inside the windows the frame tests can see (judged on the
    float64 reference: the device's results differ from it by ulps)"""
    s = L.operand_set(op)
    m = L.used(op)
    ref = L.reference(op, s.a, s.b)
    if op != "Rotate2D":
        over, under = L.exempt_band(ref, L.BOUND[op])
        assert ((over | under) & m).sum() < 0.01 * m.sum(), (op, int((over & m).sum()), int((under & m).sum()))
    seen = L.in_window(ref) & m
    assert seen.sum() >= 0.5 * m.sum(), (op, int(seen.sum()), int(m.sum()))


def test_the_measure_on_hand_computed_cases():
    assert L.ulp32(np.float64(1.0)) == 2.0 ** -23 and L.ulp32(np.float64(0.75)) == 2.0 ** -24 and L.ulp32(np.float64(1e-45)) == 2.0 ** -149
    assert L.ulp32(np.float64(3e38)) == 2.0 ** 104 and L.ulp32(np.float64(0.0)) == 2.0 ** -149
    c = L.classes(np.float64([np.nan, np.inf, -np.inf, 0.0, -0.0, 1.0, -1.0, L.OVERFLOW, L.FLT_MAX, -4e38]))
    assert c.tolist() == [0, 1, 2, 3, 3, 4, 5, 1, 4, 2]
    assert L.classes(np.float32([np.nan, np.inf, -0.0, -3.0])).tolist() == [0, 1, 3, 5]
    over, under = L.exempt_band(np.float64([L.OVERFLOW + 2.0 ** 105, L.OVERFLOW + 2.0 ** 107, 1e-39, 0.0, 2.0 ** -126]), 4.0)
    assert over.tolist() == [True, False, False, False, False] and under.tolist() == [False, False, True, False, False]
    # a result 3 ulp off passes a 4-ulp opcode, 5 ulp off fails and names its part; so do a wrong sign, a zero and a NaN
    s = L.operand_set("Sin")
    good = L.reference("Sin", s.a).astype(np.float32)
    assert not L.judge("Sin", good).failures and L.judge("Sin", good).max_ulp <= 0.5
    y, x = np.argwhere((s.part[..., 0] == "dense [-2pi, 2pi]") & (np.abs(good[..., 0]) > 0.5))[0]
    for delta, fails in ((3, False), (5, True)):
        off = good.copy()
        off[y, x, 0] = (off[y, x, 0:1].view(np.int32) + delta).view(np.float32)[0]
        v = L.judge("Sin", off)
        assert bool(v.failures) == fails and (not fails or (v.failed_parts() == ["dense [-2pi, 2pi]"] and "ulp" in v.message()))
        assert abs(v.max_ulp - delta) <= 0.5 or fails
    for wrong in (-good[y, x, 0], 0.0, np.nan, np.inf):
        off = good.copy()
        off[y, x, 0] = wrong
        v = L.judge("Sin", off)
        assert len(v.failures) == 1 and "class" in v.message(), v.message()
    one = good.copy()
    one[..., 1] = good[..., 0]          # Sin1 must zero the other components
    assert L.judge("Sin1", one).failures and not L.judge("Sin1", L.reference("Sin1", s.a).astype(np.float32)).failures


def test_teeth_a_careless_range_reduction_fails_on_large_arguments_and_near_k_pi_2():
    """f32 sin after an f32 fmod by 2 pi -- what a cheap hardware-style sine amounts to -- passes the dense part and must fail, by
    name, on the large arguments and on the neighbours of k pi/2"""
    s = L.operand_set("Sin")
    with np.errstate(all="ignore"):
        reduced = np.fmod(s.a, np.float32(2 * np.pi))
        degraded = np.sin(reduced)
    assert reduced.dtype == np.float32 and degraded.dtype == np.float32
    v = L.judge("Sin", degraded)
    assert "large arguments [1e5, 3.4e38]" in v.failed_parts() and "k pi/2 +- 8 ulp" in v.failed_parts(), v.failed_parts()
    assert "dense [-2pi, 2pi]" not in v.failed_parts(), v.message()
    assert "large arguments" in v.message() and "k pi/2" in v.message()
    rot = L.operand_set("Rotate2D")
    ref, _ = L.rotate_reference(rot.a, rot.b)
    assert not L.judge("Rotate2D", ref.astype(np.float32)).failures
    with np.errstate(all="ignore"):
        rad = np.fmod(rot.b[..., 0] * L.DEG, np.float32(2 * np.pi)).astype(np.float64)
    sloppy = np.stack([rot.a[..., 0] * np.cos(rad) - rot.a[..., 1] * np.sin(rad), rot.a[..., 0] * np.sin(rad) + rot.a[..., 1] * np.cos(rad), rot.a[..., 2]], -1)
    assert "angles to 1e6" in L.judge("Rotate2D", sloppy.astype(np.float32)).failed_parts()
