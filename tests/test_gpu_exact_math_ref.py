"""The short division / square-root / normalisation / cast sequences of rusterix_amd/csrc/rxr_exact_math.h against IEEE-754 as the host
computes it (tests/exact_math_ref.py): operands chosen on the host, one helper per call through rxr_debug_exact_math, every result
compared float by float with numpy's float32 operators -- a reference that owes nothing to hipcc, unlike rxr_selftest_math's
(tests/test_gpu_exact_math.py), whose two sides are compiled together.

The exact kinds must equal the reference in every bit (any NaN for a NaN, the sign of every zero included).  normalize3_relaxed is
held to relaxed_bound() -- 4 ulp per component and 3 for the magnitude, the model of a 1-ulp v_rsq_f32 -- and pow_exp2_log2 to
3 + 7 ln 2 |k log2 x| ulp; their measured maxima are printed (pytest -s) and recorded in profiles/exact_math/README.md."""
import ctypes as C

import numpy as np
import pytest

from tests import exact_math_ref as E

pytestmark = pytest.mark.gpu

RXR_ERR_INVALID = -1


class Probe:
    def __init__(self, product):
        import rusterix_amd
        from rusterix_amd import abi

        assert abi.RXR_ERR_INVALID == RXR_ERR_INVALID
        self.lib = rusterix_amd.rxr_abi()
        self.ctx = product.lib.rxh_context()
        assert self.ctx
        self._results = {}

    def call(self, kind, ops, results):
        n = len(ops)
        return self.lib.rxr_debug_exact_math(self.ctx, E.KIND[kind], ops.ctypes.data_as(C.c_void_p), n, results.ctypes.data_as(C.c_void_p))

    def run(self, kind, ops):
        ops = np.ascontiguousarray(ops, np.float32)
        out = np.full((len(ops), 4), np.float32(-12345.0))
        assert self.call(kind, ops, out) == 0, self.lib.rxr_last_error(self.ctx)
        return out

    def results(self, kind, name):
        """the device's results on a whole set: computed once, read-only"""
        if (kind, name) not in self._results:
            r = self.run(kind, E.operand_sets(kind)[name])
            r.setflags(write=False)
            self._results[kind, name] = r
        return self._results[kind, name]


@pytest.fixture(scope="module")
def probe(product):
    return Probe(product)


EXACT_CASES = [(k, s) for k in E.EXACT for s in E.SET_NAMES[k]]


@pytest.mark.parametrize("kind,name", EXACT_CASES, ids=[f"{k}-{s.replace(' ', '_')}" for k, s in EXACT_CASES])
def test_exact_kind_equals_the_ieee_reference(probe, kind, name):
    ops = E.operand_sets(kind)[name]
    got, ref = probe.results(kind, name), E.reference(kind, ops)
    report = E.exact_report(kind, name, ops, got, ref)
    print(f"{kind} [{name}]: {len(ops)} tuples, {int(E.differing(got, ref).sum())} differ")
    assert report is None, report


@pytest.mark.parametrize("kind", E.WITH_OUTSIDER)
def test_one_outsider_changes_the_sequence_never_the_value(probe, kind):
    """every inside wave again with one lane outside the window: the vote sends the whole wave down the compiler's path, and the 63
    untouched lanes must return the bits they returned on the short path"""
    lane, _ = E.outsider_lanes(kind)
    inside, out = probe.results(kind, "inside"), probe.results(kind, "one outsider")
    keep = np.ones(len(inside), bool)
    keep[np.arange(len(lane)) * E.WAVE + lane] = False
    ops = E.operand_sets(kind)["one outsider"]
    report = E.exact_report(kind, "one outsider, untouched lanes", ops[keep], out[keep], inside[keep], what="inside run")
    assert report is None, report


@pytest.mark.parametrize("kind", [k for k in E.KINDS if k not in E.DPP])
def test_partial_last_wave(probe, kind):
    """n = 64 k + 1 and 64 k + 63: the lanes behind the last tuple take no part, and the tuples return what they return in whole waves
    (the one-outsider sets where a kind has one: wave 3's outsider sits in lane 3 -- cut off by n = 193, inside n = 255)"""
    name = "one outsider" if kind in E.WITH_OUTSIDER else E.SET_NAMES[kind][0]
    ops, whole = E.operand_sets(kind)[name], probe.results(kind, name)
    for n in (3 * E.WAVE + 1, 3 * E.WAVE + 63):
        got = probe.run(kind, ops[:n])
        report = E.exact_report(kind, f"{name}, first {n}", ops[:n], got, whole[:n], what="whole-wave run")
        assert report is None, report


def test_relaxed_normalisation_stays_within_its_bound(probe):
    """normalize3_relaxed against the exact form.  Waves whose squared magnitudes are all inside [2^-80, 2^80] take the short path: every
    component within relaxed_bound()[0] ulp32 of the exact form's value and the magnitude within relaxed_bound()[1].  Every other wave
    (zero, denormal, infinite, NaN or out-of-window magnitudes) takes the exact path and must equal the exact form bit for bit."""
    kind = "normalize3_relaxed"
    bound_c, bound_m = E.relaxed_bound()
    worst = {"component": (0.0, None), "magnitude": (0.0, None)}
    failures = []
    n_short = n_exact = 0
    for name in E.SET_NAMES[kind]:
        ops, got = E.operand_sets(kind)[name], probe.results(kind, name)
        short = np.repeat(E.short_path(kind, ops), E.WAVE)
        n_short, n_exact = n_short + int(short.sum()), n_exact + int((~short).sum())
        if (~short).any():
            report = E.exact_report(kind, name + ", exact path", ops[~short], got[~short], E.reference(kind, ops[~short]), what="exact form")
            if report:
                failures.append(report)
        if short.any():
            o, g = ops[short], got[short]
            d = E.relaxed_distance(o, g)
            d = np.where(np.isfinite(d), d, np.inf)
            for label, part, bound in (("component", d[:, :3].max(axis=1), bound_c), ("magnitude", d[:, 3], bound_m)):
                i = int(part.argmax())
                if part[i] > worst[label][0]:
                    worst[label] = (float(part[i]), f"[{name}] operands {E.hexes(o[i], 3)} -> {E.hexes(g[i], 4)}, exact form {E.hexes(E.reference(kind, o[i:i + 1])[0], 4)}")
                bad = np.flatnonzero(~(part <= bound))
                if len(bad):
                    j = int(bad[0])
                    failures.append(f"{kind} [{name}]: {len(bad)} of {len(o)} tuples beyond {bound} ulp ({label}); first: operands {E.hexes(o[j], 3)} -> "
                                    f"{E.hexes(g[j], 4)}, exact form {E.hexes(E.reference(kind, o[j:j + 1])[0], 4)}: {part[j]:.1f} ulp")
    for label in worst:
        print(f"{kind}: largest {label} distance {worst[label][0]:.1f} ulp at {worst[label][1]}")
    print(f"{kind}: {n_short} tuples on the short path (bounds {bound_c}, {bound_m}), {n_exact} on the exact path")
    assert n_short > 100000 and n_exact > 50000
    assert not failures, "\n".join(failures)


def test_pow_stays_within_the_derived_bound(probe):
    kind = "pow_exp2_log2"
    failures, worst, n_exempt, n_all = [], (0.0, 0.0, None), 0, 0
    for name in E.SET_NAMES[kind]:
        ops, got = E.operand_sets(kind)[name], probe.results(kind, name)
        err, bound, exempt = E.pow_judge(ops, got[:, 0])
        n_exempt, n_all = n_exempt + int(exempt.sum()), n_all + len(ops)
        assert not E.bits(got[:, 1:]).any(), "unused result slots are zero"
        judged = ~exempt
        bad = np.flatnonzero(judged & ~(err <= bound))
        if len(bad):
            j = int(bad[0])
            failures.append(f"{kind} [{name}]: {len(bad)} of {len(ops)} beyond the bound; first: tuple {j} (wave {j // 64}, lane {j % 64}), operands {E.hexes(ops[j], 2)} -> "
                            f"{E.hexes(got[j], 1)}: {err[j]:.1f} ulp, bound {bound[j]:.1f}")
        if judged.any():
            e = np.where(judged, err, 0.0)
            i = int(e.argmax())
            if e[i] > worst[0]:
                worst = (float(e[i]), float(e[i] / bound[i]), f"[{name}] x = {float(ops[i, 0])!r}, k = {float(ops[i, 1])!r} {E.hexes(ops[i], 2)} -> {E.hexes(got[i], 1)}")
            f = float((e / bound).max())
            print(f"{kind} [{name}]: {int(judged.sum())} judged, largest error {e.max():.1f} ulp, {f:.2f} of the bound")
    print(f"{kind}: largest error {worst[0]:.1f} ulp ({worst[1]:.2f} of its bound) at {worst[2]}; {n_exempt} of {n_all} results below 2^-120 exempt")
    assert not failures, "\n".join(failures)


def test_refusals_leave_the_results_alone(probe):
    ops = np.ascontiguousarray(E.operand_sets("div2")["inside"][:130])
    sentinel = np.float32(-12345.0)
    out = np.full((130, 4), sentinel)
    lib, ctx = probe.lib, probe.ctx
    p_ops, p_out = ops.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    assert lib.rxr_debug_exact_math(ctx, E.KIND["div2"], None, 128, p_out) == RXR_ERR_INVALID
    assert lib.rxr_debug_exact_math(ctx, E.KIND["div2"], p_ops, 128, None) == RXR_ERR_INVALID
    assert lib.rxr_debug_exact_math(None, E.KIND["div2"], p_ops, 128, p_out) == RXR_ERR_INVALID
    assert lib.rxr_debug_exact_math(ctx, E.KIND["div2"], p_ops, 0, p_out) == RXR_ERR_INVALID
    assert lib.rxr_debug_exact_math(ctx, len(E.KINDS), p_ops, 128, p_out) == RXR_ERR_INVALID
    assert lib.rxr_debug_exact_math(ctx, 0xFFFFFFFF, p_ops, 128, p_out) == RXR_ERR_INVALID
    for kind in E.DPP:
        for n in (1, 65, 127, 130):
            assert lib.rxr_debug_exact_math(ctx, E.KIND[kind], p_ops, n, p_out) == RXR_ERR_INVALID
        assert b"multiple of 64" in lib.rxr_last_error(ctx)
    assert (out == sentinel).all()
    # ... and the accepted call next to them writes its n tuples and nothing behind them
    assert lib.rxr_debug_exact_math(ctx, E.KIND["div2"], p_ops, 129, p_out) == 0
    assert E.exact_report("div2", "inside, first 129", ops[:129], out[:129], E.reference("div2", ops[:129])) is None
    assert (out[129:] == sentinel).all()
