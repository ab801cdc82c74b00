"""tests/exact_math_ref.py checked on the host, no GPU: the float32 operators the device is held to are IEEE-754 (equal to the float64
operator rounded once, denormals kept), every operand set holds what its name says, and the two bounds -- the relaxed
normalisation's and pow's -- come out of the references alone."""
import numpy as np
import pytest

from tests import exact_math_ref as E

IEEE_KINDS = E.DIVS + ["div1_static", "sqrt_exact"]


def is_denormal(x):
    return (E.bits(x) & 0x7F800000 == 0) & (E.bits(x) & 0x007FFFFF != 0)


def test_every_kind_has_its_sets_as_whole_waves():
    for kind in E.KINDS:
        sets = E.operand_sets(kind)
        assert list(sets) == E.SET_NAMES[kind]
        total = 0
        for name, ops in sets.items():
            assert ops.dtype == np.float32 and ops.shape[1] == 4 and len(ops) % E.WAVE == 0 and len(ops) > 0, (kind, name)
            assert not E.bits(ops[:, E.N_IN[kind]:]).any(), (kind, name, "unused operand slots are zero")
            total += len(ops)
        assert total <= E.MAX_TUPLES + (704 if kind == "sat_u32" else 0), (kind, total)
    # fixed seeds: building a set again gives the same bits
    again = E._sqrt_sets()
    for name, ops in E.operand_sets("sqrt_exact").items():
        assert np.array_equal(E.bits(again[name]), E.bits(ops)), name


@pytest.mark.parametrize("kind", IEEE_KINDS)
def test_float32_operators_are_the_float64_operators_rounded_once(kind):
    """`/` and sqrt from 53 to 24 bits round innocuously twice: numpy's float32 operator must equal the float64 one rounded to float32
    in every bit -- the evidence that the reference is IEEE and flushes no denormal"""
    n_denormal = 0
    for name, ops in E.operand_sets(kind).items():
        r32, r64 = E.reference(kind, ops), E.reference64(kind, ops)
        assert E.exact_report(kind, name, ops, r32, r64, what="float64 operator") is None
        n_denormal += int(is_denormal(r32[:, :E.N_OUT[kind]]).sum())
    print(f"{kind}: {sum(len(o) for o in E.operand_sets(kind).values())} tuples, {n_denormal} denormal results kept")


@pytest.mark.parametrize("kind", E.DIVS + E.NORMS + ["sqrt_exact"])
def test_inside_sets_are_whole_waves_inside_the_window(kind):
    s = E.operand_sets(kind)
    assert len(s["inside"]) == E.WAVES * E.WAVE
    assert E.short_path(kind, s["inside"]).all()
    if kind in E.DIVS:
        assert E.short_path(kind, s["hard quotients"]).all()
        v = np.abs(s["inside"][:, :E.N_IN[kind]])
        e, m = (E.bits(v) >> 23).astype(int) - 127, E.bits(v) & 0x7FFFFF
        assert set(np.unique(e)) == set(range(-40, 40))
        for mant in (0, 1, 0x7FFFFF):
            assert (m == mant).sum() > len(v) // 16
    if kind in E.NORMS:
        v = np.abs(s["inside"][:, :3])
        assert v.min() >= E.WIN_LO and (v.max(axis=1) / v.min(axis=1) <= 16.0).sum() >= len(v) // 2   # comparable magnitudes: half the set


@pytest.mark.parametrize("kind", E.DIVS)
def test_hard_quotients_sit_next_to_a_representable_value(kind):
    ops = E.operand_sets(kind)["hard quotients"]
    h = len(ops) // 2
    n, d = ops[:h, 0].astype(np.float64), ops[:h, E.N_IN[kind] - 1].astype(np.float64)
    q = (n / d).astype(np.float32).astype(np.float64)
    off = np.abs(n / d - q) / E.ulp32(q)               # how far the exact quotient is from its float32 rounding
    assert (off < 2.0 ** -20).sum() > h // 16            # exactly representable quotients (shift 0) ...
    assert (off > 0.25).sum() > h // 4                   # ... and ones well on the way to a midpoint
    m = E.bits(ops[h:, :E.N_IN[kind]]) & 0x7FFFFF
    num, den = m[:, :-1], m[:, -1]
    assert (((num == 0x7FFFFF).all(axis=1) & (den <= 1)) | ((num <= 1).all(axis=1) & (den == 0x7FFFFF))).all()
    assert {int(x) for x in np.unique(den)} == {0, 1, 0x7FFFFF}


@pytest.mark.parametrize("kind", E.DIVS)
def test_midpoint_quotients_are_as_close_to_a_midpoint_as_float32_allows(kind):
    """2^s N = M D + delta, |delta| <= 5: the exact quotient is within 5 / (2 D) < 2^-21 ulp of the midpoint between two float32 values,
    on either side -- where a reciprocal that is one ulp off, or a missing correction step, rounds the wrong way"""
    ops = E.operand_sets(kind)["midpoints"]
    assert len(ops) == E.WAVES * E.WAVE // 2 and E.short_path(kind, ops).all()
    d = ops[:, E.N_IN[kind] - 1].astype(np.float64)
    for j in range(E.N_IN[kind] - 1):
        exact = ops[:, j].astype(np.float64) / d           # (off by 2^-53 relative: 2^-29 ulp32)
        q = exact.astype(np.float32).astype(np.float64)
        off = (exact - q) / E.ulp32(exact) * np.sign(exact)
        assert (np.abs(off) > 0.5 - 2.0 ** -20).all()
        assert (off > 0).sum() > len(ops) // 4 and (off < 0).sum() > len(ops) // 4     # rounded down and rounded up
        assert len(np.unique(E.bits(ops[:, j]))) > len(ops) // 2


@pytest.mark.parametrize("kind", E.WITH_OUTSIDER)
def test_one_outsider_sets(kind):
    s = E.operand_sets(kind)
    lane, cat = E.outsider_lanes(kind)                   # (asserts: exactly one lane of every wave differs from the inside set)
    assert len(lane) == E.WAVES
    assert np.array_equal(lane, np.arange(E.WAVES) % E.WAVE) and set(lane) == set(range(E.WAVE))
    assert {(int(a), int(b)) for a, b in zip(lane, cat)} == {(a, b) for a in range(E.WAVE) for b in range(8)}   # every lane meets every category
    names = E.SQRT_OUTSIDERS if kind == "sqrt_exact" else E.OUTSIDERS
    rows = np.arange(E.WAVES) * E.WAVE + lane
    new, old = s["one outsider"][rows], s["inside"][rows]
    col = (E.bits(new) != E.bits(old)).argmax(axis=1)
    assert ((E.bits(new) != E.bits(old)).sum(axis=1) == 1).all()
    assert set(col) == set(range(E.N_IN[kind]))
    v = new[np.arange(len(new)), col]
    a = np.abs(v)
    lo = E.SQRT_LO if kind == "sqrt_exact" else E.WIN_LO
    is_cat = {"below the window": (a < lo) & (a >= np.float32(2.0 ** -126)), "above the window": (a > E.WIN_HI) & np.isfinite(a), "denormal": is_denormal(v),
              "+0": E.bits(v) == 0, "-0": E.bits(v) == 0x80000000, "+inf": E.bits(v) == 0x7F800000, "-inf": E.bits(v) == 0xFF800000, "NaN": np.isnan(v),
              "negative": (v < 0) & np.isfinite(v) & ~is_denormal(v)}
    for k, name in enumerate(names):
        assert is_cat[name][cat == k].all() and (cat == k).sum() == E.WAVES // 8, name
    short = E.short_path(kind, s["one outsider"])
    if kind == "normalize3_z":                           # an exactly-zero component is inside ITS window
        assert np.array_equal(short, np.isin(cat, [names.index("+0"), names.index("-0")]))
    else:
        assert not short.any()


@pytest.mark.parametrize("kind", E.DIVS)
def test_division_ends_hold_both_sides_of_both_window_ends(kind):
    ops = E.operand_sets(kind)["ends"]
    n_in = E.N_IN[kind]
    for x in (E.WIN_LO, E.up(E.WIN_LO), E.down(E.WIN_LO), E.WIN_HI, E.down(E.WIN_HI), E.up(E.WIN_HI)):
        for sign in (1, -1):
            v = np.float32(sign) * x
            assert (ops[:, 0] == v).any() and (ops[:, n_in - 1] == v).any(), float(v)
    short = E.short_path(kind, ops)
    assert short.any() and (~short).any()
    # a wave of its own for every combination of numerator and denominator end
    own = ops.reshape(-1, E.WAVE, 4)[0::2]
    assert (np.abs(own) == np.abs(own[:, :1])).all()
    assert len({(float(a), float(b)) for a, b in np.abs(own[:, 0][:, [0, n_in - 1]])}) == 36


@pytest.mark.parametrize("kind", E.NORMS)
def test_normalisation_ends_hold_the_ends_of_the_magnitude_window(kind):
    ops = E.operand_sets(kind)["ends"]
    m2 = E.squared_magnitude(ops)
    for x in (E.SQ_LO, E.up(E.SQ_LO), E.down(E.SQ_LO), E.SQ_HI, E.down(E.SQ_HI), E.up(E.SQ_HI)):
        assert (m2 == x).any(), float(x)
    a = np.abs(ops[:, :3])
    for x in (E.WIN_LO, E.up(E.WIN_LO), E.down(E.WIN_LO), E.WIN_HI, E.down(E.WIN_HI), E.up(E.WIN_HI)):
        assert (a == x).any(axis=0).all(), float(x)      # in every component
    short = E.short_path(kind, ops)
    assert short.any() and (~short).any()
    own_short = short[0::2]                              # the waves that hold one tuple in every lane
    at = lambda x: own_short[(m2.reshape(-1, E.WAVE)[0::2, 0] == x)]  # noqa: E731
    assert at(E.SQ_HI).any() and not at(E.up(E.SQ_HI)).any() and not at(E.down(E.SQ_LO)).any()
    if kind != "normalize3":                             # (2^-40, 0, 0): only the forms that accept a zero component reach m2 = 2^-80 on the short path
        assert at(E.SQ_LO).any()


def test_zero_patterns_and_unit_normals():
    ops = E.operand_sets("normalize3_z")["zero patterns"]
    b = E.bits(ops[:, :3])
    pat = np.where(b == 0, 1, np.where(b == 0x80000000, 2, 0))
    whole = pat.reshape(-1, E.WAVE, 3)
    uniform = (whole == whole[:, :1]).all(axis=(1, 2))
    assert {tuple(int(v) for v in p) for p in whole[uniform][:, 0]} == set(E.ZERO_PATTERNS)          # a wave of its own for all 27
    assert {tuple(int(v) for v in p) for p in pat} == set(E.ZERO_PATTERNS)
    short = E.short_path("normalize3_z", ops)
    assert short.sum() > len(short) // 4 and (~short).any()
    unit = E.operand_sets("normalize3_z")["unit normals"]
    m = np.sqrt(E.squared_magnitude(unit))
    assert m.max() <= 2.0 and (E.bits(unit[:, 1]) == 0).sum() > len(unit) // 8 and (E.bits(unit[:, 2]) == 0x80000000).sum() > len(unit) // 8


def test_square_root_ends():
    ops = E.operand_sets("sqrt_exact")["ends"][:, 0]
    for x in (E.SQRT_LO, E.up(E.SQRT_LO), E.down(E.SQRT_LO), E.FLT_MAX):
        assert (ops == x).any()
    b = E.bits(ops)
    have = {(int(e), int(m)) for e, m in zip((b >> 23).astype(int) - 127, b & 0x7FFFFF)}
    assert {(e, m) for e in range(-96, 128) for m in (0, 1, 0x7FFFFF)} <= have
    r = np.sqrt(ops.astype(np.float64))
    square = (r == np.rint(np.ldexp(r, 60)) / 2.0 ** 60) & (r.astype(np.float32) == r) & (ops > 0)   # exact roots
    assert square.sum() >= 4096
    short = E.short_path("sqrt_exact", E.operand_sets("sqrt_exact")["ends"])
    assert short[0] and not short[1] and not short[2]    # the ends inside; with the lower neighbour in one lane; the lower neighbour alone


@pytest.mark.parametrize("kind", E.DIVS + E.NORMS + ["sqrt_exact"])
def test_specials_hold_every_class_and_denormal_results(kind):
    ops = E.operand_sets(kind)["specials"]
    v = ops[:, :E.N_IN[kind]]
    assert (E.bits(v) == 0).any() and (E.bits(v) == 0x80000000).any() and np.isposinf(v).any() and np.isneginf(v).any()
    assert len(np.unique(E.bits(v[np.isnan(v)]))) > 3 and is_denormal(v).any()
    r = E.reference(kind, ops)[:, :E.N_OUT[kind]]
    n_den = int(is_denormal(r).sum())
    assert n_den > 100 or kind == "sqrt_exact", "the reference keeps denormal results"      # (no square root is denormal)
    assert np.isnan(r).any() and np.isinf(r).any() and (E.bits(r) == 0x80000000).any()
    if kind in E.DIVS:
        n, d = v[:, 0], v[:, -1]
        with np.errstate(all="ignore"):
            assert ((n == 0) & (d == 0)).any() and (np.isinf(n) & np.isinf(d)).any()
            for sn in (False, True):
                for sd in (False, True):
                    assert (np.isfinite(n) & (n != 0) & (np.signbit(n) == sn) & (d == 0) & (np.signbit(d) == sd)).any()
            assert (np.isinf(r[:, 0]) & np.isfinite(n) & np.isfinite(d) & (d != 0)).any()          # quotients that overflow
    print(f"{kind}: {len(ops)} special tuples, {n_den} denormal results")


def test_static_sets_are_what_the_call_sites_claim():
    s = E.operand_sets("div1_static")
    px = s["pixel centres"]
    k, w = px[:, 0] - np.float32(0.5), px[:, 1]
    assert (k == np.rint(k)).all() and k.min() == 0 and k.max() == 32767 and w.min() == 1 and w.max() == 32767
    assert E.in_window(px[:, :2]).all()
    by = s["bytes over 255"]
    assert np.array_equal(by[:, 0], np.arange(256, dtype=np.float32)) and (by[:, 1] == 255).all()
    z = s["one over z"]
    assert (z[:, 0] == 1).all() and E.in_window(z[:, 1]).all() and (np.abs(z[:, 1]) == E.WIN_LO).any() and (np.abs(z[:, 1]) == E.WIN_HI).any()


def test_sat_u32_reference_and_sets():
    x = np.float32([np.nan, -1.0, -0.0, 0.0, 0.99, 1.0, 255.9, 256.0, 2.0 ** 31, 4294967040.0, 2.0 ** 32, np.inf, -np.inf, 3e38])
    assert list(E.sat_u32(x)) == [0, 0, 0, 0, 0, 1, 255, 256, 1 << 31, 4294967040, 0xFFFFFFFF, 0xFFFFFFFF, 0, 0xFFFFFFFF]
    s = E.operand_sets("sat_u32")
    assert len(s["sweep"]) == 1 << 20
    b = E.bits(s["sweep"][:, 0]).astype(np.int64)
    assert (np.diff(b) == 4096).all() and b[0] < 4096 and b[-1] > (1 << 32) - 4096
    have = set(E.bits(s["anchors"][:, 0]).tolist())
    for a in E.SAT_ANCHORS:
        assert {(a + k) & 0xFFFFFFFF for k in range(-16, 17)} <= have


def test_wave_references():
    v = np.zeros((128, 4), np.float32)
    v[:, 0] = np.arange(128) % 64
    v[64 + 17, 0] = 1000.0
    r = E.reference("wave_max_nonneg", v)[:, 0]
    assert (r[:64] == 63).all() and (r[64:] == 1000).all()
    c = np.zeros((64, 4), np.float32)
    c[:, 0] = E.from_bits(np.full(64, 0xC0000000))
    got = E.bits(E.reference("wave_inclusive_add", c)[:, 0])
    assert list(got[:4]) == [0xC0000000, 0x80000000, 0x40000000, 0x00000000]                   # wraps mod 2^32
    for kind in E.DPP:
        for ops in E.operand_sets(kind).values():
            assert kind == "wave_inclusive_add" or not (np.isnan(ops).any() or np.signbit(ops[:, 0]).any())
    m = E.operand_sets("wave_max_nonneg")["random"][:, 0].reshape(-1, 64)
    assert set(m.argmax(axis=1)) == set(range(64))        # the maximum in every lane position


def test_relaxed_bound_comes_from_the_reference_alone():
    """x * inv, m2 * inv with inv the correctly rounded 1 / sqrt(m2) moved by -1, 0, +1 ulp, against the exact form.  A v_rsq_f32 that is
    in effect correctly rounded gives the shift-0 figures; the ISA manual's 1 ulp gives the bound the device is held to.  Analytic
    ceiling: inv within (1/2 + 1) ulp <= 3 * 2^-24 relative, one rounding of the product 2^-24, the exact form's own two roundings
    2 * 2^-24: 6 * 2^-24 relative, at most 6 ulp32."""
    c0, m0 = E.relaxed_bound((0,))
    c1, m1 = E.relaxed_bound()
    print(f"relaxed model: correctly rounded rsq {c0:.1f} ulp per component, {m0:.1f} magnitude; within 1 ulp {c1:.1f} and {m1:.1f}")
    assert 0.0 < c0 <= c1 <= 6.0 and 0.0 < m0 <= m1 <= 6.0
    assert (c0, m0) == (2.0, 1.0) and (c1, m1) == (4.0, 3.0)
    n = sum(int(E.sq_in_window(E.squared_magnitude(E.operand_sets("normalize3_relaxed")[s])).sum()) for s in E.RELAXED_SHORT_SETS)
    assert n > 100000


def test_pow_bound_holds_for_a_float32_emulation():
    """3 + 7 ln 2 |y| ulp32 of the float64 2^y, y = k log2 x: the sequence in numpy float32 (glibc's log2f and exp2f, far inside the 3 ulp
    the bound allows each) must lie inside it"""
    sets = E.operand_sets("pow_exp2_log2")
    worst, frac, n_all, n_exempt = 0.0, 0.0, 0, 0
    for name, ops in sets.items():
        assert (ops[:, 0] > 0).all() and (ops[:, 0] <= 1).all() and (ops[:, 1] >= 1).all() and (ops[:, 1] <= E.K_MAX).all(), name
        err, bound, exempt = E.pow_judge(ops, E.pow_emulation(ops))
        judged = ~exempt
        assert (err[judged] <= bound[judged]).all(), name
        if judged.any():
            worst, frac = max(worst, float(err[judged].max())), max(frac, float((err[judged] / bound[judged]).max()))
        n_all, n_exempt = n_all + len(ops), n_exempt + int(exempt.sum())
    print(f"pow emulation: largest error {worst:.1f} ulp, {frac:.2f} of the bound; {n_exempt} of {n_all} results below 2^-120 exempt")
    assert 2 * n_exempt <= n_all
    assert is_denormal(sets["denormal x"][:, 0]).all() and (sets["x = 1"][:, 0] == 1).all()
    assert (sets["k = 6"][:, 1] == 6).all() and sets["k to 2048"][:, 1].max() == E.K_MAX and sets["bounded result"][:, 1].max() > 1024
    ref, y, _, exempt = E.pow_reference(sets["bounded result"])
    assert not exempt.any() and y.min() < -110
