"""rusterix_amd/csrc/rxr_exact_math.h held to IEEE-754 as the host computes it: the references, the operand sets and the verdicts that
tests/test_exact_math_cpu.py (no GPU) and tests/test_gpu_exact_math_ref.py (the device, through rxr_debug_exact_math) share.  numpy only.

rxr_selftest_math compares every short sequence with what hipcc makes of the plain operator in the same translation unit: both sides
move together under a build-flag change.  Here the operands are chosen on the host, every result comes back float by float, and the
expected value is numpy's float32 operator (x86 divss / sqrtss; tests/test_exact_math_cpu.py shows it equal to the float64 operator
rounded once, denormals kept).

A tuple is four float32 operand slots and four result slots (rxr_debug.h lists them per kind; unused slots are zero).  Tuple i is
lane i % 64 of wave i / 64, and the helpers vote per wave: every set is built as whole waves, so a set decides which operands
share a vote.

References: division and square root are the float32 operators; normalize3* form m2 = (x*x + y*y) + z*z in float32, unfused, then
sqrt and three divisions; sat_u32 is Rust's `as u32` written out; the wave maximum is max per 64, the prefix sum cumsum mod 2^32 per
64.  normalize3_relaxed is measured against the exact form, pow_exp2_log2 against float64 2^(k log2 x); both in ulp32, the float32
spacing at the reference value."""
import functools

import numpy as np

KINDS = ["div1_known", "div1_static", "div2", "div2_pre", "div3", "div3_self", "normalize3", "normalize3_z", "normalize3_relaxed", "sqrt_exact",
         "pow_exp2_log2", "sat_u32", "wave_max_nonneg", "wave_inclusive_add"]            # the order of rxr_debug.h's table
KIND = {k: i for i, k in enumerate(KINDS)}
N_IN = dict(div1_known=2, div1_static=2, div2=3, div2_pre=3, div3=4, div3_self=4, normalize3=3, normalize3_z=3, normalize3_relaxed=3, sqrt_exact=1,
            pow_exp2_log2=2, sat_u32=1, wave_max_nonneg=1, wave_inclusive_add=1)
N_OUT = dict(div1_known=1, div1_static=1, div2=2, div2_pre=2, div3=3, div3_self=4, normalize3=4, normalize3_z=3, normalize3_relaxed=4, sqrt_exact=1,
             pow_exp2_log2=1, sat_u32=1, wave_max_nonneg=1, wave_inclusive_add=1)
DIVS = ["div1_known", "div2", "div2_pre", "div3", "div3_self"]
NORMS = ["normalize3", "normalize3_z", "normalize3_relaxed"]
EXACT = [k for k in KINDS if k not in ("normalize3_relaxed", "pow_exp2_log2")]           # equal to the reference in every bit
DPP = ["wave_max_nonneg", "wave_inclusive_add"]                                          # every lane active: n % 64 == 0

DIV_SETS = ["inside", "hard quotients", "midpoints", "ends", "one outsider", "specials"]
NORM_SETS = ["inside", "ends", "one outsider", "specials", "zero patterns", "unit normals"]
SET_NAMES = {**{k: DIV_SETS for k in DIVS}, **{k: NORM_SETS for k in NORMS},
             "div1_static": ["pixel centres", "bytes over 255", "one over z"],
             "sqrt_exact": ["inside", "ends", "one outsider", "specials"],
             "pow_exp2_log2": ["k = 6", "small k", "bounded result", "k to 2048", "denormal x", "x = 1"],
             "sat_u32": ["sweep", "anchors"],
             "wave_max_nonneg": ["random", "edges"],
             "wave_inclusive_add": ["small counts", "words"]}
WITH_OUTSIDER = DIVS + ["normalize3", "normalize3_z", "sqrt_exact"]   # (the relaxed form's VALUE depends on the vote: not a property of it)

WAVE = 64
WAVES = 1024                       # waves of an inside set: 65 536 tuples
MAX_TUPLES = 1 << 20               # per kind; sat_u32's sweep alone has that many, its 704 anchors come on top
WIN_LO, WIN_HI = np.float32(2.0 ** -40), np.float32(2.0 ** 40)
SQ_LO, SQ_HI = np.float32(2.0 ** -80), np.float32(2.0 ** 80)
SQRT_LO = np.float32(2.0 ** -96)
FLT_MAX = np.finfo(np.float32).max
INF32 = np.float32(np.inf)
OUTSIDERS = ["below the window", "above the window", "denormal", "+0", "-0", "+inf", "-inf", "NaN"]
SQRT_OUTSIDERS = ["below the window", "denormal", "+0", "-0", "+inf", "-inf", "NaN", "negative"]
SPECIAL_BITS = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00001, 0x7F800001, 0x00000001, 0x80000001, 0x007FFFFF,
                         0x807FFFFF, 0x00800000, 0x80800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x3F800000, 0xBF800000], np.uint32)


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def from_bits(b):
    return np.ascontiguousarray(np.asarray(b, np.int64) & 0xFFFFFFFF, np.uint32).view(np.float32)


def up(x):
    return np.nextafter(np.float32(x), INF32)


def down(x):
    return np.nextafter(np.float32(x), -INF32)


def pack(e, m, s=0):
    """sign, unbiased exponent, 23 mantissa bits -> float32"""
    return from_bits((np.asarray(s, np.int64) << 31) | ((np.asarray(e, np.int64) + 127) << 23) | np.asarray(m, np.int64))


def shifted(x, k):
    """x moved by k ulp away from zero (towards it for negative k); the caller keeps clear of zero and infinity"""
    return from_bits(bits(x).astype(np.int64) + k)


def _rng(tag):
    return np.random.default_rng([0x45584D54, tag])


def _mantissas(r, shape):
    """0, 1, 0x7FFFFF (an eighth each) and random"""
    m, pick = r.integers(0, 1 << 23, shape), r.integers(0, 8, shape)
    return np.where(pick == 0, 0, np.where(pick == 1, 1, np.where(pick == 2, 0x7FFFFF, m)))


def inside_values(r, shape, lo_e=-40, hi_e=39):
    """both signs, exponents lo_e..hi_e: with the defaults every float32 of the division window but 2^40 itself"""
    return pack(r.integers(lo_e, hi_e + 1, shape), _mantissas(r, shape), r.integers(0, 2, shape))


def ulp32(ref):
    """the spacing of float32 at |ref| (float64), floored at 2^-149; the spacing at FLT_MAX beyond it (as tests/libm_ref.py)"""
    ref = np.asarray(ref, np.float64)
    with np.errstate(all="ignore"):
        _, ex = np.frexp(np.where(np.isfinite(ref) & (ref != 0), np.abs(ref), 2.0 ** -126))
    return np.exp2(np.clip(ex - 1, -126, 127).astype(np.float64) - 23.0)


# ---- references --------------------------------------------------------------------------------------------------------------------
def in_window(x):
    with np.errstate(all="ignore"):
        a = np.abs(np.asarray(x, np.float32))
        return (a >= WIN_LO) & (a <= WIN_HI)


def squared_magnitude(ops):
    o = np.asarray(ops, np.float32)
    with np.errstate(all="ignore"):
        return (o[:, 0] * o[:, 0] + o[:, 1] * o[:, 1]) + o[:, 2] * o[:, 2]


def sq_in_window(m2):
    with np.errstate(all="ignore"):
        return (m2 >= SQ_LO) & (m2 <= SQ_HI)


def sat_u32(x):
    """Rust's `x as u32`: NaN -> 0, truncate toward zero, clamp to [0, 2^32 - 1]"""
    x = np.asarray(x, np.float32).astype(np.float64)
    t = np.clip(np.trunc(np.where(np.isnan(x), 0.0, x)), 0.0, 4294967295.0)
    return t.astype(np.uint64).astype(np.uint32)


def reference(kind, ops):
    """[n][4] float32 operands -> [n][4] float32, the bits the device must return (an integer result as its bits; unused slots zero).
    For normalize3_relaxed: the exact form."""
    o = np.ascontiguousarray(ops, np.float32)
    a, b, c, d = o[:, 0], o[:, 1], o[:, 2], o[:, 3]
    out = np.zeros((len(o), 4), np.float32)
    with np.errstate(all="ignore"):
        if kind in ("div1_known", "div1_static"):
            out[:, 0] = a / b
        elif kind in ("div2", "div2_pre"):
            out[:, 0], out[:, 1] = a / c, b / c
        elif kind in ("div3", "div3_self"):
            out[:, 0], out[:, 1], out[:, 2] = a / d, b / d, c / d
            if kind == "div3_self":
                out[:, 3] = d / d
        elif kind in NORMS:
            m = np.sqrt(squared_magnitude(o))
            out[:, 0], out[:, 1], out[:, 2] = a / m, b / m, c / m
            if kind != "normalize3_z":
                out[:, 3] = m
        elif kind == "sqrt_exact":
            out[:, 0] = np.sqrt(a)
        elif kind == "sat_u32":
            out[:, 0] = sat_u32(a).view(np.float32)
        elif kind == "wave_max_nonneg":
            out[:, 0] = np.repeat(a.reshape(-1, WAVE).max(axis=1), WAVE)
        elif kind == "wave_inclusive_add":
            s = np.cumsum(bits(a).astype(np.uint64).reshape(-1, WAVE), axis=1) & 0xFFFFFFFF
            out[:, 0] = s.astype(np.uint32).reshape(-1).view(np.float32)
        else:
            raise KeyError(kind)
    return out


def reference64(kind, ops):
    """the float64 operator rounded once to float32, for the kinds made of `/` and sqrt alone (the innocuous double rounding: 53 bits
    to 24): what tests/test_exact_math_cpu.py holds the float32 operators to"""
    with np.errstate(all="ignore"):   # (a signalling NaN among the raw bit patterns)
        o = np.asarray(ops, np.float32).astype(np.float64)
    a, b, c, d = o[:, 0], o[:, 1], o[:, 2], o[:, 3]
    out = np.zeros((len(o), 4), np.float32)
    with np.errstate(all="ignore"):
        if kind in ("div1_known", "div1_static"):
            out[:, 0] = a / b
        elif kind in ("div2", "div2_pre"):
            out[:, 0], out[:, 1] = a / c, b / c
        elif kind in ("div3", "div3_self"):
            out[:, 0], out[:, 1], out[:, 2] = a / d, b / d, c / d
            if kind == "div3_self":
                out[:, 3] = d / d
        elif kind == "sqrt_exact":
            out[:, 0] = np.sqrt(a)
        else:
            raise KeyError(kind)
    return out


def normalize3_f64(ops):
    """v / |v| and |v| in float64 from the float32 operands: [n][4]"""
    o = np.asarray(ops, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        m = np.sqrt((o[:, 0] * o[:, 0] + o[:, 1] * o[:, 1]) + o[:, 2] * o[:, 2])
        return np.stack([o[:, 0] / m, o[:, 1] / m, o[:, 2] / m, m], 1)


def short_path(kind, ops):
    """[waves] bool: the host's model of the helper's vote (every lane of the wave inside the window).  Used to COUNT what a set holds
    and to tell the relaxed form's two paths apart; no exact result depends on it."""
    o = np.asarray(ops, np.float32)
    with np.errstate(all="ignore"):
        if kind in DIVS:
            ok = np.all(in_window(o[:, :N_IN[kind]]), axis=1)
        elif kind in NORMS:
            ok = sq_in_window(squared_magnitude(o))
            a = np.abs(o[:, :3])
            if kind == "normalize3":
                ok &= np.all(a >= WIN_LO, axis=1)
            elif kind == "normalize3_z":
                ok &= np.all((a == 0) | (a >= WIN_LO), axis=1)
        elif kind == "sqrt_exact":
            ok = (o[:, 0] >= SQRT_LO) & (o[:, 0] < INF32) & ~np.signbit(o[:, 0])
        else:
            raise KeyError(kind)
    return ok.reshape(-1, WAVE).all(axis=1)


# ---- verdicts ----------------------------------------------------------------------------------------------------------------------
def hexes(row, n):
    return "(" + ", ".join(f"0x{int(v):08X}" for v in bits(row)[:n]) + ")"


def differing(got, ref):
    """[n] bool: tuples with a slot that differs in any bit (any NaN stands for a NaN)"""
    got, ref = np.asarray(got, np.float32), np.asarray(ref, np.float32)
    return ((bits(got) != bits(ref)) & ~(np.isnan(got) & np.isnan(ref))).any(axis=1)


def exact_report(kind, name, ops, got, ref, what="reference"):
    """None, or the failure text: the set, how many tuples differ, and the first of them with its wave and lane, in hex"""
    rows = np.flatnonzero(differing(got, ref))
    if len(rows) == 0:
        return None
    i = int(rows[0])
    return (f"{kind} [{name}]: {len(rows)} of {len(ops)} tuples differ from the {what}; first: tuple {i} (wave {i // WAVE}, lane {i % WAVE}), "
            f"operands {hexes(ops[i], N_IN[kind])}, device {hexes(got[i], 4)}, {what} {hexes(ref[i], 4)}")


# ---- operand sets ------------------------------------------------------------------------------------------------------------------
def place(kind, v4):
    """(n0, n1, n2, d) -> the operand slots of a division kind"""
    o = np.zeros((len(v4), 4), np.float32)
    if N_IN[kind] == 2:
        o[:, 0], o[:, 1] = v4[:, 0], v4[:, 3]
    elif N_IN[kind] == 3:
        o[:, 0], o[:, 1], o[:, 2] = v4[:, 0], v4[:, 1], v4[:, 3]
    else:
        o[:] = v4
    return o


def placed_waves(tuples, filler):
    """Two waves per tuple: the tuple in all 64 lanes (its own vote; the lane index sets the signs of the slots, one bit each), and a
    wave of `filler` (inside tuples) with lane i % 64 replaced by it (one vote for 63 ordinary tuples and this one)."""
    tuples = np.asarray(tuples, np.float32)
    assert len(filler) >= len(tuples) * WAVE
    lanes = np.arange(WAVE)
    out = []
    for i, t in enumerate(tuples):
        own = np.tile(t, (WAVE, 1))
        for c in range(4):
            flip = ((lanes >> c) & 1).astype(bool) & (bits(own[:, c]) != 0)      # (an unused slot stays +0)
            own[:, c] = np.where(flip, -own[:, c], own[:, c])
        mixed = filler[i * WAVE:(i + 1) * WAVE].copy()
        mixed[i % WAVE] = t
        out += [own, mixed]
    return np.concatenate(out)


def outsider_values(r, category, n, sqrt=False):
    sign = r.integers(0, 2, n)
    if category == "below the window":
        return pack(r.integers(-126, -96 if sqrt else -40, n), r.integers(0, 1 << 23, n), 0 if sqrt else sign)
    if category == "above the window":
        return pack(r.integers(41, 128, n), r.integers(0, 1 << 23, n), sign)
    if category == "denormal":
        return from_bits(r.integers(1, 1 << 23, n) | ((0 if sqrt else sign) << 31))
    if category == "NaN":
        return from_bits(0x7FC00000 | r.integers(0, 1 << 22, n) | (sign << 31))
    if category == "negative":
        return pack(r.integers(-96, 128, n), r.integers(0, 1 << 23, n), 1)
    return np.full(n, from_bits({"+0": 0x00000000, "-0": 0x80000000, "+inf": 0x7F800000, "-inf": 0xFF800000}[category]))


def with_one_outsider(r, inside, n_in, categories):
    """every wave of `inside` again with ONE slot of ONE lane replaced: lane w % 64 walks 0..63, the category cycles so that every lane
    meets every category.  Returns (operands, [waves] category index)."""
    o = inside.copy()
    w = np.arange(len(o) // WAVE)
    lane, cat, col = w % WAVE, (w + w // WAVE) % len(categories), (9 * (w // WAVE) + (w % WAVE) // 8) % n_in
    for k, name in enumerate(categories):
        sel = np.flatnonzero(cat == k)
        o[sel * WAVE + lane[sel], col[sel]] = outsider_values(r, name, len(sel), sqrt=n_in == 1)
    return o, cat


def raw_values(r, shape):
    """raw bit patterns, a quarter of them from the list of special values"""
    b = r.integers(0, 1 << 32, shape)
    return from_bits(np.where(r.integers(0, 4, shape) == 0, SPECIAL_BITS[r.integers(0, len(SPECIAL_BITS), shape)], b))


def near_midpoint_numerators(D, delta):
    """For odd 24-bit denominators D and odd delta: the 24-bit N with 2^s N = M D + delta for an odd M of 25 bits (s = 24: quotient in
    [1, 2), s = 25: in [1/2, 1)) -- N / D lies |delta| / (2 D), about |delta| 2^-25 ulp, off the midpoint between two float32 values:
    as close as a quotient of float32 values gets to one.  M = -delta / D mod 2^s.  Returns (N, found); int64 arithmetic throughout."""
    inv = D.astype(np.uint64)
    for _ in range(6):                                   # Newton's iteration for 1 / D mod 2^64
        inv = inv * (np.uint64(2) - D.astype(np.uint64) * inv)
    N, found = np.zeros_like(D), np.zeros(len(D), bool)
    for s in (25, 24):
        M = ((-delta).astype(np.uint64) * inv).astype(np.int64) & ((1 << s) - 1)
        M = M + (1 << 24) if s == 24 else M
        n = (M * D + delta) >> s
        ok = (M >= 1 << 24) & (M < 1 << 25) & (((M * D + delta) & ((1 << s) - 1)) == 0) & (n >= 1 << 23) & (n < 1 << 24) & ~found
        N, found = np.where(ok, n, N), found | ok
    return N, found


def _midpoint_v4():
    """whole waves inside the window whose three quotients all lie next to a rounding midpoint; exponents and signs at random"""
    r = _rng(11)
    n = WAVES * WAVE // 2
    D = r.integers(1 << 23, 1 << 24, 24 * n) | 1
    N = []
    ok = np.ones(len(D), bool)
    for j in range(3):
        Nj, found = near_midpoint_numerators(D, r.choice(np.array([-5, -3, -1, 1, 3, 5]), len(D)))
        N.append(Nj)
        ok &= found
    assert ok.sum() >= n
    m = np.stack(N + [D], 1)[ok][:n] & 0x7FFFFF
    e_d = r.integers(-40, 40, n)
    e_n = r.integers(-40, 40, (n, 3))
    return pack(np.concatenate([e_n, e_d[:, None]], 1), m, r.integers(0, 2, (n, 4)))


@functools.lru_cache(maxsize=None)
def _division_v4():
    """(n0, n1, n2, d) of the division sets; the kinds take their slots out of the same tuples"""
    r = _rng(1)
    n = WAVES * WAVE
    inside = inside_values(r, (n, 4))
    # hard quotients: n = fl(q d) moved by -2..+2 ulp (quotients next to a representable value and next to a rounding midpoint) ...
    h = n // 2
    d = inside_values(r, h, -28, 28)
    q = inside_values(r, (h, 3), -10, 10)
    hard_a = np.concatenate([shifted(q * d[:, None], r.integers(-2, 3, (h, 3))), d[:, None]], axis=1)
    # ... and mantissas of all ones against mantissas 0 and 1, both ways round
    e, s = r.integers(-40, 40, (h, 4)), r.integers(0, 2, (h, 4))
    ones_up = (np.arange(h) & 1).astype(bool)[:, None]
    low = r.integers(0, 2, (h, 4))
    m = np.where(ones_up, np.where(np.arange(4) < 3, 0x7FFFFF, low), np.where(np.arange(4) < 3, low, 0x7FFFFF))
    hard = np.concatenate([hard_a, pack(e, m, s)])
    # ends: |x| exactly 2^-40 and 2^40 and the neighbours on both sides of each
    v = np.float32([WIN_LO, up(WIN_LO), down(WIN_LO), WIN_HI, down(WIN_HI), up(WIN_HI)])
    t = np.float32([[v[i], v[(i + 1) % 6], v[(j + 2) % 6], v[j]] for i in range(6) for j in range(6)])
    ends = placed_waves(np.concatenate([t, t[:, [1, 0, 2, 3]]]), inside)
    # specials: raw bit patterns, then whole waves of one named case each
    raw = raw_values(r, (n, 4))
    k = 16 * WAVE
    x = inside_values(r, (k, 4), -100, 100)
    zero, inf = from_bits(r.integers(0, 2, (k, 4)) << 31), from_bits(0x7F800000 | (r.integers(0, 2, (k, 4)) << 31))
    den = from_bits(r.integers(1, 1 << 23, (k, 4)) | (r.integers(0, 2, (k, 4)) << 31))
    col_d = np.arange(4) == 3
    named = [zero,                                                     # 0 / 0
             inf,                                                      # inf / inf
             np.where(col_d, zero, x),                                 # x / 0, every combination of signs
             np.where(col_d, x, zero),                                 # 0 / x
             np.where(col_d, x, inf), np.where(col_d, inf, x),         # inf / x, x / inf
             np.where(col_d, den, x), np.where(col_d, x, den), den,    # x / denormal, denormal / x, denormal / denormal
             np.where(col_d, inside_values(r, (k, 4), -126, -30), inside_values(r, (k, 4), 100, 127)),       # quotients that overflow
             np.where(col_d, inside_values(r, (k, 4), 10, 60), inside_values(r, (k, 4), -126, -70))]         # quotients in the denormal range
    specials = np.concatenate([raw] + named)
    return {"inside": inside, "hard quotients": hard, "midpoints": _midpoint_v4(), "ends": ends, "specials": specials}


def _division_sets(kind):
    v4 = _division_v4()
    sets = {name: place(kind, a) for name, a in v4.items()}
    sets["one outsider"], _ = with_one_outsider(_rng(2), sets["inside"], N_IN[kind], OUTSIDERS)
    return {name: sets[name] for name in DIV_SETS}


def _vec(a):
    o = np.zeros((len(a), 4), np.float32)
    o[:, :3] = a
    return o


ZERO_PATTERNS = [(a, b, c) for a in range(3) for b in range(3) for c in range(3)]      # per component: 0 non-zero, 1 +0, 2 -0


def _normalize_sets():
    r = _rng(3)
    n = WAVES * WAVE
    h = n // 2
    # inside: independent exponents -40..38 (m2 <= 3 * 2^78), and comparable magnitudes, the common case
    free = inside_values(r, (h, 3), -40, 38)
    x = inside_values(r, h, -38, 36)
    ratio = lambda: (np.float32(0.25) + r.integers(0, 1024, h).astype(np.float32) / np.float32(256.0)) * np.where(r.integers(0, 2, h) == 0, np.float32(-1), np.float32(1))  # noqa: E731
    inside = _vec(np.concatenate([free, np.stack([x, x * ratio(), x * ratio()], 1)]))
    # ends: m2 exactly 2^-80 and 2^80 and the neighbours of each, and components at the ends of their own window
    p = lambda e, f=1.0: np.float32(f * 2.0 ** e)  # noqa: E731
    t = [(p(-40), 0, 0),                       # m2 = 2^-80
         (down(p(-40)), p(-52), 0),            # its lower neighbour: fl(x^2) = 2^-80 (1 - 2^-23), + 2^-104
         (p(-40), p(-52, 1.5), 0),             # its upper neighbour: 2^-80 + 2.25 * 2^-104 rounds up
         (p(40), 0, 0),                        # m2 = 2^80
         (p(40), p(-40), p(-40)),              # the same with every component inside its window
         (down(p(40)), p(28), p(-40)),         # its lower neighbour: 2^80 (1 - 2^-23) + 2^56
         (p(40), p(28, 1.5), p(-40)),          # its upper neighbour: 2^80 + 2.25 * 2^56 rounds up
         (p(-40), p(-40), p(-40)), (up(p(-40)), p(-40), p(-40)), (down(p(-40)), p(-40), p(-40)), (down(p(-40)), 0, 0),
         (p(39), p(39), p(39)), (down(p(40)), p(-40), 0), (up(p(40)), 0, 0), (p(39, 1.5), p(39), p(-40))]
    t = np.float32(t)
    ends = placed_waves(_vec(np.concatenate([t, t[:, [2, 0, 1]], t[:, [1, 2, 0]]])), inside)
    # specials: raw bit patterns, then whole waves of zero, denormal, infinite and NaN magnitudes
    k = 16 * WAVE
    zero = from_bits(r.integers(0, 2, (k, 3)) << 31)
    den = from_bits(r.integers(1, 1 << 23, (k, 3)) | (r.integers(0, 2, (k, 3)) << 31))
    one = np.arange(3) == r.integers(0, 3, k)[:, None]
    y = inside_values(r, (k, 3), -30, 30)
    inf, nan = from_bits(0x7F800000 | (r.integers(0, 2, (k, 3)) << 31)), from_bits(0x7FC00000 | r.integers(0, 1 << 22, (k, 3)))
    named = [zero, den, np.where(one, den, zero), np.where(one, inf, y), inf, np.where(one, nan, y),
             inside_values(r, (k, 3), 41, 62),            # m2 above its window, finite
             inside_values(r, (k, 3), 64, 127),           # m2 overflows
             inside_values(r, (k, 3), -62, -41),          # m2 below its window, normal
             inside_values(r, (k, 3), -75, -64),          # m2 denormal or zero
             inside_values(r, (k, 3), -126, -76)]         # m2 zero: x / 0
    specials = _vec(np.concatenate([raw_values(r, (n // 2, 3))] + named))
    # zero patterns: every pattern of exactly-zero components with both signs of zero; whole waves of one pattern each, then mixed waves
    w = 27 * 8
    pat = np.array(ZERO_PATTERNS)[np.concatenate([np.repeat(np.arange(w) % 27, WAVE), r.integers(0, 27, w * WAVE)])]
    val = inside_values(r, pat.shape, -40, 38)
    zeros = _vec(np.where(pat == 0, val, np.where(pat == 1, np.float32(0.0), np.float32(-0.0))).astype(np.float32))
    # unit-length-ish normals on a grid of 1 / 1024, a zero y or a negative-zero z in a quarter each
    m = 256 * WAVE
    g = (r.integers(0, 2048, (m, 3)) - 1024).astype(np.float32) / np.float32(1024.0)
    g[:, 1] = np.where(r.integers(0, 4, m) == 0, np.float32(0.0), g[:, 1])
    g[:, 2] = np.where(r.integers(0, 4, m) == 0, np.float32(-0.0), g[:, 2])
    sets = {"inside": inside, "ends": ends, "specials": specials, "zero patterns": zeros, "unit normals": _vec(g)}
    sets["one outsider"], _ = with_one_outsider(_rng(4), inside, 3, OUTSIDERS)
    return {name: sets[name] for name in NORM_SETS}


def _first(a):
    o = np.zeros((len(a), 4), np.float32)
    o[:, 0] = a
    return o


def _sqrt_sets():
    r = _rng(5)
    n = WAVES * WAVE
    inside = pack(r.integers(-96, 128, n), _mantissas(r, n))
    lo = [SQRT_LO, up(SQRT_LO), FLT_MAX, down(FLT_MAX)]
    a = np.resize(np.float32(lo), WAVE)                     # the ends of the window, inside
    b = a.copy()
    b[5] = down(SQRT_LO)                                    # ... and the lower neighbour among them
    k = r.integers(1, 4096, 4096).astype(np.float32)        # perfect squares (k^2 < 2^24 is exact) times 4^j, and both neighbours
    sq = np.ldexp(k * k, 2 * r.integers(-40, 50, 4096)).astype(np.float32)
    e = np.repeat(np.arange(-96, 128), 3)                   # one value for each of the three mantissas at every exponent of the window
    per_exp = pack(e, np.tile([0, 1, 0x7FFFFF], 224))
    ends = np.concatenate([a, b, np.full(WAVE, down(SQRT_LO)), sq, shifted(sq, -1), shifted(sq, 1), per_exp])
    ends = np.concatenate([ends, np.ones(-len(ends) % WAVE, np.float32)])
    specials = np.concatenate([raw_values(r, n), np.abs(raw_values(r, n))])
    sets = {"inside": _first(inside), "ends": _first(ends), "specials": _first(specials)}
    sets["one outsider"], _ = with_one_outsider(_rng(6), sets["inside"], 1, SQRT_OUTSIDERS)
    return {name: sets[name] for name in SET_NAMES["sqrt_exact"]}


def _static_sets():
    """what the call sites of div1_known(.., true) claim: pixel centre over frame size, byte over 255, 1 over a window value"""
    r = _rng(7)
    n = WAVES * WAVE
    k, w = r.integers(0, 32768, n), r.integers(1, 32768, n)
    k[:8], w[:8] = [0, 0, 32767, 32767, 0, 1, 16383, 32766], [1, 32767, 1, 32767, 2, 3, 32767, 32767]
    px = np.zeros((n, 4), np.float32)
    px[:, 0], px[:, 1] = k.astype(np.float32) + np.float32(0.5), w.astype(np.float32)
    by = np.zeros((256, 4), np.float32)
    by[:, 0], by[:, 1] = np.arange(256, dtype=np.float32), 255.0
    z = np.zeros((n, 4), np.float32)
    z[:, 0], z[:, 1] = 1.0, inside_values(r, n)
    z[:4, 1] = [WIN_LO, WIN_HI, -WIN_LO, -WIN_HI]
    return {"pixel centres": px, "bytes over 255": by, "one over z": z}


K_MAX = 2048.0        # the clamp range of `shininess` in shade_fast_brdf: [1, 2048]; the other exponent of the kernels is the constant 6


def _pow_sets():
    r = _rng(8)
    n = 256 * WAVE
    dense = lambda m: np.maximum(r.integers(0, 1 << 24, m), 1).astype(np.float32) / np.float32(16777216.0)     # (0, 1] on the grid of 2^-24 ...  # noqa: E731
    wide = lambda m: np.minimum(np.exp2(-r.uniform(0.0, 24.0, m)), 1.0).astype(np.float32)                      # ... and log-spaced  # noqa: E731
    xk = lambda x, k: np.stack([x, np.asarray(k, np.float32), np.zeros(len(x), np.float32), np.zeros(len(x), np.float32)], 1).astype(np.float32)  # noqa: E731
    x6 = np.concatenate([dense(n), wide(n)])
    ks = np.exp2(r.uniform(0.0, 4.0, 2 * n)).astype(np.float32)
    ks[::4] = np.rint(ks[::4])
    kb = np.exp2(r.uniform(0.0, 11.0, 4 * n))
    kb[::4] = np.rint(kb[::4])
    kb = np.clip(kb.astype(np.float32), 1.0, K_MAX)
    xb = np.minimum(np.exp2(-r.uniform(0.0, 119.0, 4 * n) / kb.astype(np.float64)), 1.0).astype(np.float32)    # k log2 x in [-119, 0]
    kw = np.clip(np.exp2(r.uniform(0.0, 11.0, n)).astype(np.float32), 1.0, K_MAX)
    kw[:4] = [1.0, K_MAX, 6.0, 2047.0]
    xd = from_bits(r.integers(1, 1 << 23, n))
    xd[:2] = from_bits([1, 0x7FFFFF])
    kd = np.where(r.integers(0, 2, n) == 0, np.float32(6.0), np.clip(np.exp2(r.uniform(0.0, 11.0, n)).astype(np.float32), 1.0, K_MAX)).astype(np.float32)
    kd[:2] = 1.0
    k1 = np.resize(np.concatenate([np.float32([1.0, 6.0, K_MAX]), np.exp2(np.linspace(0.0, 11.0, 61)).astype(np.float32)]), 4 * WAVE)
    return {"k = 6": xk(x6, np.full(2 * n, 6.0)), "small k": xk(np.concatenate([dense(n), wide(n)]), ks), "bounded result": xk(xb, kb),
            "k to 2048": xk(dense(n), kw), "denormal x": xk(xd, kd), "x = 1": xk(np.ones(4 * WAVE, np.float32), k1)}


SAT_ANCHORS = [0x00000000, 0x80000000, 0x3F800000, 0x437F0000, 0x43800000, 0x4F000000, 0x4F800000, 0x4F7FFFFF, 0x7F800000, 0x7FC00000]
#              0           -0          1           255         256         2^31        2^32        below 2^32  inf         NaN


def _sat_sets():
    sweep = from_bits(np.arange(1 << 20, dtype=np.int64) * 4096 + 0x5A5)           # every 4096th of all 2^32 bit patterns
    a = (np.array(SAT_ANCHORS, np.int64)[:, None] + np.arange(-16, 17)[None, :]).reshape(-1)
    a = np.concatenate([a, a + 0x80000000])                                          # ... and the same magnitudes with the other sign
    return {"sweep": _first(sweep), "anchors": _first(from_bits(np.resize(a, len(a) + (-len(a) % WAVE))))}


def _wave_max_sets():
    r = _rng(9)
    w = 512
    b = r.integers(0, 0x7F800000, (w, WAVE))                                         # +0 .. the largest finite, every exponent
    b[np.arange(w), np.arange(w) % WAVE] = 0x7F000000 | (b[np.arange(w), np.arange(w) % WAVE] & 0x7FFFFF)   # a likely winner that walks through the lanes
    b[np.arange(0, w, 7), (np.arange(0, w, 7) * 5 + 3) % WAVE] = 0x7F800000          # +inf in some waves
    e = np.zeros((4 * WAVE, WAVE), np.int64)
    e[WAVE:2 * WAVE] = r.integers(1, 1 << 23, (WAVE, WAVE))                          # all denormal
    e[2 * WAVE:3 * WAVE][np.arange(WAVE), np.arange(WAVE)] = 1                       # the smallest denormal among zeros, in every lane
    e[3 * WAVE:] = 0x3F800000                                                        # ties, one larger value in every lane position
    e[3 * WAVE:][np.arange(WAVE), np.arange(WAVE)] = 0x3F800001
    return {"random": _first(from_bits(b.reshape(-1))), "edges": _first(from_bits(e.reshape(-1)))}


def _wave_add_sets():
    r = _rng(10)
    w = 512
    small = r.integers(0, 256, (w, WAVE))
    small[::3] = np.where(r.integers(0, 2, small[::3].shape) == 0, 0, small[::3])
    small[1] = 0
    words = r.integers(0, 1 << 32, (w, WAVE))
    words[0] = 0xFFFFFFFF
    words[1] = np.where(np.arange(WAVE) == 0, 0xFFFFFFFF, 1)
    words[2] = np.arange(WAVE) == 63
    return {"small counts": _first(from_bits(small.reshape(-1))), "words": _first(from_bits(words.reshape(-1)))}


@functools.lru_cache(maxsize=None)
def operand_sets(kind):
    """{set name: [n][4] float32 operands, n a multiple of 64}; built once, read-only"""
    if kind in DIVS:
        sets = _division_sets(kind)
    elif kind in NORMS:
        sets = _normalize_sets()
    else:
        sets = {"div1_static": _static_sets, "sqrt_exact": _sqrt_sets, "pow_exp2_log2": _pow_sets, "sat_u32": _sat_sets,
                "wave_max_nonneg": _wave_max_sets, "wave_inclusive_add": _wave_add_sets}[kind]()
    assert list(sets) == SET_NAMES[kind]
    out = {}
    for name, a in sets.items():
        a = np.ascontiguousarray(a, np.float32)
        assert a.ndim == 2 and a.shape[1] == 4 and len(a) % WAVE == 0, (kind, name, a.shape)
        a.setflags(write=False)
        out[name] = a
    return out


def outsider_lanes(kind):
    """([waves] lane, [waves] category index) of the one-outsider set, found by comparing it with the inside set"""
    s = operand_sets(kind)
    changed = (bits(s["one outsider"]) != bits(s["inside"])).any(axis=1).reshape(-1, WAVE)
    assert (changed.sum(axis=1) == 1).all()
    w = np.arange(len(changed))
    return changed.argmax(axis=1), (w + w // WAVE) % 8


# ---- the relaxed normalisation -----------------------------------------------------------------------------------------------------
RELAXED_SHORT_SETS = ["inside", "ends", "zero patterns", "unit normals"]


def relaxed_distance(ops, got):
    """[n][4]: |got - exact form| in ulp32 of the exact form's value (float32 reference(): components and magnitude)"""
    ref = reference("normalize3_relaxed", ops).astype(np.float64)
    with np.errstate(all="ignore"):
        return np.abs(np.asarray(got, np.float32).astype(np.float64) - ref) / ulp32(ref)


def relaxed_model(ops, shift):
    """x * inv, m2 * inv in float32 with inv the correctly rounded float32 1 / sqrt(m2) moved by `shift` ulp: what the short path
    returns if v_rsq_f32 is `shift` ulp off the correctly rounded value"""
    o = np.asarray(ops, np.float32)
    m2 = squared_magnitude(o)
    with np.errstate(all="ignore"):
        inv = shifted((1.0 / np.sqrt(m2.astype(np.float64))).astype(np.float32), shift)
        return np.stack([o[:, 0] * inv, o[:, 1] * inv, o[:, 2] * inv, m2 * inv], 1)


@functools.lru_cache(maxsize=None)
def relaxed_bound(shifts=(-1, 0, 1)):
    """(per component, magnitude): the largest distance of the model from the exact form over the tuples of the relaxed sets whose
    squared magnitude is inside its window, for a v_rsq_f32 within 1 ulp of correctly rounded (the ISA manual's figure).  Computed
    from the references alone."""
    comp = mag = 0.0
    for name in RELAXED_SHORT_SETS:
        ops = operand_sets("normalize3_relaxed")[name]
        ops = ops[sq_in_window(squared_magnitude(ops))]
        for s in shifts:
            d = relaxed_distance(ops, relaxed_model(ops, s))
            comp, mag = max(comp, float(d[:, :3].max())), max(mag, float(d[:, 3].max()))
    return comp, mag


# ---- pow through exp2(k log2 x) ----------------------------------------------------------------------------------------------------
POW_EXEMPT_BELOW = 2.0 ** -120


def pow_reference(ops):
    """(float64 2^y, y = k log2 x in float64, the bound in ulp32 of 2^y, exempt): the bound is 3 + 7 ln 2 |y| -- log2 and exp2 within
    3 ulp each (the OpenCL full-profile figures tests/libm_ref.py adopts), the product k * lg rounded once: y is off by at most
    (3 + 1/2) ulp32(y) twice over, 7 |y| 2^-24 in all, which 2^y turns into a relative error of 7 ln 2 |y| 2^-24, at most
    7 ln 2 |y| ulp32 of the result; exp2's own 3 ulp on top.  Results below 2^-120 are exempt (the device may scale, flush or keep them)."""
    o = np.asarray(ops, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        y = o[:, 1] * np.log2(o[:, 0])
        ref = np.exp2(y)
    return ref, y, 3.0 + 7.0 * np.log(2.0) * np.abs(y), ~(ref >= POW_EXEMPT_BELOW)


def pow_emulation(ops):
    """the sequence in numpy float32: log2f, one rounded product, exp2f"""
    o = np.asarray(ops, np.float32)
    with np.errstate(all="ignore"):
        return np.exp2((o[:, 1] * np.log2(o[:, 0])).astype(np.float32)).astype(np.float32)


def pow_judge(ops, got):
    """(error in ulp32 of the reference [n], bound [n], exempt [n]); a NaN or infinite result has an infinite error"""
    ref, _, bound, exempt = pow_reference(ops)
    got = np.asarray(got, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        err = np.abs(got - ref) / ulp32(ref)
    return np.where(np.isfinite(err), err, np.inf), bound, exempt
