"""The twelve Rusteria opcodes backed by a maths library (slow_unary / slow_binary of rusterix_amd/csrc/rxr_vm.h; oracle/rusteria_vm.hpp
on glibc) measured in ulps: the float64 reference, the ulp measure, the operand sets and the program builders that
tests/test_libm_cpu.py (the oracle, no GPU) and tests/test_gpu_libm_ulp.py (the device) share.

How an operand reaches an opcode: a pattern is a float array that crosses the host mirror untouched, `Sample` is a nearest fetch, and
rxr_bake_shaders hands back the interpreter's float results bit for bit.  A 64 x 64 bake (the bake's own size) of
`UV, Push 0, Sample, OP, SetColor` therefore applies OP to every texel of a 64 x 64 x 3 pattern: 12 288 f32 bit patterns of the
test's choosing per call, their f32 results read back.

Reference: numpy float64 of the f32 operands (np.sin, np.tan, np.arctan, np.log, np.arctan2, np.power), with the reference
implementation's quirks restated from slow_unary: Cos1 / Cos2 compute the SINE (execution.rs:337-344), the 1- and 2-component
forms zero the other components, Rotate2D forms its angle in f32.

Error: |got - ref64| / ulp32(ref64), the f32 spacing at |ref64| floored at 2^-149.  Class rule: NaN, +inf, -inf and zero must
be met exactly, and so must the sign of every non-zero result (the sign of a zero is not visible through the bake's `+ 0.0`).
Exempt from both are only results within the opcode's bound of the f32 overflow threshold and non-zero results below 2^-126
(where the device may return the denormal or zero: counted, not judged).

Bounds: the single-precision bounds of the OpenCL full profile, the standard tests/bake_ref.py adopted for powf."""
import functools

import numpy as np

from tests import bake_ref as R
from tests.bake_ref import P

W = H = 64                                    # R.SIZES[0], the bake's own size; a power of two: uv = x / W is exact
UNARY = ["Sin", "Sin1", "Sin2", "Cos", "Cos1", "Cos2", "Tan", "Atan", "Log"]
BINARY = ["Atan2", "Pow", "Rotate2D"]
OPS = UNARY + BINARY
# ulps, OpenCL full profile, single precision: sin / cos 4, tan 5, atan 5, atan2 6, log 3, pow 16
BOUND = {"Sin": 4.0, "Sin1": 4.0, "Sin2": 4.0, "Cos": 4.0, "Cos1": 4.0, "Cos2": 4.0, "Tan": 5.0, "Atan": 5.0, "Log": 3.0, "Atan2": 6.0, "Pow": 16.0}
COMPONENTS = {"Sin1": 1, "Cos1": 1, "Sin2": 2, "Cos2": 2}      # how many components the opcode computes (default 3); the others are zeroed
U = 2.0 ** -24                                # relative error of one f32 rounding
FLT_MAX = float(np.finfo(np.float32).max)
OVERFLOW = (2.0 - 2.0 ** -24) * 2.0 ** 127    # the smallest magnitude that rounds to infinity
MIN_NORMAL = 2.0 ** -126
DEG = np.float32(3.14159265358979323846 / 180.0)   # `3.14159265358979323846f / 180.0f` of slow_binary
WINDOW = (2.0 ** -8, 256.0)                   # results whose last bit lies inside the four Fract(r * 2^k) windows of the frame tests


def f32(x):
    return np.asarray(x, np.float64).astype(np.float32)


def from_bits(b):
    return np.asarray(b, np.uint32).view(np.float32)


def neighbours(x, n):
    """the f32 values within n ulp of every (finite, non-zero, same-binade-safe) x: [len(x) * (2n + 1)]"""
    b = np.asarray(x, np.float32).view(np.int32).astype(np.int64)[:, None] + np.arange(-n, n + 1)[None, :]
    return b.reshape(-1).astype(np.uint32).view(np.float32)


def log_spaced(rng, lo_exp, hi_exp, n):
    """n positive f32 values, exponents uniform in [lo_exp, hi_exp), random mantissas"""
    return f32(np.exp2(rng.uniform(lo_exp, hi_exp, n)))


# what fills the rest of every set, over and over: +-0, +-inf, NaN, +-1, +-FLT_MAX, the smallest normals ...
SPECIALS = from_bits([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0x3F800000, 0xBF800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x00800000, 0x80800000])
# ... and, once per set (their results are denormal for most opcodes: the exemption band must stay small), the ends of the denormal range
DENORMAL_ENDS = from_bits([0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF])


# ---- operand sets ------------------------------------------------------------------------------------------------------------------
class Set:
    """12 288 operands (pairs for a binary opcode) as 64 x 64 x 3 patterns, and the part of the set each one belongs to"""

    def __init__(self, parts, second=None):
        names, chunks, chunks_b = [], [], []
        for name, a in parts:
            a = np.asarray(a, np.float32).reshape(-1) if second is None else np.asarray(a, np.float32).reshape(-1, 2)
            names += [name] * len(a)
            chunks.append(a)
        ends = DENORMAL_ENDS if second is None else np.stack(np.meshgrid(np.concatenate([DENORMAL_ENDS, SPECIALS]), DENORMAL_ENDS, indexing="ij"), -1).reshape(-1, 2)
        ends = ends if second is None else np.concatenate([ends, ends[:, ::-1]])
        names += ["denormal ends"] * len(ends)
        a = np.concatenate(chunks + [ends])
        n = W * H * 3
        assert len(a) <= n, len(a)
        fill = SPECIALS if second is None else np.stack(np.meshgrid(SPECIALS, SPECIALS, indexing="ij"), -1).reshape(-1, 2)
        k = n - len(a)
        a = np.concatenate([a, np.resize(fill, (k,) + fill.shape[1:])])
        names += ["specials"] * k
        self.part = np.array(names).reshape(H, W, 3)
        if second is None:
            self.a, self.b = a.reshape(H, W, 3).copy(), None
        else:
            self.a, self.b = a[:, 0].reshape(H, W, 3).copy(), a[:, 1].reshape(H, W, 3).copy()

    def patterns(self):
        return [self.a] if self.b is None else [self.a, self.b]


def trig_set():
    rng = np.random.default_rng([0x4C49424D, 1])
    k = np.unique(np.rint(np.exp2(np.linspace(0.0, 22.0, 150)))).astype(np.float64)
    k = np.concatenate([k, -k[::3]])
    big = log_spaced(rng, np.log2(1e5), np.log2(3.4e38), 3000) * np.where(rng.random(3000) < 0.5, -1, 1).astype(np.float32)
    mags = f32(np.exp2(np.linspace(-149.0, 127.0, 300)))
    return Set([("dense [-2pi, 2pi]", f32(rng.uniform(-2 * np.pi, 2 * np.pi, 4600))),
                ("k pi/2 +- 8 ulp", neighbours(f32(k * (np.pi / 2)), 8)),
                ("magnitudes 2^-149 .. 2^127", np.concatenate([mags, -mags])),
                ("large arguments [1e5, 3.4e38]", big)])


def atan_set():
    rng = np.random.default_rng([0x4C49424D, 2])
    e = np.repeat(np.arange(1, 255, dtype=np.uint32), 6)
    binades = from_bits((e << 23) | rng.integers(0, 1 << 23, len(e)).astype(np.uint32))
    den = from_bits(np.unique(np.rint(np.exp2(np.linspace(0.0, 22.99, 40))).astype(np.uint32)))
    return Set([("every binade", np.concatenate([binades, -binades])),
                ("+-1 +- 64 ulp", neighbours(np.float32([1.0, -1.0]), 64)),
                ("denormals", np.concatenate([den, -den])),
                ("dense [-8, 8]", f32(rng.uniform(-8.0, 8.0, 7000)))])


def log_set():
    rng = np.random.default_rng([0x4C49424D, 3])
    return Set([("(0, FLT_MAX] log-spaced", np.concatenate([log_spaced(rng, -126.0, 128.0, 5000), np.float32([FLT_MAX])])),
                ("1 +- 64 ulp", neighbours(np.float32([1.0]), 64)),
                ("powers of two", f32(np.exp2(np.arange(-149.0, 128.0)))),
                ("denormals", from_bits(rng.integers(1, 1 << 23, 600).astype(np.uint32))),
                ("dense [0.25, 4]", f32(rng.uniform(0.25, 4.0, 3500))),
                ("negatives", -log_spaced(rng, -149.0, 128.0, 400))])


def atan2_set():
    rng = np.random.default_rng([0x4C49424D, 4])
    n = 7000
    ratio, mid = rng.uniform(-120.0, 120.0, n), rng.uniform(-3.0, 3.0, n)
    sign = lambda m: np.where(rng.random(m) < 0.5, -1.0, 1.0)   # noqa: E731
    y = f32(np.exp2(mid + ratio / 2) * rng.uniform(1.0, 2.0, n) * sign(n))
    x = f32(np.exp2(mid - ratio / 2) * rng.uniform(1.0, 2.0, n) * sign(n))
    dense = f32(rng.uniform(-4.0, 4.0, (3500, 2)))
    r = f32(np.exp2(rng.uniform(-100.0, 100.0, 400)) * sign(400))
    z = np.where(rng.random(400) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    axes = np.concatenate([np.stack([z[:200], r[:200]], 1), np.stack([r[200:], z[200:]], 1)])
    return Set([("quadrants, ratios to 2^+-120", np.stack([y, x], 1)), ("dense [-4, 4]^2", dense), ("axes", axes)], second=True)


def pow_set():
    rng = np.random.default_rng([0x4C49424D, 5])
    general = np.stack([f32(rng.uniform(0.0, 4.0, 4000)) + np.float32(2.0 ** -20), f32(rng.uniform(-8.0, 8.0, 4000))], 1)
    n = 2500
    near = f32(1.0 + np.exp2(rng.uniform(-23.0, -10.0, n)) * np.where(rng.random(n) < 0.5, -0.5, 1.0))   # (below 1 the spacing halves)
    ynear = f32(np.exp2(rng.uniform(0.0, 20.0, n)) * np.where(rng.random(n) < 0.5, -1.0, 1.0))
    nb = -f32(rng.uniform(0.01, 4.0, 1200))
    ny = np.concatenate([np.rint(rng.uniform(-8.0, 8.0, 600)), rng.uniform(-8.0, 8.0, 600)])
    base = f32(rng.uniform(1.5, 4.0, 250))
    target = np.concatenate([rng.uniform(120.0, 136.0, 200), rng.uniform(-156.0, -118.0, 50)])    # log2 of the result
    gamma = np.stack([f32(rng.uniform(0.0, 1.0, 3000)), np.full(3000, np.float32(0.4545))], 1)
    named = np.float32([[0.0, 0.0], [-0.0, 0.0], [0.0, -3.0], [-0.0, -3.0], [0.0, -2.0], [-0.0, -2.0], [-0.0, 3.0], [0.0, 2.5], [-0.0, -2.5],
                        [0.5, np.inf], [0.5, -np.inf], [2.0, np.inf], [2.0, -np.inf], [-0.5, np.inf], [-2.0, -np.inf], [1.0, np.inf], [-1.0, np.inf],
                        [1.0, np.nan], [np.nan, 0.0], [-1.0, 0.5], [-8.0, 1.0 / 3.0], [np.inf, -1.0], [-np.inf, 3.0], [-np.inf, 2.0], [-np.inf, -3.0]])
    return Set([("bases (0, 4], exponents [-8, 8]", general), ("bases within 2^-10 of 1, |y| to 2^20", np.stack([near, ynear], 1)),
                ("negative bases", np.stack([nb, f32(ny)], 1)), ("near overflow and underflow", np.stack([base, f32(target / np.log2(base.astype(np.float64)))], 1)),
                ("gamma 0.4545", gamma), ("named cases", np.tile(named, (8, 1)))], second=True)


def rotate_set():
    """a = the vector (all three components), b.x = the angle in degrees: 4096 cases"""
    rng = np.random.default_rng([0x4C49424D, 6])
    n = W * H
    ang = np.concatenate([f32(rng.uniform(-720.0, 720.0, 2400)), f32(90.0 * np.rint(rng.uniform(-12.0, 12.0, 500))), f32(90.0 * np.rint(rng.uniform(-11000.0, 11000.0, 296))),
                          f32(np.exp2(rng.uniform(np.log2(720.0), np.log2(1e6), 900)) * np.where(rng.random(900) < 0.5, -1.0, 1.0))])
    names = ["angles [-720, 720]"] * 2400 + ["multiples of 90"] * 796 + ["angles to 1e6"] * 900
    assert len(ang) == n
    s = Set.__new__(Set)
    s.a = f32(rng.uniform(-4.0, 4.0, (H, W, 3)))
    s.b = np.repeat(ang.reshape(H, W, 1), 3, axis=2).copy()
    s.part = np.repeat(np.array(names).reshape(H, W, 1), 3, axis=2)
    return s


@functools.lru_cache(maxsize=None)
def operand_set(op):
    if op in ("Sin", "Sin1", "Sin2", "Cos", "Cos1", "Cos2", "Tan"):
        return trig_set()
    return {"Atan": atan_set, "Log": log_set, "Atan2": atan2_set, "Pow": pow_set, "Rotate2D": rotate_set}[op]()


def used(op):
    """[H][W][3] bool: the components the opcode computes from an operand (the others are zeroed, or passed through by Rotate2D)"""
    m = np.zeros((H, W, 3), bool)
    m[..., :2 if op == "Rotate2D" else COMPONENTS.get(op, 3)] = True
    return m


# ---- the reference -----------------------------------------------------------------------------------------------------------------
def reference(op, a, b=None):
    """float64 result of `op` on f32 operands, [.., 3]"""
    a64 = np.asarray(a, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        if op in COMPONENTS or op in ("Sin", "Cos"):
            r = np.cos(a64) if op == "Cos" else np.sin(a64)       # Cos1 / Cos2: the sine
            r[..., COMPONENTS.get(op, 3):] = 0.0
            return r
        if op == "Tan":
            return np.tan(a64)
        if op == "Atan":
            return np.arctan(a64)
        if op == "Log":
            return np.log(a64)
        b64 = np.asarray(b, np.float32).astype(np.float64)
        if op == "Atan2":
            return np.arctan2(a64, b64)
        if op == "Pow":
            return np.power(a64, b64)
        return rotate_reference(a, b)[0]


def rotate_reference(a, b):
    """Rotate2D: (float64 result, absolute bound).  rad = b.x * f32(pi / 180) in f32; (a.x c - a.y s, a.x s + a.y c, a.z).
    Bound: s and c are each within 4 ulp (the sin / cos bound) of a value of magnitude at most 1 -- e_s = 4 ulp32(s), e_c = 4 ulp32(c);
    each product is one rounding of |a| (|c| + e_c), the sum one rounding of the two rounded products.  With
    T = |a.x| (|c| + e_c) + |a.y| (|s| + e_s):  |error| <= |a.x| e_c + |a.y| e_s + U T + U T (1 + U), U = 2^-24.  a.z is exact."""
    a = np.asarray(a, np.float32)
    rad = (np.asarray(b, np.float32)[..., 0] * DEG).astype(np.float64)
    ax, ay = a[..., 0].astype(np.float64), a[..., 1].astype(np.float64)
    with np.errstate(all="ignore"):
        s, c = np.sin(rad), np.cos(rad)
        es, ec = BOUND["Sin"] * ulp32(s), BOUND["Cos"] * ulp32(c)
        ref = np.stack([ax * c - ay * s, ax * s + ay * c, a[..., 2].astype(np.float64)], -1)
        tx = np.abs(ax) * (np.abs(c) + ec) + np.abs(ay) * (np.abs(s) + es)
        ty = np.abs(ax) * (np.abs(s) + es) + np.abs(ay) * (np.abs(c) + ec)
        bx = np.abs(ax) * ec + np.abs(ay) * es + U * tx + U * tx * (1 + U)
        by = np.abs(ax) * es + np.abs(ay) * ec + U * ty + U * ty * (1 + U)
    return ref, np.stack([bx, by, np.zeros_like(bx)], -1)


def ulp32(ref):
    """the spacing of f32 at |ref| (float64), floored at 2^-149; the spacing at FLT_MAX beyond it"""
    with np.errstate(all="ignore"):
        _, ex = np.frexp(np.where(np.isfinite(ref) & (ref != 0), np.abs(ref), MIN_NORMAL))        # |ref| = m 2^ex, m in [0.5, 1)
    return np.exp2(np.clip(ex - 1, -126, 127).astype(np.float64) - 23.0)


def classes(x):
    """0 NaN, 1 +inf, 2 -inf, 3 zero, 4 positive, 5 negative.  A float64 reference is classed as its f32 rounding is: at or beyond
    the overflow threshold it is an infinity."""
    x = np.asarray(x)
    big = np.abs(x) >= OVERFLOW if x.dtype == np.float64 else np.isinf(x)
    return np.where(np.isnan(x), 0, np.where(big & (x > 0), 1, np.where(big, 2, np.where(x == 0, 3, np.where(x > 0, 4, 5)))))


CLASS_NAMES = ["NaN", "+inf", "-inf", "zero", "positive", "negative"]


def exempt_band(ref, bound):
    """(near the overflow threshold, non-zero below 2^-126)"""
    with np.errstate(all="ignore"):
        over = np.abs(np.abs(ref) - OVERFLOW) <= bound * 2.0 ** 104
        under = (ref != 0) & (np.abs(ref) < MIN_NORMAL)
    return over, under


class Verdict:
    def __init__(self, op):
        self.op, self.failures = op, []
        self.max_ulp, self.worst, self.n_band, self.denormal_kept, self.denormal_flushed, self.n_judged = 0.0, None, 0, 0, 0, 0

    def denormals(self):
        if self.denormal_kept + self.denormal_flushed == 0:
            return "no result below 2^-126"
        return f"{self.denormal_kept} denormal, {self.denormal_flushed} zero"

    def line(self):
        unit = "of its derived bound" if self.op == "Rotate2D" else "ulp"
        return f"{self.op}: max {self.max_ulp:.3f} {unit} at {self.worst}; {self.n_band} of {self.n_judged} exempt; below 2^-126: {self.denormals()}"

    def failed_parts(self):
        return sorted({f[0] for f in self.failures})

    def message(self):
        by = {}
        for part, text in self.failures:
            by.setdefault(part, []).append(text)
        return f"{self.op}: " + "; ".join(f"[{p}] {len(t)} operands, e.g. {t[0]}" for p, t in sorted(by.items()))


def fmt(v):
    v = np.float32(v)
    return f"{float(v)!r} (0x{int(v.view(np.uint32)):08X})"


def judge(op, got, s=None):
    """`got`: [H][W][3] f32 results per OPERAND texel (see by_operand).  Returns a Verdict; nothing is asserted here."""
    s = s or operand_set(op)
    got = np.asarray(got, np.float32)
    v = Verdict(op)
    m = used(op)
    if op == "Rotate2D":
        ref, bound_abs = rotate_reference(s.a, s.b)
        finite = np.isfinite(ref)
        err = np.abs(got.astype(np.float64) - ref)
        with np.errstate(all="ignore"):
            bad = np.where(finite, ~(err <= bound_abs + 2.0 ** -149), classes(got) != classes(ref))
            ratio = np.where(finite & m & (bound_abs > 0), err / np.where(bound_abs > 0, bound_abs, 1.0), 0.0)
        v.n_judged = int(m.sum())
        v.max_ulp = float(ratio.max())            # (as a fraction of the derived bound)
        at = np.unravel_index(int(ratio.argmax()), ratio.shape)
        v.worst = f"v = ({fmt(s.a[at[0], at[1], 0])}, {fmt(s.a[at[0], at[1], 1])}), angle {fmt(s.b[at[0], at[1], 0])}"
        for y, x, c in np.argwhere(bad):
            v.failures.append((str(s.part[y, x, c]), f"v = ({fmt(s.a[y, x, 0])}, {fmt(s.a[y, x, 1])}, {fmt(s.a[y, x, 2])}), angle {fmt(s.b[y, x, 0])}: component {c} is {fmt(got[y, x, c])}, "
                               f"reference {ref[y, x, c]!r} +- {bound_abs[y, x, c]:.3g}"))
        return v
    bound = BOUND[op]
    ref = reference(op, s.a, s.b)
    over, under = exempt_band(ref, bound)
    band = (over | under) & m
    cr, cg = classes(ref), classes(got)
    with np.errstate(all="ignore"):
        err = np.where(cr >= 4, np.abs(got.astype(np.float64) - ref) / ulp32(ref), 0.0)
        err = np.where(np.isfinite(err), err, np.inf)
    judged = ~band
    bad = judged & ((cr != cg) | (err > bound))
    v.n_judged, v.n_band = int(m.sum()), int(band.sum())
    v.denormal_kept = int((under & m & (got != 0)).sum())
    v.denormal_flushed = int((under & m & (got == 0)).sum())
    e = np.where(judged & m & (cr == cg), err, 0.0)
    v.max_ulp = float(e.max())
    at = np.unravel_index(int(e.argmax()), e.shape)
    v.worst = fmt(s.a[at]) if s.b is None else f"({fmt(s.a[at])}, {fmt(s.b[at])})"
    for y, x, c in np.argwhere(bad):
        operand = fmt(s.a[y, x, c]) if s.b is None else f"({fmt(s.a[y, x, c])}, {fmt(s.b[y, x, c])})"
        what = f"class {CLASS_NAMES[cg[y, x, c]]}, reference {CLASS_NAMES[cr[y, x, c]]}" if cr[y, x, c] != cg[y, x, c] else f"{err[y, x, c]:.2f} ulp (bound {bound:g})"
        v.failures.append((str(s.part[y, x, c]), f"{operand} -> {fmt(got[y, x, c])}, reference {ref[y, x, c]!r}: {what}"))
    return v


def judged_mask(op):
    """[H][W][3] bool: the operands outside the exemption band (every operand for Rotate2D)"""
    s = operand_set(op)
    if op == "Rotate2D":
        return np.ones((H, W, 3), bool)
    over, under = exempt_band(reference(op, s.a, s.b), BOUND[op])
    return ~(over | under)


def in_window(results):
    """results whose last bit lies inside the four Fract(r * 2^k) windows, k = 0, 8, 16, 24"""
    with np.errstate(all="ignore"):
        return (np.abs(results) >= WINDOW[0]) & (np.abs(results) < WINDOW[1])


# ---- programs and the texel-to-operand map -----------------------------------------------------------------------------------------
OPERAND = ["UV", ("Push", 0.0), "Sample"]
SECOND = ["UV", ("Push", 1.0), "Sample"]
PASS_THROUGH = P(OPERAND + ["SetColor"])


def program(op, wrapped=False):
    """`operand(s), OP, SetColor`; wrapped: the opcode inside a function (a set with a call has no static stack depths: k_bake)"""
    n = 1 if op in UNARY else 2
    args = OPERAND + (SECOND if n == 2 else [])
    if wrapped:
        return P(args + [("FunctionCall", n, n, 1), "SetColor"], [("LoadLocal", i) for i in range(n)] + [op])
    return P(args + [op, "SetColor"])


def by_operand(pixels):
    """bake texel (x, y) has uv = (x / W, 1 - y / H) and pattern_sample fetches pattern texel (x, (H - y) mod H) -- exact for powers of
    two.  [H][W][>=3] bake pixels -> [H][W][3] in the pattern's own order (the map is its own inverse)."""
    return np.asarray(pixels)[(H - np.arange(H)) % H][..., :3]


class Oracle:
    """the opcodes on the CPU oracle (glibc), through tests/bake_ref.Reference: one orc_vm_shade per texel"""

    def __init__(self, oracle):
        self.oracle = oracle
        self._results = {}

    def bake(self, prog, patterns):
        ref = R.Reference(self.oracle, [prog])
        ref.assets = self.oracle.Assets.default().patterns(patterns)
        return ref.pixels(0, W, H)

    def results(self, op):
        """[H][W][3] f32 per operand texel; computed once, not to be written to"""
        if op not in self._results:
            r = by_operand(self.bake(program(op), operand_set(op).patterns())).copy()
            r.setflags(write=False)
            self._results[op] = r
        return self._results[op]


_ORACLES = {}


def oracle_results(oracle):
    return _ORACLES.setdefault(id(oracle), Oracle(oracle))
