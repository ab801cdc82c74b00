#!/usr/bin/env python3
"""The relaxed light loop of a raster kernel in a gfx950 assembly listing (hipcc --cuda-device-only -S of rxr_kernels.hip): what a
light costs a wave around its arithmetic.  Used by tests/test_light_prefix_isa.py and for the table of profiles/light_prefix/README.md.

    tools/light_loop_isa.py rxr_kernels.s [kernel ...]     # default: k_raster_rl k_raster_rows_rl

Per kernel two blocks are looked for and counted.  Both are loops (a label and the last branch back to it) whose body holds exactly
two v_rsq_f32 and neither v_sqrt_f32 nor v_div_scale_f32, the innermost of their kind:
  prefix loop   the loop of the leading fast lights (shade3d_lights<LV, true>): the first of the two
  fast block    the fast term's cycle through the general loop, which has the same signature (the general path leaves it for code
                placed elsewhere): the second such loop of a kernel, and the only one in a listing from before the prefix loop
"""
import re
import sys

VALU = re.compile(r"^v_(?!readlane|readfirstlane|writelane)")  # lane moves are counted separately
BRANCH = re.compile(r"^s_c?branch\w*\s+(\.LBB\d+_\d+)")
LABEL = re.compile(r"^(\.LBB\d+_\d+):")


def kernel_lines(isa, name):
    """instruction and label lines of a kernel, comments dropped"""
    m = re.search(rf"^{re.escape(name)}:[^\n]*\n(.*?)^\.Lfunc_end\d+:", isa, flags=re.S | re.M)
    assert m, name
    out = []
    for line in m.group(1).split("\n"):
        t = line.split(";")[0].strip()
        if t and not t.startswith((".p2align", ".amdhsa", ".section", ".end_amdhsa")):
            out.append(t)
    return out


def loops(lines):
    """(first, last) line indices of every loop: a label and the last branch back to it (an early `continue` or a `break` that is
    routed through the header's test is a branch to the same label: one loop, not two)"""
    at = {LABEL.match(t).group(1): i for i, t in enumerate(lines) if LABEL.match(t)}
    last = {}
    for j, t in enumerate(lines):
        m = BRANCH.match(t)
        if m and m.group(1) in at and at[m.group(1)] <= j:
            last[at[m.group(1)]] = j
    return sorted(last.items())


def count(body):
    ops = [t.split()[0] for t in body if not LABEL.match(t)]
    kernarg_loads = [t for t in body if t.startswith("s_load_") and re.search(r",\s*s\[0:1\]", t)]
    return {
        "instructions": len(ops),
        "valu": sum(1 for o in ops if VALU.match(o)),
        "salu": sum(1 for o in ops if o.startswith("s_") and not o.startswith(("s_load_", "s_buffer_load_", "s_waitcnt", "s_nop", "s_cbranch", "s_branch"))),
        "v_mov_from_vgpr": sum(1 for t in body if re.match(r"v_mov_b32(_e32|_e64)?\s+v\d+,\s*v\d+\s*$", t)),
        "lane_moves": sum(1 for o in ops if o.startswith(("v_writelane_b32", "v_readlane_b32"))),
        "saveexec": sum(1 for o in ops if "saveexec" in o),
        "scalar_loads": sum(1 for o in ops if o.startswith(("s_load_", "s_buffer_load_"))),
        "scalar_loads_from_kernarg": len(kernarg_loads),
        "waits_lgkm": sum(1 for t in body if t.startswith("s_waitcnt") and "lgkmcnt" in t),
        "v_rsq_f32": sum(1 for o in ops if o.startswith("v_rsq_f32")),
    }


def fast_loops(isa, kernel):
    """bodies of the loops with exactly two v_rsq_f32 and neither v_sqrt_f32 nor v_div_scale_f32 that hold no other such loop, in the
    order of the listing.  (A loop inside one of them that holds no v_rsq_f32 is part of its control flow: the compiler routes a
    `break` through the header's test, which is a branch back to a label of its own.)"""
    lines = kernel_lines(isa, kernel)

    def is_fast(a, b):
        ops = [t.split()[0] for t in lines[a:b + 1]]
        return sum(o.startswith("v_rsq_f32") for o in ops) == 2 and not any(o.startswith(("v_sqrt_f32", "v_div_scale_f32")) for o in ops)

    fast = [(a, b) for a, b in loops(lines) if is_fast(a, b)]
    return [lines[a:b + 1] for a, b in fast if not any((c, d) != (a, b) and a <= c and d <= b for c, d in fast)]


def prefix_loop(isa, kernel):
    """the body of the prefix loop (it stands in front of the general loop), or None in a listing that has none"""
    found = fast_loops(isa, kernel)
    assert 1 <= len(found) <= 2, "%s: %d candidate loops" % (kernel, len(found))
    return found[0] if len(found) == 2 else None


def fast_block(isa, kernel):
    """the fast term's cycle through the general loop: its latch (with the copies where the two paths join), the narrowing of exec, the
    two scalar loads, the arithmetic and the branch back to the latch"""
    found = fast_loops(isa, kernel)
    assert 1 <= len(found) <= 2, "%s: %d candidate loops" % (kernel, len(found))
    return found[-1]


def main(args):
    isa = open(args[0]).read()
    for kernel in args[1:] or ["k_raster_rl", "k_raster_rows_rl"]:
        for what, body in (("prefix loop", prefix_loop(isa, kernel)), ("fast block", fast_block(isa, kernel))):
            print(kernel, what, count(body) if body else None)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
