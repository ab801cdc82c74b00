#!/usr/bin/env python3
"""SHA-256 of every function of a gfx950 assembly listing (hipcc --cuda-device-only -S): for a refactor that must not move an
instruction.  Per kernel the instruction text from its label to its last s_endpgm and, separately, its .amdhsa_kernel descriptor
block; per out-of-line device function its whole body.  Normalised: comments, blank lines and surrounding white space dropped.

    tools/kernel_text_sha.py rxr_kernels.s               # name, sha of the text, sha of the descriptor
    tools/kernel_text_sha.py before.s after.s            # the same side by side; exit status 1 when a column differs
    tools/kernel_text_sha.py --rename NEW=OLD before.s after.s   # a symbol whose mangled name had to change: NEW reads as OLD everywhere
    tools/kernel_text_sha.py --local-labels before.s after.s     # functions were added ahead of others: a block label .LBB<f>_<b> carries
                                                                 # its function's position <f> in the file, which then moves; read as .LBB_<b>
"""
import hashlib
import re
import sys


def functions(path, renames=(), local_labels=False):
    text = open(path).read()
    for new, old in renames:
        text = text.replace(new, old)
    if local_labels:
        text = re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", text)
    lines = text.split("\n")
    out, desc = {}, {}
    i = 0
    while i < len(lines):
        m = re.match(r"\s*\.type\s+([\w.$]+),@function", lines[i])
        if m:
            name = m.group(1)
            while lines[i].split(";")[0].strip() != name + ":":
                i += 1
            body = []
            i += 1
            while not re.match(r"\.Lfunc_end\d+:", lines[i].strip()):
                t = lines[i].split(";")[0].strip()
                if t.startswith(".amdhsa_kernel "):  # (the descriptor sits between a kernel's padding and its end label)
                    desc[name] = []
                if name in desc and desc[name][-1:] != [".end_amdhsa_kernel"]:
                    desc[name].append(t)
                elif t:
                    body.append(t)
                i += 1
            out[name] = body
        i += 1
    for name in desc:  # a kernel's text ends at its last s_endpgm (padding follows)
        body = out[name]
        out[name] = body[:max(k for k, t in enumerate(body) if t == "s_endpgm") + 1]
    return out, desc


def sha(lines):
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()[:16] if lines is not None else "-" * 16


def main(args):
    renames, paths, local_labels = [], [], False
    while args:
        a = args.pop(0)
        if a == "--rename":
            renames.append(tuple(args.pop(0).split("=", 1)))
        elif a == "--local-labels":
            local_labels = True
        else:
            paths.append(a)
    tables = [functions(p, renames, local_labels) for p in paths]
    names = sorted(set().union(*(t[0] for t in tables)), key=lambda n: (n not in tables[0][1], n))
    differ = 0
    for n in names:
        cols = [sha(t[0].get(n)) + " " + (sha(t[1][n]) if n in t[1] else "function".ljust(16)) for t in tables]
        same = len(set(cols)) == 1
        differ += not same
        print(n, *cols, "" if same or len(cols) == 1 else "DIFFERS")
    return 1 if differ and len(paths) > 1 else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
