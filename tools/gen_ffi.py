#!/usr/bin/env python3
"""Generates, from include/rxr.h (the single source of truth of the C ABI):

  shim/rusterix-hip-shim/src/ffi.rs   the Rust mirror: constants, #[repr(C)] structs, the extern "C" block and
                                      compile-time asserts of every size and field offset (core::mem::offset_of!)
  tests/abi_layout_asserts.h          the same sizes / offsets as C11 _Static_asserts, compiled by tests/abi_host.c
                                      (a CPU test): the C compiler thereby confirms the layout model used for the Rust side
  rusterix_amd/abi.py                 the Python mirror: constants, one ctypes.Structure per struct, the signature of every
                                      prototype of rxr.h and -- the test entry points, which the other two leave out -- of
                                      rusterix_amd/csrc/rxr_debug.h, and declare(lib), which types a loaded library with them

    python tools/gen_ffi.py            rewrite the three files
    python tools/gen_ffi.py --check    exit 1 if one of them is not what the headers imply (tests/test_abi_c.py,
                                       tests/test_abi_python_cpu.py)

The parser handles exactly the C subset the header uses: `#define NAME <integer expr>`, anonymous and named enums,
`typedef struct NAME {...} NAME;` with scalar / pointer / fixed-array / nested-struct fields, and plain prototypes.
Layout model: LP64 natural alignment (what C on x86-64 / aarch64 Linux and Rust's repr(C) both implement).
"""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rxr.h")
DEBUG_HEADER = os.path.join(ROOT, "rusterix_amd", "csrc", "rxr_debug.h")
ABI_PY = os.path.join(ROOT, "rusterix_amd", "abi.py")
FFI_RS = os.path.join(ROOT, "shim", "rusterix-hip-shim", "src", "ffi.rs")
ASSERTS_H = os.path.join(ROOT, "tests", "abi_layout_asserts.h")

SCALARS = {  # C type -> (Rust type, size, alignment)
    "uint8_t": ("u8", 1, 1), "uint32_t": ("u32", 4, 4), "int32_t": ("i32", 4, 4), "uint64_t": ("u64", 8, 8), "float": ("f32", 4, 4),
    "int": ("c_int", 4, 4), "size_t": ("usize", 8, 8), "char": ("c_char", 1, 1), "void": ("c_void", 0, 1),
}
PY_SCALARS = {  # C type -> ctypes name (`unsigned long long`: rxr_debug.h only)
    "uint8_t": "c_uint8", "uint32_t": "c_uint32", "int32_t": "c_int32", "uint64_t": "c_uint64", "float": "c_float", "int": "c_int",
    "size_t": "c_size_t", "unsigned long long": "c_ulonglong", "void": "None",
}


def strip_comments(text):
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def parse(text):
    text = strip_comments(text)
    defines, enums, structs, funcs = [], [], [], []
    for m in re.finditer(r"^#define\s+(RXR_\w+)\s+(.+)$", text, flags=re.M):
        name, val = m.group(1), m.group(2).strip()
        if name == "RXR_H":
            continue
        defines.append((name, val))
    for m in re.finditer(r"(typedef\s+)?enum\s*(\w*)\s*\{(.*?)\}\s*(\w*)\s*;", text, flags=re.S):
        tname = m.group(4) or m.group(2)
        items, nxt = [], 0
        for part in m.group(3).split(","):
            part = part.strip()
            if not part:
                continue
            if "=" in part:
                k, v = [x.strip() for x in part.split("=")]
                nxt = int(v, 0)
            else:
                k = part
            items.append((k, nxt))
            nxt += 1
        enums.append((tname, items))
    for m in re.finditer(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*(\w+)\s*;", text, flags=re.S):
        fields = []
        for decl in m.group(2).split(";"):
            decl = " ".join(decl.split())
            if not decl:
                continue
            fm = re.match(r"^(const\s+)?(\w+)\s*(\*?)\s*(.+)$", decl)
            const, ctype, star, rest = fm.group(1), fm.group(2), fm.group(3), fm.group(4)
            for item in rest.split(","):
                item = item.strip()
                ptr = bool(star)
                if item.startswith("*"):
                    ptr, item = True, item[1:].strip()
                am = re.match(r"^(\w+)\s*\[\s*(\w+)\s*\]$", item)
                fields.append(dict(name=am.group(1) if am else item, ctype=ctype, ptr=ptr, const=bool(const), array=int(am.group(2)) if am else None))
        structs.append((m.group(1), fields))
    return defines, enums, structs, prototypes(text[text.index("typedef struct rxr_ctx rxr_ctx;"):])


def prototypes(text):
    """(return type, name, parameter list) of every plain prototype of comment-free text"""
    funcs = []
    for m in re.finditer(r"^([\w\s\*]+?)\b(rxr_\w+)\s*\(([^;{}]*?)\)\s*;", text, flags=re.M | re.S):
        ret = " ".join(m.group(1).split())
        if ret.startswith("typedef"):
            continue
        args = " ".join(m.group(3).split())
        funcs.append((ret, m.group(2), args))
    return funcs


class Layout:
    def __init__(self, structs):
        self.known = {}
        self.structs = structs
        for name, fields in structs:
            self.known[name] = self.compute(fields)

    def field_size_align(self, f):
        if f["ptr"]:
            size, align = 8, 8
        elif f["ctype"] in SCALARS:
            _, size, align = SCALARS[f["ctype"]]
        else:
            st = self.known[f["ctype"]]
            size, align = st["size"], st["align"]
        if f["array"] is not None:
            size *= f["array"]
        return size, align

    def compute(self, fields):
        off, max_align, out = 0, 1, []
        for f in fields:
            size, align = self.field_size_align(f)
            off = (off + align - 1) // align * align
            out.append((f["name"], off))
            off += size
            max_align = max(max_align, align)
        total = (off + max_align - 1) // max_align * max_align
        return dict(size=total, align=max_align, offsets=out)


def rust_type(f):
    base = SCALARS[f["ctype"]][0] if f["ctype"] in SCALARS else f["ctype"]
    if f["ptr"]:
        base = ("*const " if f["const"] else "*mut ") + base
    if f["array"] is not None:
        base = f"[{base}; {f['array']}]"
    return base


def rust_arg(arg):
    """one C parameter -> (name, rust type)"""
    arg = arg.strip()
    m = re.match(r"^(const\s+)?(\w+)\s*(\*{0,2})\s*(\w+)\s*(\[\s*\w*\s*\])?$", arg)
    const, ctype, stars, name, arr = m.group(1), m.group(2), m.group(3), m.group(4), m.group(5)
    base = SCALARS[ctype][0] if ctype in SCALARS else ctype
    if arr:  # `T x[N]` in a parameter list is a pointer
        return name, ("*const " if const else "*mut ") + base
    if stars == "**":
        return name, "*mut *mut " + base
    if stars == "*":
        return name, ("*const " if const else "*mut ") + base
    return name, base


def rust_ret(ret):
    ret = ret.strip()
    if ret == "void":
        return ""
    m = re.match(r"^(const\s+)?(\w+)\s*(\*?)$", ret)
    base = SCALARS[m.group(2)][0] if m.group(2) in SCALARS else m.group(2)
    if m.group(3):
        base = ("*const " if m.group(1) else "*mut ") + base
    return " -> " + base


def define_value(val):
    v = val.strip()
    m = re.match(r"^\(?\s*(\d+)u?\s*<<\s*(\d+)\s*\)?$", v)
    if m:
        return f"{m.group(1)} << {m.group(2)}"
    m = re.match(r"^(\d+)u?$", v)
    return m.group(1) if m else None


def gen_rust(defines, enums, structs, funcs, layout):
    o = []
    o.append("//! Raw bindings of include/rxr.h -- GENERATED by tools/gen_ffi.py from the C header; do not edit.")
    o.append("//! Constants, `#[repr(C)]` mirrors of every struct, the `extern \"C\"` block, and compile-time asserts of every")
    o.append("//! struct size and field offset (the same numbers tests/abi_host.c asserts with the C compiler).")
    o.append("#![allow(non_camel_case_types, dead_code)]")
    o.append("use core::mem::{offset_of, size_of};")
    o.append("use std::os::raw::{c_char, c_int, c_void};")
    o.append("")
    for name, val in defines:
        v = define_value(val)
        if v is not None:
            o.append(f"pub const {name}: u32 = {v};")
    o.append("")
    for tname, items in enums:
        ty = "c_int" if tname == "rxr_status" else "u32"
        if tname:
            o.append(f"// enum {tname}")
        for k, v in items:
            o.append(f"pub const {k}: {ty} = {v};")
        o.append("")
    o.append("#[repr(C)]\npub struct rxr_ctx {\n    _private: [u8; 0],\n}\n")
    for name, fields in structs:
        o.append("#[repr(C)]\n#[derive(Clone, Copy)]")
        o.append(f"pub struct {name} {{")
        for f in fields:
            o.append(f"    pub {f['name']}: {rust_type(f)},")
        o.append("}")
        st = layout.known[name]
        o.append(f"const _: () = assert!(size_of::<{name}>() == {st['size']});")
        for fname, off in st["offsets"]:
            o.append(f"const _: () = assert!(offset_of!({name}, {fname}) == {off});")
        o.append("")
    o.append('extern "C" {')
    for ret, name, args in funcs:
        params = [] if args in ("", "void") else [rust_arg(a) for a in args.split(",")]
        o.append(f"    pub fn {name}({', '.join(f'{n}: {t}' for n, t in params)}){rust_ret(ret)};")
    o.append("}")
    return "\n".join(o) + "\n"


def gen_asserts(structs, layout):
    o = ["/* GENERATED by tools/gen_ffi.py from include/rxr.h; do not edit.  The sizes and offsets the Rust mirror",
         " * (shim/rusterix-hip-shim/src/ffi.rs) asserts, checked here by the C compiler (tests/abi_host.c). */",
         "#include <stddef.h>", ""]
    for name, fields in structs:
        st = layout.known[name]
        o.append(f'_Static_assert(sizeof({name}) == {st["size"]}, "sizeof({name})");')
        o.append(f'_Static_assert(_Alignof({name}) == {st["align"]}, "alignof({name})");')
        for fname, off in st["offsets"]:
            o.append(f'_Static_assert(offsetof({name}, {fname}) == {off}, "offsetof({name}, {fname})");')
        o.append("")
    return "\n".join(o)


def py_type(decl):
    """THE type rule of rusterix_amd/abi.py's two tables, for a parameter (`const float *lo`, `uint32_t out[3]`) or a return type:
    a scalar is its ctypes scalar; `char *` / `const char *` is c_char_p; every other pointer, `T x[N]` parameter or `T **` is c_void_p
    -- which as an argument type takes byref(...), ctypes arrays and pointers, c_void_p, ints and None alike; `void` is None."""
    decl = " ".join(decl.replace("*", " * ").split())
    if "*" in decl or "[" in decl:
        return "c_char_p" if re.match(r"^(const )?char \*( \w+)?$", decl) else "c_void_p"
    words = [w for w in decl.split() if w != "const"]
    if " ".join(words) not in PY_SCALARS:  # (a parameter carries its name behind the type)
        words = words[:-1]
    return PY_SCALARS[" ".join(words)]


def py_field(f, struct_names):
    if f["ptr"]:  # a pointer to a struct of the header keeps its type; every other pointer is an address
        base = f"POINTER({f['ctype']})" if f["ctype"] in struct_names else "c_void_p"
    else:
        base = f["ctype"] if f["ctype"] in struct_names else PY_SCALARS[f["ctype"]]
    return base if f["array"] is None else f"{base} * {f['array']}"


def split_args(args):
    return [] if args in ("", "void") else args.split(",")


def gen_python(defines, enums, structs, funcs, debug_funcs):
    o = ["# GENERATED by tools/gen_ffi.py from include/rxr.h and rusterix_amd/csrc/rxr_debug.h; do not edit.",
         '"""The ctypes mirror of the C ABI: the constants and structs of include/rxr.h, the signature of every entry point of rxr.h',
         "(SIGNATURES) and of every test entry point of rxr_debug.h (DEBUG_SIGNATURES), and declare(), which types a loaded library",
         'with them.  The type rule of the tables is tools/gen_ffi.py::py_type; tests/test_abi_python_cpu.py checks the layouts."""',
         "from ctypes import (POINTER, Structure, c_char_p, c_float, c_int, c_int32, c_size_t, c_uint8, c_uint32, c_uint64, c_ulonglong,",
         "                    c_void_p)",
         ""]
    for name, val in defines:
        v = define_value(val)
        if v is not None:
            o.append(f"{name} = {v}")
    o.append("")
    for tname, items in enums:
        if tname:
            o.append(f"# enum {tname}")
        o.extend(f"{k} = {v}" for k, v in items)
        o.append("")
    names = {name for name, _ in structs}
    for name, fields in structs:
        o.append("")
        o.append(f"class {name}(Structure):")
        o.append("    _fields_ = [" + ",\n                ".join(f'("{f["name"]}", {py_field(f, names)})' for f in fields) + "]")
        o.append("")
    for table, fs in (("SIGNATURES", funcs), ("DEBUG_SIGNATURES", debug_funcs)):
        o.append("")
        o.append(table + " = {")
        for ret, name, args in fs:
            o.append(f'    "{name}": ({py_type(ret)}, [{", ".join(py_type(a) for a in split_args(args))}]),')
        o.append("}")
    o.extend(["", "",
              "def declare(lib, partial=False):",
              '    """Sets restype and argtypes of every entry point on a loaded librxr_hip.so and returns the handle.  A missing function of',
              '    SIGNATURES is an error, unless `partial` says that the build links only some of the library\'s files; one of',
              '    DEBUG_SIGNATURES is skipped (rxr_debug_phase_read exists only in a RXR_PHASE_TIMING build)."""',
              "    for name, (restype, argtypes) in {**SIGNATURES, **DEBUG_SIGNATURES}.items():",
              "        f = getattr(lib, name, None) if partial or name in DEBUG_SIGNATURES else getattr(lib, name)",
              "        if f is not None:",
              "            f.restype, f.argtypes = restype, argtypes",
              "    return lib"])
    return "\n".join(o) + "\n"


def main():
    defines, enums, structs, funcs = parse(open(HEADER).read())
    debug_funcs = prototypes(strip_comments(open(DEBUG_HEADER).read()))
    layout = Layout(structs)
    outputs = {FFI_RS: gen_rust(defines, enums, structs, funcs, layout), ASSERTS_H: gen_asserts(structs, layout),
               ABI_PY: gen_python(defines, enums, structs, funcs, debug_funcs)}
    if "--check" in sys.argv:
        stale = [p for p, text in outputs.items() if not os.path.exists(p) or open(p).read() != text]
        for p in stale:
            print("stale:", os.path.relpath(p, ROOT))
        sys.exit(1 if stale else 0)
    for p, text in outputs.items():
        open(p, "w").write(text)
        print("wrote", os.path.relpath(p, ROOT), f"({len(structs)} structs, {len(funcs)} functions)")


if __name__ == "__main__":
    main()
