"""rusterix_amd/abi.py, the generated ctypes mirror of include/rxr.h and rusterix_amd/csrc/rxr_debug.h (tools/gen_ffi.py): current, laid
out as the C compiler lays the structs out (the numbers of tests/abi_layout_asserts.h, which tests/abi_host.c compiles), complete, and
loadable onto the built library.  CPU only."""
import ctypes as C
import os
import subprocess
import sys

import rusterix_amd
from rusterix_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_ffi  # noqa: E402

_, _, STRUCTS, FUNCS = gen_ffi.parse(open(gen_ffi.HEADER).read())
DEBUG_FUNCS = gen_ffi.prototypes(gen_ffi.strip_comments(open(gen_ffi.DEBUG_HEADER).read()))
PHASE_TIMING_ONLY = {"rxr_debug_phase_read"}   # defined under RXR_PHASE_TIMING alone (rxr_debug.h)


def test_generated_files_are_current():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_ffi.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert open(gen_ffi.ABI_PY).readline().startswith("# GENERATED") and "do not edit" in open(gen_ffi.ABI_PY).readline()


def test_every_struct_is_laid_out_as_in_c():
    layout = gen_ffi.Layout(STRUCTS)
    assert len(STRUCTS) >= 18
    for name, fields in STRUCTS:
        cls, want = getattr(abi, name), layout.known[name]
        assert issubclass(cls, C.Structure)
        assert C.sizeof(cls) == want["size"] and C.alignment(cls) == want["align"], name
        assert [f for f, _ in cls._fields_] == [f["name"] for f in fields], name
        for field, offset in want["offsets"]:
            assert getattr(cls, field).offset == offset, (name, field)


def test_every_prototype_has_its_signature():
    assert len(FUNCS) >= 94 and len(DEBUG_FUNCS) >= 29
    for table, funcs in ((abi.SIGNATURES, FUNCS), (abi.DEBUG_SIGNATURES, DEBUG_FUNCS)):
        assert list(table) == [name for _, name, _ in funcs]
        for ret, name, args in funcs:
            restype, argtypes = table[name]
            assert len(argtypes) == len(gen_ffi.split_args(args)), name
            assert (restype is None) == (ret == "void"), name
    # a pointer that is cut to 32 bits is what a wrong table costs: none may be left to ctypes' default int
    assert abi.SIGNATURES["rxr_member"][0] is C.c_void_p and abi.SIGNATURES["rxr_last_error"] == (C.c_char_p, [C.c_void_p])
    assert abi.SIGNATURES["rxr_render_rows"] == (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32])
    assert abi.SIGNATURES["rxr_trace_rand"][0] is C.c_float


def test_constants_follow_the_header():
    assert (abi.RXR_OK, abi.RXR_ERR_INVALID, abi.RXR_ERR_UNSUPPORTED) == (0, -1, -4)
    assert abi.RXR_ABI_VERSION == 5 and abi.RXR_FLAG_HAS_SUN == 1 << 6 and abi.RXR_RAY_REFRESH_INFO_WORDS == 8


def test_declare_types_the_built_library():
    lib = abi.declare(rusterix_amd.load_rxr())
    for name, (restype, argtypes) in {**abi.SIGNATURES, **abi.DEBUG_SIGNATURES}.items():
        if name in PHASE_TIMING_ONLY and not hasattr(lib, name):
            continue
        f = getattr(lib, name)   # (every other debug entry point must be in the library: declare() skips what is missing)
        assert f.restype is restype and list(f.argtypes) == argtypes, name


def test_the_package_exports_the_generated_stats():
    assert rusterix_amd.RxrStats is abi.rxr_stats
    assert rusterix_amd.rxr_abi() is rusterix_amd.rxr_abi()
