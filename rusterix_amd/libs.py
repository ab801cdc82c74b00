"""Locates and loads the in-tree native libraries (built by __graft_entry__.build())."""
import ctypes
import os

from . import abi
from .binding import make_api

_HERE = os.path.dirname(os.path.abspath(__file__))
_cached = None


def lib_paths():
    # RXR_HOST_SO / RXR_DEVICE_SO: other builds of the two libraries (tools/sanitize_cpu.sh: host code under AddressSanitizer)
    return dict(rxr=os.environ.get("RXR_DEVICE_SO") or os.path.join(_HERE, "csrc", "librxr_hip.so"),
                host=os.environ.get("RXR_HOST_SO") or os.path.join(_HERE, "csrc", "librusterix_host.so"))


def load_rxr():
    """The C-ABI device library (include/rxr.h)."""
    p = lib_paths()["rxr"]
    if not os.path.exists(p):
        raise RuntimeError(f"{p} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` first "
                           "(there is no CPU fallback)")
    return ctypes.CDLL(p, mode=ctypes.RTLD_GLOBAL)


RxrStats = abi.rxr_stats

_rxr_typed = None


def rxr_abi():
    """The C-ABI library with the result and argument types of every entry point declared (rusterix_amd/abi.py, generated from
    include/rxr.h), for callers that drive a context themselves after `rxh_rasterizer_upload` (bench.py, tools/, tests/)."""
    global _rxr_typed
    if _rxr_typed is None:
        # (RXR_DEVICE_SO: another build, which may link only the files under test -- tools/sanitize_cpu.sh)
        _rxr_typed = abi.declare(load_rxr(), partial="RXR_DEVICE_SO" in os.environ)
    return _rxr_typed


def load():
    global _cached
    if _cached is None:
        load_rxr()
        p = lib_paths()["host"]
        if not os.path.exists(p):
            raise RuntimeError(f"{p} is missing: run __graft_entry__.build() first (there is no CPU fallback)")
        lib = ctypes.CDLL(p)
        lib.rxh_context.restype = ctypes.c_void_p
        lib.rxh_last_error.restype = ctypes.c_char_p
        lib.rxh_set_device.argtypes = [ctypes.c_int]
        lib.rxh_set_devices.argtypes = [ctypes.POINTER(ctypes.c_int), ctypes.c_int]
        lib.rxh_set_device_projection.argtypes = [ctypes.c_int]
        lib.rxh_set_device_edges.argtypes = [ctypes.c_int]
        lib.rxh_set_light_math_exact.argtypes = [ctypes.c_int]
        lib.rxh_rasterizer_upload.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p]
        _cached = make_api(lib, "rxh_", "product")
    return _cached
