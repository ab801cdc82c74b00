"""Which raster kernel drew the last frame (rxr_debug_last_raster_kernel), for every test that names the kernel it is for."""
import ctypes as C


def last_raster_kernel(product):
    """symbol name of the raster kernel the host mirror's context launched last ("" when its last frame launched none)"""
    from rusterix_amd.libs import rxr_abi

    return rxr_abi().rxr_debug_last_raster_kernel(C.c_void_p(product.lib.rxh_context())).decode()


def assert_route(product, expected, what=""):
    got = last_raster_kernel(product)
    assert got == expected, f"{what}: the frame was drawn by {got or 'no raster kernel'}, not by {expected}"
