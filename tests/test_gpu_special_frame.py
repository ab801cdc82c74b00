"""Frame-level parameters with one poisoned number each -- an entry of the view or the projection matrix, the rasterizer's ambient
colour, the animation time -- over the lit map scene and the shaded box grid, in both light-loop modes against the oracle: within the
one step per channel of lit 3D fragments, host- and device-projected.  A NaN in a matrix makes every projected coordinate NaN: the
frame is the miss colour everywhere on both sides; an infinite entry moves some triangles only."""
import ctypes as C

import numpy as np
import pytest

from rusterix_amd import binding as B
from rusterix_amd import scenes

pytestmark = pytest.mark.gpu
NAN, INF = float("nan"), float("inf")
CASES = [("view", 0, NAN), ("view", 5, INF), ("view", 14, -INF), ("view", 10, 0.0), ("view", 15, 0.0), ("view", 12, 1.0e30),
         ("proj", 0, NAN), ("proj", 5, INF), ("proj", 11, 0.0), ("proj", 14, 3.0e38), ("proj", 10, -0.0), ("proj", 15, NAN),
         ("ambient", 0, NAN), ("ambient", 1, INF), ("ambient", 2, -1.0), ("ambient", 3, NAN)]


def build(api, what, index, value, grid):
    cfg = scenes.box_grid_scene(api, n=10, width=320, height=180) if grid else scenes.map_scene(api, width=320, height=180, n_lights=4, logo_size=16)
    base = cfg.setup

    def setup():
        # the scene's own setup() with ONE number replaced on its way into Rasterizer::setup / .ambient
        orig = api.Rasterizer.setup

        def patched(m2d, v, p):
            v, p = np.array(v, np.float32).copy(), np.array(p, np.float32).copy()
            if what == "view":
                v[index] = value
            elif what == "proj":
                p[index] = value
            r = orig(m2d, v, p)
            if what == "ambient":
                plain = r.ambient

                def ambient(v4):
                    a = list(v4)
                    a[index] = value
                    return plain(tuple(a))

                r.ambient = ambient
            return r

        api.Rasterizer.setup = staticmethod(patched)
        try:
            return base()
        finally:
            api.Rasterizer.setup = staticmethod(orig)

    cfg.setup = setup
    return cfg


@pytest.mark.parametrize("device_projection", [False, True])
@pytest.mark.parametrize("grid", [False, True])
def test_poisoned_frame_parameters(oracle, product, grid, device_projection):
    clean = scenes.render(scenes.box_grid_scene(oracle, n=10, width=320, height=180) if grid else scenes.map_scene(oracle, width=320, height=180, n_lights=4, logo_size=16))
    changed = 0
    for exact in (0, 1):
        product.lib.rxh_set_light_math_exact(exact)
        try:
            for what, index, value in CASES:
                product.lib.rxh_set_device_projection(1 if device_projection else 0)
                try:
                    got = scenes.render(build(product, what, index, value, grid))
                finally:
                    product.lib.rxh_set_device_projection(0)
                ref = scenes.render(build(oracle, what, index, value, grid))
                changed += int(not np.array_equal(ref, clean))
                d = np.abs(got.astype(np.int16) - ref.astype(np.int16)).max(axis=2)
                tol = 0 if grid else 1
                assert d.max() <= tol and (d > 0).sum() <= 64, \
                    f"{what}[{index}] = {value} (exact={exact}): {int((d > tol).sum())} pixels beyond {tol}, {int((d > 0).sum())} differ, max {int(d.max())}; first at {np.argwhere(d > 0)[:2].tolist()}"
        finally:
            product.lib.rxh_set_light_math_exact(0)
    assert changed >= 16, f"only {changed} of {2 * len(CASES)} poisoned frames differ from the clean one: the poison does not arrive"
