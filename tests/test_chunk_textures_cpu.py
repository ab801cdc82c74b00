"""Resident chunk textures without a GPU (include/rxr.h, rusterix_amd/csrc/rxr_chunk_tex.hip): rxr_check_chunk_textures' refusals, each
with its message, the ABI staying functions-only (the generated files current, the layout asserts untouched), and the mirror's
per-chunk generation counter that decides whether a registration is still current (Chunk::textures_generation)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import rusterix_amd
from rusterix_amd import binding as B
from rusterix_amd.abi import RXR_ERR_INVALID, RXR_OK, rxr_texture as Tex

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def check(sizes, terrain, first, slots, n_chunks=None, null=(), with_bytes=True):
    """rxr_check_chunk_textures over slots of `sizes` (no texel is read: one shared buffer stands for every rgba); (status, message)"""
    rxr = rusterix_amd.rxr_abi()
    some = np.zeros(16, np.uint8)
    tex = (Tex * max(len(sizes), 1))()
    for t, (w, h) in zip(tex, sizes):
        t.rgba, t.width, t.height = (some.ctypes.data if with_bytes else None), w, h
    terrain, slots = np.asarray(terrain, np.int32), np.asarray(slots, np.int32)
    first = np.asarray(first, np.uint32)
    args = dict(textures=C.cast(tex, C.c_void_p), terrain=terrain.ctypes.data, first=first.ctypes.data, slots=slots.ctypes.data)
    for k in null:
        args[k] = None
    msg = C.create_string_buffer(512)
    rc = rxr.rxr_check_chunk_textures(args["textures"], len(sizes), args["terrain"], args["first"], args["slots"],
                                      len(terrain) if n_chunks is None else n_chunks, msg, 512)
    return rc, msg.value.decode()


def test_a_well_formed_registration_is_accepted():
    assert check([(4, 4), (64, 64), (3, 5)], [0, -1], [0, 2, 3], [1, -1, 2]) == (RXR_OK, "")
    assert check([(7, 9)], [0, 0, 0], [0, 0, 0, 0], []) == (RXR_OK, "")       # a slot named by several chunks, no shader textures


def test_the_empty_set_and_a_slot_without_bytes_are_accepted():
    assert check([], [], [0], [], n_chunks=0, null=("textures", "terrain", "first", "slots")) == (RXR_OK, "")
    assert check([(256, 256)], [0], [0, 0], [], with_bytes=False) == (RXR_OK, "")


@pytest.mark.parametrize("sizes, terrain, first, slots, kw, expect", [
    ([(0, 4)], [0], [0, 0], [], {}, "textures[0]: a side of 0"),
    ([(4, 4), (4, 0)], [0], [0, 0], [], {}, "textures[1]: a side of 0"),
    ([(32769, 1)], [0], [0, 0], [], {}, "textures[0]: a side above 32768"),
    ([(1, 40000)], [0], [0, 0], [], {}, "textures[0]: a side above 32768"),
    ([(32768, 32768), (32768, 32768)], [0], [0, 0], [], {}, "textures[1]: chunk textures too large"),      # 2^30 + 2^30 = 2^31 texels
    ([(4, 4)], [1], [0, 0], [], {}, "chunk_terrain[0] = 1: slot out of range"),
    ([(4, 4)], [0, -2], [0, 0, 0], [], {}, "chunk_terrain[1] = -2: slot out of range"),
    ([(4, 4)], [0], [0, 2], [0, 5], {}, "chunk_shader_slots[1] = 5: slot out of range"),
    ([(4, 4)], [0, 0], [0, 2, 1], [0, 0], {}, "chunk_shader_first[2]: the prefix decreases"),
    ([(4, 4)], [0], [1, 1], [0], {}, "chunk_shader_first[0] is not 0"),
    ([(4, 4)], [0], [0, 0], [], dict(null=("textures",)), "NULL textures"),
    ([(4, 4)], [0], [0, 0], [], dict(null=("terrain",)), "NULL chunk_terrain"),
    ([(4, 4)], [0], [0, 0], [], dict(null=("first",)), "NULL chunk_terrain / chunk_shader_first"),
    ([(4, 4)], [0], [0, 1], [0], dict(null=("slots",)), "NULL chunk_shader_slots"),
])
def test_malformed_registrations_are_refused_with_their_message(sizes, terrain, first, slots, kw, expect):
    rc, msg = check(sizes, terrain, first, slots, **kw)
    assert rc == RXR_ERR_INVALID and expect in msg, (rc, msg)


def test_just_below_the_texel_limit_is_accepted():
    assert check([(32768, 32768), (32768, 32767)], [0], [0, 0], [])[0] == RXR_OK


def test_the_entry_points_refuse_a_null_context():
    rxr = rusterix_amd.rxr_abi()
    one = np.zeros(4, np.uint32)
    assert rxr.rxr_set_chunk_textures(None, None, 0, None, None, None, 0) == RXR_ERR_INVALID
    assert rxr.rxr_update_chunk_textures(None, one.ctypes.data, 1, one.ctypes.data) == RXR_ERR_INVALID
    assert rxr.rxr_update_chunk_textures_to(None, one.ctypes.data, 1, one.ctypes.data, None) == RXR_ERR_INVALID
    assert rxr.rxr_read_chunk_texture(None, 0, None, None, None) == RXR_ERR_INVALID


def test_generated_files_stay_current_and_the_layout_asserts_untouched():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_ffi.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout
    ffi = open(os.path.join(ROOT, "shim", "rusterix-hip-shim", "src", "ffi.rs")).read()
    for name in ("rxr_check_chunk_textures", "rxr_set_chunk_textures", "rxr_update_chunk_textures", "rxr_update_chunk_textures_to", "rxr_read_chunk_texture"):
        assert f"pub fn {name}(" in ffi
    assert "pub const RXR_ABI_VERSION: u32 = 5;" in ffi
    if os.path.isdir(os.path.join(ROOT, ".git")):
        r = subprocess.run(["git", "-C", ROOT, "diff", "--quiet", "HEAD", "--", "tests/abi_layout_asserts.h"], capture_output=True)
        # (1: the file differs; other codes: git could not look -- --check above still holds)
        assert r.returncode != 1, "tests/abi_layout_asserts.h changed: resident chunk textures must add functions only"


# ---- the mirror's generation counter ----------------------------------------------------------------------------------------------------
def texture(tag, side=8):
    rng = np.random.default_rng(tag)
    return B.Texture(rng.integers(0, 256, side * side * 4, dtype=np.uint8), side, side)


def test_everything_that_assigns_a_chunk_texture_bumps_its_generation_and_reading_does_not(product):
    scene = product.Scene.empty()
    a, b = scene.add_chunk(), scene.add_chunk()
    seen = {a.textures_generation(), b.textures_generation()}
    assert len(seen) == 2 and 0 not in seen                   # process-wide unique stamps

    def bumped(chunk, other):
        g, o = chunk.textures_generation(), other.textures_generation()
        assert g not in seen and o in seen, "the chunk's stamp must be new, its neighbour's unchanged"
        seen.add(g)

    a.terrain(texture(1), origin=(0, 0), size=8)              # assigning a texture
    bumped(a, b)
    a.terrain(None)                                           # ... and taking it away
    bumped(a, b)
    b.add_shader(B.Program([[("Push", 1.0, 0.0, 0.0), "SetColor"]]), texture(2, 16))     # add_shader with its baked texture
    bumped(b, a)
    b.add_shader(B.Program([[("Push", 1.0, 0.0, 0.0), "SetColor"]]), None)               # ... and with None
    bumped(b, a)
    b.touch_textures()                                        # direct field writes
    bumped(b, a)
    # build_chunk_at re-stamps whether or not the bake succeeds (without a device it does not)
    terrain = product.Terrain((1.0, 1.0), 4).set_source(0, 0, texture(3))
    try:
        terrain.build_chunk_at((0, 0), 2, a)
    except B.RasterizeError:
        pass
    bumped(a, b)
    # reading
    a.terrain(texture(4), origin=(0, 0), size=8)
    bumped(a, b)
    before = (a.textures_generation(), b.textures_generation())
    assert a.terrain_texture().width == 8 and b.shader_texture(0).width == 16 and b.shader_texture(1) is None
    assert not a.terrain_texture_stale()
    assert (a.textures_generation(), b.textures_generation()) == before


def test_the_option_is_off_by_default_and_settable(product):
    scene = product.Scene.empty()
    assert scene.resident_chunk_textures is False
    scene.resident_chunk_textures = True
    assert scene.resident_chunk_textures is True
    scene.resident_chunk_textures = False
    assert scene.resident_chunk_textures is False
