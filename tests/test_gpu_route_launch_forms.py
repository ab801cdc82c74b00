"""Every raster route held to its whole frame under bands and stripes.

tests/test_gpu_routes.py pins each of the 22 raster kernels to a scene and tests/test_gpu_route_walk.py holds those frames against the
context's history; both draw every frame as ONE whole-frame launch.  The library launches the same kernels in five other forms, and each
changes the tile-row arithmetic inside the kernel (RasterParams.row0 / row1, tile_y0, tile_stride, compact, out_base_row, bin_row0, the
d3_trow range, the row-span look-up) and the phases of render_impl (rxr_render.hip):

  1  bands on tile rows into caller buffers       rxr_render_rows_to: out_base_row != 0, the host-made records reused (band_on_tiles)
  2  bands off tile rows                          rxr_render_rows + rxr_download_rows: partial first and last tile, k_setup3d's own clamp
  3  compact interleaved stripes                  rxr_render_stripes_to / _batch: tile_stride > 1, compact; no content clamp, no spans
  4  members of a group                           rxr_rasterize and rxr_render_gather on rxr_create_multi: the stripe forms, the strided
                                                  frame-addressed share of the root (tile_stride = n, compact = false), peer and host copies
  5  four raster launches behind one pre-pass     rxr_render_download at >= 2^22 pixels: bin_row0 != 0, band events, the download plan

The reference is never the oracle: it is the same upload's whole frame, rxr_render_rows(ctx, 0, H) + rxr_download_rows, drawn first.  Every
partial launch of that upload must equal it BYTE FOR BYTE, lit routes in their default (relaxed) arithmetic included -- with the one
exception test_bands_off_tile_rows decides from the code.  Behind every launch: the status, the kernel by name (KERNEL_UNDER: for a group,
of every member), the scratch words the next launch assumes zero, and that rxr_debug_rerenders did not move.  Caller buffers are filled
with FILL first, a byte no frame holds in its alpha channel (asserted on the whole frame): rows a launch owns must have lost it, every
other row -- a guard row in front of and behind every band, the stripe slots a rank does not own, the rows of a ragged last stripe beyond
the frame -- must still hold it.

profiles/route_launch_forms/README.md has the times, the mutations the file was tried against and what it found."""
import ctypes as C
import os
import types

import numpy as np
import pytest

import rusterix_amd
from rusterix_amd import distributed as D
from rusterix_amd import scenes
from tests.test_gpu_routes import (MISS, ROUTES, STAGE_TRIS, _oracle_frame, _recreate_context, assert_parity, assert_route, cloud_scene,
                                   knobs, sparse_scene, sparse_span_ends)
from tests.test_gpu_sparse_frames import assert_scratch_clean

gpu = pytest.mark.gpu
TILE = 16
FILL = 9                   # caller buffers of legs 1 to 4 (the existing tests' byte)
FILL_BIG = 0x5A            # the caller's frame of leg 5
BIG_W, BIG_H = 2029, 2075  # 4 210 175 pixels >= 2^22 (rxr_render_download's threshold); 127 x 130 tiles, both edges partial

SMALL = ("k_raster", "k_raster_rl", "k_raster_fused")     # at most RXR_STAGE_TRIS triangles: no binning
SPARSE = ("k_raster_rows_sp", "k_raster_rows_rl_sp")      # sparse_scene under row spans
# the instantiations with RL = true (rxr_kernels.hip: raster_tile<.., RL> / raster_tile_pair<.., RL>): the relaxed light loop and the
# guarded relaxed decisions of shade3d_begin.  k_raster_fused, the interpreter kernels and the compiled ones are RL = false whatever
# RXR_LIGHT_MATH says: their lit frames are exact arithmetic
RELAXED = ("k_raster_rl", "k_raster_rows_rl", "k_raster_rows_rl_sp", "k_raster_rows_cut_rl", "k_raster_pair_rl", "k_raster_chunk_rl",
           "k_raster_chunk_cut_rl")


def exact_twin(name):
    """the kernel of the same frame uploaded under RXR_LIGHT_MATH=exact (rxr_route.h: Facts.rl false)"""
    return {"k_raster_rl": "k_raster", "k_raster_rows_rl_sp": "k_raster_rows_sp"}.get(name, name[:-3] if name.endswith("_rl") else name)


# ---- the kernel a NON-EMPTY launch of each form gets ------------------------------------------------------------------------------
# Derived by hand from raster_route (rxr_route.h) and render_impl (rxr_render.hip).  A route keeps its own name unless a line below says
# otherwise, with the reason; a launch with tiles_y == 0 (an empty band, a rank without a stripe) reports "" under every form.
FORMS = ("bands_on_tiles", "bands_off_tiles", "bands_off_tiles_exact", "stripes", "members", "four_bands")
_STRIDED = {
    # raster_route: `pairs_on && !has_opacity && tile_stride == 1` -- a strided launch's tile rows are not adjacent.  k_raster_pair's own
    # scene has cut-out texels (split_rounds), so what it falls to is k_raster_rows_cut; k_raster_pair_rl's has none
    "k_raster_pair": ("k_raster_rows_cut", "tile_stride != 1: no pair kernel; the scene's cut-out texels (split_rounds) choose the _cut kernel"),
    "k_raster_pair_rl": ("k_raster_rows_rl", "tile_stride != 1: no pair kernel"),
    # content_band: `tile_stride == 1 && !compact` -- no clamp, so clamp_to_content leaves use_spans false and row_spans unattached
    "k_raster_rows_sp": ("k_raster_rows", "stripe launches are never clamped to the content: no row spans"),
    "k_raster_rows_rl_sp": ("k_raster_rows_rl", "stripe launches are never clamped to the content: no row spans"),
}
DEVIATIONS = {
    # bands keep tile_stride 1 (the pair kernels stay) and, under the route's RXR_CONTENT_MIN_TILES=0, content_band applies to every band
    # with rows (saved_tiles < 0 never holds): the _sp kernels stay as well.  Four bands: the last launch's name, the same kernel as all four
    "bands_on_tiles": {},
    "bands_off_tiles": {},
    "four_bands": {},
    # the identity leg of the relaxed routes: uploaded under RXR_LIGHT_MATH=exact, Facts.rl is false
    "bands_off_tiles_exact": {name: (exact_twin(name), "RXR_LIGHT_MATH=exact: the kernel without the relaxed light loop") for name in RELAXED},
    "stripes": _STRIDED,
    # member_render: compact stripes (tile_y0 = i, tile_stride = n); the gather root's own share: the same stride in frame addressing
    "members": _STRIDED,
}
KERNEL_UNDER = {form: {name: DEVIATIONS[form].get(name, (name, ""))[0] for name in ROUTES} for form in FORMS}
# form -> {route: reason}: routes a leg does not run.  Only leg 5 may shed routes (for time), and never these five
EXCLUDED = {}
KEPT_UNDER_FOUR_BANDS = {"k_raster_pair", "k_raster_chunk_cut_rl", "k_raster_rows_rl_sp", "k_raster_vm_v", "k_raster_jit_cut"}

# rxr_debug_last_setup_route of a small frame's launch with rows: (band on tile rows, band off tile rows).  1: the host-made records of
# rxr_upload_frame, 2: a k_setup3d launch with the band's own clamp (Render::small_frame_records).  k_raster_fused builds its records
# inside the raster kernel (fused_small == 1): neither branch is taken and the route stays 0 under every band
SETUP_ROUTE = {"k_raster": (1, 2), "k_raster_rl": (1, 2), "k_raster_fused": (0, 0)}


def routes_of(form):
    return [name for name in sorted(ROUTES) if name not in EXCLUDED.get(form, {})]


# ---- without a GPU --------------------------------------------------------------------------------------------------------------
def test_the_kernel_table_names_every_route_under_every_form():
    assert set(DEVIATIONS) == set(FORMS)
    for form in FORMS:
        assert set(KERNEL_UNDER[form]) == set(ROUTES), form
        assert set(KERNEL_UNDER[form].values()) <= set(ROUTES), form
        for name, (kernel, reason) in DEVIATIONS[form].items():
            assert name in ROUTES and kernel != name and reason, (form, name)
    # the two deviations the forms have: strided launches lose the pair kernels and the row spans; exact arithmetic loses the _rl kernels
    assert set(_STRIDED) == {n for n in ROUTES if "_pair" in n or n.endswith("_sp")}
    assert set(DEVIATIONS["bands_off_tiles_exact"]) == set(RELAXED) == {n for n in ROUTES if n.endswith("_rl") or n.endswith("_rl_sp")}
    assert all(ROUTES[n]["tol"] == "lit" for n in RELAXED)
    assert set(SETUP_ROUTE) == set(SMALL) <= set(ROUTES) and set(SPARSE) <= set(ROUTES)


def test_no_route_is_left_out_of_a_leg():
    """every ROUTES key runs under every leg; only the four-band leg may shed routes, with a reason each, and never the five it is for"""
    assert set(EXCLUDED) <= {"four_bands"}
    left_out = EXCLUDED.get("four_bands", {})
    assert set(left_out) <= set(ROUTES) - KEPT_UNDER_FOUR_BANDS and all(left_out.values())
    assert KEPT_UNDER_FOUR_BANDS <= set(ROUTES)
    for form in FORMS:
        assert set(routes_of(form)) | set(EXCLUDED.get(form, {})) == set(ROUTES)
    assert not EXCLUDED   # (today: nothing is left out)


def test_the_four_band_frame_is_what_the_pair_kernel_needs():
    """render_impl's four bands of 130 tile rows are 32, 33, 32 and 33 rows: the third starts on an odd row and two have an odd count"""
    tiles_y = (BIG_H + TILE - 1) // TILE
    assert BIG_W * BIG_H >= 1 << 22 and BIG_W % TILE and BIG_H % TILE and ((BIG_W + TILE - 1) // TILE, tiles_y) == (127, 130)
    starts = [tiles_y * k // 4 for k in range(5)]
    assert [b - a for a, b in zip(starts, starts[1:])] == [32, 33, 32, 33] and starts[2] % 2 == 1
    assert "RXR_NO_DOWNLOAD_PIPELINE" not in os.environ   # (read once per process: the four-band leg would test render_then_download)


def test_off_tile_cuts_cut_waves():
    """the cuts of leg 2 are off tile rows for every route frame, and all but 0 and H fall inside a wave's four rows somewhere"""
    for name, r in ROUTES.items():
        H = r["kw"].get("height", 150 if r["build"].func is sparse_scene else 131)
        bands = off_tile_bands(H)
        assert (H // 2, H // 2) in bands and len(bands) == 6
        assert [a for a, b in bands if a != b] == sorted({0, 5, H // 3 + 1, H // 2, H - 9})
        assert sum(not on_tile_rows(a, b, H) for a, b in bands if a != b) >= 4, name
        assert 0 < len(rows_of_cut_waves(H)) <= 4 * 4


def test_the_sparse_scene_scales_with_its_sheet_ends_by_a_tile_boundary(oracle):
    """sparse_scene(width, height): at 250 x 150 the ends are today's; at another size (here 517 x 311, no multiple of anything) sheet A
    still ends one pixel left of a tile boundary, sheet B one pixel right of one, and whole tile rows between them are empty"""
    assert sparse_span_ends() == (144, 208) and sparse_span_ends(BIG_W) == (1168, 1680)
    W, H = 517, 311
    end_a, end_b = sparse_span_ends(W)
    assert (end_a, end_b) == (288, 416)
    bare = scenes.render(sparse_scene(oracle, overlay=False, width=W, height=H))
    hit = (bare != np.array(MISS, np.uint8)).any(axis=2)
    ky = H / 150
    rows_a, rows_b = slice(int(4 * ky) + 1, int(60 * ky)), slice(int(84 * ky) + 1, int(148 * ky))
    assert hit[rows_a, end_a - 2].any() and not hit[rows_a, end_a - 1:].any()
    assert hit[rows_b, end_b].any() and not hit[rows_b, end_b + 1:].any()
    rows = [hit[y:y + TILE].any() for y in range(0, H, TILE)]
    assert not any(rows[8:10]) and rows[7] and rows[10], rows


# ---- helpers ----------------------------------------------------------------------------------------------------------------------
def rxr():
    return rusterix_amd.rxr_abi()


def view_of(pointer):
    """what assert_route and assert_scratch_clean ask of `product`, answering for one context (a member of a group)"""
    return types.SimpleNamespace(lib=types.SimpleNamespace(rxh_context=lambda: pointer))


def handle(view):
    return C.c_void_p(view.lib.rxh_context())


def upload(product, cfg):
    """the frame made resident on the host mirror's context; the Rasterizer is returned so that it outlives the renders"""
    r = cfg.setup()
    assert product.lib.rxh_rasterizer_upload(r._h, cfg.scene._h, cfg.width, cfg.height, cfg.tile_size, cfg.assets._h) == 0, product.lib.rxh_last_error()
    return r


def rerenders(view):
    return rxr().rxr_debug_rerenders(handle(view))


def behind_a_launch(view, status, kernel, before, what):
    """the four checks behind every launch: status, kernel name, scratch, and that nothing was rendered again behind the caller's back"""
    ctx = handle(view)
    assert status == 0, f"{what}: status {status}: {rxr().rxr_last_error(ctx)}"
    rc = rxr().rxr_synchronize(ctx)
    assert rc == 0, f"{what}: rxr_synchronize {rc}: {rxr().rxr_last_error(ctx)}"
    assert_route(view, kernel, what)
    assert_scratch_clean(view, what)
    again = rerenders(view) - before
    assert again == 0, f"{what}: rendered {again} more time(s) behind the caller's back (rxr_debug_rerenders)"


def assert_same(got, ref, what):
    if np.array_equal(got, ref):
        return
    d = np.argwhere((got != ref).any(axis=2))
    y, x = d[0]
    raise AssertionError(f"{what}: {len(d)} pixels differ from the whole frame's; first at (x={x}, y={y}): got {got[y, x].tolist()}, whole frame {ref[y, x].tolist()}")


def whole_frame(product, cfg, kernel, what):
    """the reference of every leg: one upload, rxr_render_rows(ctx, 0, H) + rxr_download_rows.  Returns the Rasterizer (to be kept alive
    while the upload is rendered from) and the frame"""
    keep = upload(product, cfg)
    before = rerenders(product)
    ctx = handle(product)
    behind_a_launch(product, rxr().rxr_render_rows(ctx, 0, cfg.height), kernel, before, f"{what}: whole frame")
    frame = np.zeros((cfg.height, cfg.width, 4), np.uint8)
    assert rxr().rxr_download_rows(ctx, frame.ctypes.data, 0, cfg.height) == 0, rxr().rxr_last_error(ctx)
    assert (frame[..., 3] != FILL).all() and (frame[..., 3] != FILL_BIG).all(), f"{what}: the fill byte occurs as an alpha value of the frame"
    assert (frame != np.array(MISS, np.uint8)).any(axis=2).mean() > 0.2, f"{what}: the frame is all but empty"
    frame.setflags(write=False)
    return keep, frame


def fill_framebuffer(product, cfg, value):
    """the context's own framebuffer filled with `value`, behind the whole frame's download.  The legs that render into it draw on top of
    the reference otherwise: a row a launch owns and does not write would hold the reference's bytes and pass"""
    ctx = handle(product)
    assert rxr().rxr_synchronize(ctx) == 0, rxr().rxr_last_error(ctx)
    fb = rxr().rxr_device_framebuffer(ctx)   # (include/rxr.h: width * height * 4 bytes of the last uploaded frame)
    assert fb
    hip = rxr()   # (the HIP runtime the library itself is linked against, through the library's handle)
    hip.hipMemset.argtypes, hip.hipMemset.restype = [C.c_void_p, C.c_int, C.c_size_t], C.c_int
    hip.hipDeviceSynchronize.argtypes, hip.hipDeviceSynchronize.restype = [], C.c_int
    assert hip.hipMemset(fb, value, cfg.width * cfg.height * 4) == 0 and hip.hipDeviceSynchronize() == 0


def device_buffer(rows, width, guard=0):
    """`rows` rows of FILL on the device with `guard` more in front and behind; (tensor, address of the first row proper).  The fill runs on
    torch's default stream and the render on another: no implicit order between the two, hence the synchronize"""
    import torch

    buf = torch.full((rows + 2 * guard, width, 4), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return buf, C.c_void_p(buf.data_ptr() + guard * width * 4)


def assert_owned(got, owned, what):
    """rows a launch owns have lost the fill byte (in every pixel's alpha), the others hold it in every byte"""
    assert (got[~owned] == FILL).all(), f"{what}: rows the launch does not own were written: {np.nonzero((got[~owned] != FILL).any(axis=(1, 2)))[0][:4].tolist()} (of the rows not owned)"
    stale = (got[owned][..., 3] == FILL).any(axis=1)
    assert not stale.any(), f"{what}: rows the launch owns still hold the fill byte: {np.nonzero(owned)[0][stale][:4].tolist()}"


def on_tile_rows(a, b, H):
    """Render::small_frame_records' band_on_tiles"""
    return a % TILE == 0 and (b % TILE == 0 or b == H)


def off_tile_bands(H):
    cuts = sorted({0, 5, H // 3 + 1, H // 2, H - 9, H})
    bands = list(zip(cuts[:-1], cuts[1:]))
    at = [a for a, _ in bands].index(H // 2)
    return bands[:at] + [(H // 2, H // 2)] + bands[at:]   # (the empty band: no launch, no kernel, no bytes)


def rows_of_cut_waves(H):
    """the frame rows whose wave (rows 4w .. 4w + 3 of a tile: raster_tile) is cut by a band edge of off_tile_bands"""
    rows = set()
    for a, b in off_tile_bands(H):
        for c in (a, b):
            if c % 4 and 0 < c < H:
                rows.update(range(c // 4 * 4, min(c // 4 * 4 + 4, H)))
    return sorted(rows)


def setup_route_of(name, a, b, H):
    return 0 if a == b else SETUP_ROUTE[name][0 if on_tile_rows(a, b, H) else 1]


# ---- leg 1: bands on tile rows into caller buffers --------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", routes_of("bands_on_tiles"))
def test_bands_on_tile_rows_into_caller_buffers(product, monkeypatch, name):
    """rxr_render_rows_to over [0, 32) [32, 96) [96, H), each into a buffer of its own (the address handed over is that of the band's first
    row: out_base_row) with a guard row either side; the middle band on a stream of the caller's"""
    import torch

    r = ROUTES[name]
    kernel = KERNEL_UNDER["bands_on_tiles"][name]
    with knobs(product, monkeypatch, r["env"], r["ctx_env"]):
        cfg = r["build"](product)
        keep, whole = whole_frame(product, cfg, name, name)
        ctx, W, H = handle(product), cfg.width, cfg.height
        stream = torch.cuda.Stream()
        for k, (a, b) in enumerate(((0, 32), (32, 96), (96, H))):
            what = f"{name}: band [{a}, {b}) into a caller buffer"
            buf, first_row = device_buffer(b - a, W, guard=1)
            before = rerenders(product)
            status = rxr().rxr_render_rows_to(ctx, a, b, first_row, C.c_void_p(stream.cuda_stream) if k == 1 else None)
            behind_a_launch(product, status, kernel, before, what)
            if name in SMALL:
                assert rxr().rxr_debug_last_setup_route(ctx) == setup_route_of(name, a, b, H), f"{what}: set-up route {rxr().rxr_debug_last_setup_route(ctx)}"
            got = buf.cpu().numpy()
            owned = np.ones(len(got), bool)
            owned[[0, -1]] = False
            assert_owned(got, owned, what)
            assert_same(got[1:-1], whole[a:b], what)
        del keep


# ---- leg 2: bands off tile rows ---------------------------------------------------------------------------------------------------
def draw_off_tile_bands(product, cfg, name, kernel, what):
    """rxr_render_rows + rxr_download_rows over off_tile_bands into a host frame of FILL; the resident frame is the caller's upload"""
    ctx, H = handle(product), cfg.height
    out = np.full((H, cfg.width, 4), FILL, np.uint8)
    fill_framebuffer(product, cfg, FILL)
    for a, b in off_tile_bands(H):
        band = f"{what}: band [{a}, {b})"
        before = rerenders(product)
        behind_a_launch(product, rxr().rxr_render_rows(ctx, a, b), kernel if b > a else "", before, band)
        if name in SMALL:
            assert rxr().rxr_debug_last_setup_route(ctx) == setup_route_of(name, a, b, H), f"{band}: set-up route {rxr().rxr_debug_last_setup_route(ctx)}"
        assert rxr().rxr_download_rows(ctx, out.ctypes.data, a, b) == 0, rxr().rxr_last_error(ctx)
        owned = np.zeros(H, bool)
        owned[:b] = True   # (the bands ascend: everything above this band's end has been drawn, nothing below it)
        assert_owned(out, owned, band)
    return out


@gpu
@pytest.mark.parametrize("name", routes_of("bands_off_tiles"))
def test_bands_off_tile_rows(product, monkeypatch, name):
    """rxr_render_rows + rxr_download_rows over the cuts {0, 5, H // 3 + 1, H // 2, H - 9, H} and one empty band [H // 2, H // 2).

    Is byte identity the contract for a band that does not start and end on tile rows?  For the kernels without the relaxed light loop
    (RL = false: every route not in RELAXED, lit or not): YES.  A pixel outside the band is outside every triangle's clamped pixel box
    (rxr_tri_records: in.row0 / in.row1) and so never `hit`; what that changes is the SET OF LANES behind a wave vote, and the votes of
    the exact paths (rxr_exact_math.h: div1_known, div2, div3, norm3 -- `wave_all(in window)` choosing the division chain over the plain
    quotient) choose between two sequences that return the same correctly rounded float (tests/test_gpu_exact_math_ref.py holds them to
    IEEE references).  The wave-level light culling of shade3d_lights (centre: the first hit lane; radius: the wave's maximum) only ever drops a
    light whose `distance >= end_distance` test fails for every fragment of the wave: it contributes nothing either way.

    For the RL = true kernels: NO, not in the default arithmetic.  shade3d_begin takes the relaxed world position only if
    `wave_all(in_window(vw))`, the relaxed normal and view direction only if `wave_all(sq_in_window(vm2) && (... |n.v| >= guard))`;
    shade3d_lights leaves the prefix loop at `__ballot(!sq_in_window(m2)) & hitmask` and takes the fast point-light term under
    `wave_all(sq_in_window(m2))`.  Each chooses between the relaxed and the exact sequence, which differ in the last bits: ONE grazing
    fragment (|n.v| below the guard) sends its whole wave through the exact sequences.  Cut that fragment's row off and the remaining lanes
    of the wave vote `relaxed`: their colours may move by the arithmetic modes' distance.  So Render::small_frame_records' comment holds,
    and test_a_band_that_is_not_on_tile_rows' identity is a property of the map scene (no fragment fails a guard), not of the library.
    What is asserted for those seven routes, then:
      - in the default arithmetic: byte identity in every row whose wave no band edge cuts (a wave is rows 4w .. 4w + 3 of a tile and
        votes on nothing outside itself: rows_of_cut_waves), the route's own bar (assert_parity, "lit") against the oracle's frame for the
        assembled frame, and the number of pixels that did move is printed;
      - under RXR_LIGHT_MATH=exact (the route's exact twin draws the frame: KERNEL_UNDER["bands_off_tiles_exact"]): byte identity."""
    r = ROUTES[name]
    with knobs(product, monkeypatch, r["env"], r["ctx_env"]):
        cfg = r["build"](product)
        keep, whole = whole_frame(product, cfg, name, name)
        got = draw_off_tile_bands(product, cfg, name, KERNEL_UNDER["bands_off_tiles"][name], name)
        del keep
        if name in RELAXED:
            uncut = np.ones(cfg.height, bool)
            uncut[rows_of_cut_waves(cfg.height)] = False
            moved = int((got != whole).any(axis=2).sum())
            print(f"{name}: {moved} pixels of the rows whose wave a band edge cuts differ from the whole frame's (relaxed arithmetic)")
            assert_same(got[uncut], whole[uncut], f"{name}: off-tile bands, rows of uncut waves")
            assert_parity(got, _oracle_frame(name), r["tol"], f"{name}: off-tile bands against the oracle")
        else:
            assert_same(got, whole, f"{name}: off-tile bands")
    if name in RELAXED:
        with knobs(product, monkeypatch, dict(r["env"], RXR_LIGHT_MATH="exact"), r["ctx_env"]):
            keep, whole = whole_frame(product, cfg, exact_twin(name), f"{name} in exact arithmetic")
            got = draw_off_tile_bands(product, cfg, name, KERNEL_UNDER["bands_off_tiles_exact"][name], f"{name} in exact arithmetic")
            del keep
            assert_same(got, whole, f"{name}: off-tile bands in exact arithmetic")


# ---- leg 3: compact stripes -------------------------------------------------------------------------------------------------------
def owned_rows_of(H, world, rank):
    """which rows of rank's compact buffer [stripes_per_rank * 16] its stripes fill (a ragged last stripe: its rows inside the frame)"""
    owned = np.zeros(D.stripes_per_rank(H, world) * TILE, bool)
    for j, (a, b) in enumerate(D.stripe_rows(H, world, rank)):
        owned[j * TILE:j * TILE + (b - a)] = True
    return owned


@gpu
@pytest.mark.parametrize("name", routes_of("stripes"))
def test_compact_stripes(product, monkeypatch, name):
    """rxr_render_stripes_to for worlds of 2, of 3 and of one more rank than the frame has tile rows (the last rank owns nothing: its buffer
    stays untouched and it reports no kernel), assembled as the all-gather does; rxr_render_stripes_batch with two frames for world 3"""
    import torch

    r = ROUTES[name]
    kernel = KERNEL_UNDER["stripes"][name]
    with knobs(product, monkeypatch, r["env"], r["ctx_env"]):
        cfg = r["build"](product)
        keep, whole = whole_frame(product, cfg, name, name)
        ctx, W, H = handle(product), cfg.width, cfg.height
        n_stripes = (H + TILE - 1) // TILE
        stream = torch.cuda.Stream()
        for world in (2, 3, n_stripes + 1):
            parts = []
            for rank in range(world):
                what = f"{name}: stripes of rank {rank} of {world}"
                owned = owned_rows_of(H, world, rank)
                assert owned.any() == (rank < n_stripes)
                buf, first_row = device_buffer(len(owned), W)
                before = rerenders(product)
                status = rxr().rxr_render_stripes_to(ctx, rank, world, first_row, C.c_void_p(stream.cuda_stream) if rank == 1 else None)
                behind_a_launch(product, status, kernel if owned.any() else "", before, what)
                parts.append(buf.cpu().numpy())
                assert_owned(parts[-1], owned, what)
            assert_same(D.assemble_numpy(np.concatenate(parts, axis=0), H, W, world), whole, f"{name}: the stripes of {world} ranks")
        world, frames = 3, 2
        share = D.stripes_per_rank(H, world) * TILE
        parts = []
        for rank in range(world):
            what = f"{name}: a batch of {frames} frames, rank {rank} of {world}"
            buf, first_row = device_buffer(frames * share, W)
            before = rerenders(product)
            status = rxr().rxr_render_stripes_batch(ctx, rank, world, frames, first_row, C.c_size_t(share * W * 4), None)
            behind_a_launch(product, status, kernel, before, what)
            parts.append(buf.cpu().numpy().reshape(frames, share, W, 4))
            for k in range(frames):
                assert_owned(parts[-1][k], owned_rows_of(H, world, rank), f"{what}, frame {k}")
        for k in range(frames):
            assert_same(D.assemble_numpy(np.concatenate([p[k] for p in parts], axis=0), H, W, world), whole, f"{name}: frame {k} of the batch")
        del keep


# ---- leg 4: members of a group ----------------------------------------------------------------------------------------------------
def behind_a_group_launch(members, status, group, kernel, before, what):
    assert status == 0, f"{what}: status {status}: {rxr().rxr_last_error(group)}"
    rc = rxr().rxr_synchronize(group)
    assert rc == 0, f"{what}: rxr_synchronize {rc}: {rxr().rxr_last_error(group)}"
    for i, m in enumerate(members):
        behind_a_launch(m, 0, kernel, before[i], f"{what}, member {i}")


@gpu
@pytest.mark.parametrize("name", routes_of("members"))
def test_members_of_a_group(product, monkeypatch, name):
    """2 and 3 logical members on device 0: rxr_rasterize into host pixels (compact stripes, host copies), rxr_render_gather to root 0 and
    to the last member -- into the root's framebuffer and into a caller's device buffer (the root's share strided in frame addressing, the
    others' by device copies) -- against the frame of the single context"""
    import torch

    r = ROUTES[name]
    kernel = KERNEL_UNDER["members"][name]
    with knobs(product, monkeypatch, r["env"], r["ctx_env"]):
        cfg = r["build"](product)
        keep, whole = whole_frame(product, cfg, name, name)
        del keep
        W, H = cfg.width, cfg.height
        try:
            for n in (2, 3):
                assert (H + TILE - 1) // TILE >= n   # (every member owns a stripe and reports a kernel)
                product.lib.rxh_set_devices((C.c_int * n)(*([0] * n)), n)   # (created under the route's create-time variables)
                group = C.c_void_p(product.lib.rxh_context())
                assert group.value, product.lib.rxh_last_error()
                assert rxr().rxr_member_count(group) == n
                members = [view_of(rxr().rxr_member(group, i)) for i in range(n)]
                what = f"{name}: {n} members, rxr_rasterize"
                before = [rerenders(m) for m in members]
                out = np.full(W * H * 4, FILL, np.uint8)
                got = scenes.render(cfg, out)   # (Rasterizer::rasterize: raises on an error status)
                behind_a_group_launch(members, 0, group, kernel, before, what)
                assert_owned(got, np.ones(H, bool), what)
                assert_same(got, whole, what)
                keep = upload(product, cfg)
                stream = torch.cuda.Stream()
                for root in (0, n - 1):
                    what = f"{name}: {n} members, gather into member {root}'s framebuffer"
                    before = [rerenders(m) for m in members]
                    behind_a_group_launch(members, rxr().rxr_render_gather(group, root, None, None), group, kernel, before, what)
                    got = np.full((H, W, 4), FILL, np.uint8)
                    assert rxr().rxr_download_rows(handle(members[root]), got.ctypes.data, 0, H) == 0, rxr().rxr_last_error(handle(members[root]))
                    assert_same(got, whole, what)
                    what = f"{name}: {n} members, gather into a caller buffer, root {root}"
                    buf, first_row = device_buffer(H, W, guard=1)
                    before = [rerenders(m) for m in members]
                    status = rxr().rxr_render_gather(group, root, first_row, C.c_void_p(stream.cuda_stream))
                    stream.synchronize()
                    behind_a_group_launch(members, status, group, kernel, before, what)
                    got = buf.cpu().numpy()
                    owned = np.ones(H + 2, bool)
                    owned[[0, -1]] = False
                    assert_owned(got, owned, what)
                    assert_same(got[1:-1], whole, what)
                del keep
        finally:
            product.lib.rxh_set_device(0)
            product.lib.rxh_set_device_projection(0)


# ---- leg 5: four raster launches behind one pre-pass ------------------------------------------------------------------------------
def big_scene(api, name):
    """the route's scene at BIG_W x BIG_H: cloud_scene's camera takes the frame size, sparse_scene scales its pixel positions"""
    r = ROUTES[name]
    assert r["build"].func in (cloud_scene, sparse_scene)
    return r["build"].func(api, **dict(r["kw"], width=BIG_W, height=BIG_H))


def _four_band_cases():
    cases = [pytest.param(name, False, id=name) for name in routes_of("four_bands")]
    # the sparse routes once more with RXR_NO_COLUMN_TRIM: whole-row copies against the strided copies and host fills of the run above
    return cases + [pytest.param(name, True, id=f"{name}-whole-rows") for name in SPARSE if name in routes_of("four_bands")]


@gpu
@pytest.mark.parametrize("name, whole_rows", _four_band_cases())
def test_four_raster_launches_behind_one_pre_pass(product, monkeypatch, name, whole_rows):
    """rxr_render_download of the route's scene at 2029 x 2075 into a frame of 0x5A, on a context that has downloaded nothing yet
    (rxr_debug_download_bytes starts at zero): link bytes plus host-fill bytes are the whole frame's -- the banded path ran, not
    render_then_download -- and every byte equals the one-launch frame's"""
    r = ROUTES[name]
    kernel = KERNEL_UNDER["four_bands"][name]
    env = dict(r["env"], RXR_NO_COLUMN_TRIM="1") if whole_rows else r["env"]
    with knobs(product, monkeypatch, env, r["ctx_env"]):
        if not r["ctx_env"]:
            _recreate_context(product)
        cfg = big_scene(product, name)
        if name in SMALL:
            assert cfg.n_triangles <= STAGE_TRIS, f"{name}: {cfg.n_triangles} triangles"
        keep, whole = whole_frame(product, cfg, name, f"{name} at {BIG_W} x {BIG_H}")
        ctx, W, H = handle(product), cfg.width, cfg.height
        if name in SPARSE:
            end_a, end_b = sparse_span_ends(W)
            hit, ky = (whole != np.array(MISS, np.uint8)).any(axis=2), H / 150
            rows_a, rows_b = slice(int(4 * ky) + 1, int(60 * ky)), slice(int(84 * ky) + 1, int(148 * ky))
            assert hit[rows_a, end_a - 2].any() and not hit[rows_a, end_a - 1:].any(), "sheet A does not end one pixel left of its tile boundary"
            assert hit[rows_b, end_b].any() and not hit[rows_b, end_b + 1:].any(), "sheet B does not end one pixel right of its tile boundary"
        sent = (C.c_uint64 * 2)()
        assert rxr().rxr_debug_download_bytes(ctx, sent) == 0 and list(sent) == [0, 0], list(sent)
        what = f"{name}: rxr_render_download at {W} x {H}"
        out = np.full((H, W, 4), FILL_BIG, np.uint8)
        fill_framebuffer(product, cfg, FILL_BIG)
        before = rerenders(product)
        behind_a_launch(product, rxr().rxr_render_download(ctx, out.ctypes.data_as(C.POINTER(C.c_uint8))), kernel, before, what)
        assert rxr().rxr_debug_download_bytes(ctx, sent) == 0
        assert sent[0] + sent[1] == W * H * 4, f"{what}: {sent[0]} bytes over the link and {sent[1]} written by the host are not the frame's {W * H * 4}"
        if name in SPARSE and not whole_rows:
            assert 0 < sent[1] and sent[0] < 0.8 * W * H * 4, f"{what}: the row ends outside the spans travelled: {list(sent)}"
        del keep
        assert_same(out, whole, what)
