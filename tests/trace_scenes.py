"""The small scenes of the path tracer's tests (tests/test_trace_cpu.py, tests/test_gpu_trace.py): dicts in tests/trace_ref.py's form,
built from boxes in Batch3D::from_box's vertex order with compute_vertex_normals' normals."""
import numpy as np

from rusterix_amd import binding as B
from rusterix_amd import trace as T
from tests import trace_ref as TR

F = np.float32


def box(x, y, z, w, h, d, **kw):
    """Batch3D::from_box (src/batch/batch3d.rs:140-229) with computed vertex normals, as a rusterix_amd.trace.mesh"""
    X, Y, Z = x + w, y + h, z + d
    v = np.array([(x, y, z, 1), (X, y, z, 1), (X, Y, z, 1), (x, Y, z, 1), (x, y, Z, 1), (X, y, Z, 1), (X, Y, Z, 1), (x, Y, Z, 1),
                  (x, y, z, 1), (x, Y, z, 1), (x, Y, Z, 1), (x, y, Z, 1), (X, y, z, 1), (X, Y, z, 1), (X, Y, Z, 1), (X, y, Z, 1),
                  (x, Y, z, 1), (X, Y, z, 1), (X, Y, Z, 1), (x, Y, Z, 1), (x, y, z, 1), (X, y, z, 1), (X, y, Z, 1), (x, y, Z, 1)], F)
    idx = np.array([0, 1, 2, 0, 2, 3, 4, 6, 5, 4, 7, 6, 8, 9, 10, 8, 10, 11, 12, 14, 13, 12, 15, 14, 16, 17, 18, 16, 18, 19, 20, 23, 22, 20, 22, 21],
                   np.uint32).reshape(-1, 3)
    uv = np.tile(np.array([(0, 1), (1, 1), (1, 0), (0, 0)], F), (6, 1))
    nrm = np.zeros((24, 3), F)
    for tri in idx:
        p0, p1, p2 = (v[int(i), :3] for i in tri)
        c = np.cross(p1 - p0, p2 - p0).astype(F)
        c = c / np.sqrt(np.dot(c, c), dtype=F)
        nrm[tri] += c
    nrm = (nrm / np.sqrt((nrm * nrm).sum(axis=1, dtype=F))[:, None]).astype(F)
    return T.mesh(v, idx, uv, nrm, **kw)


def texture(seed, w, h, opaque=True):
    rng = np.random.default_rng(seed)
    px = rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8)
    if opaque:
        px[..., 3] = 255
    return B.Texture(px, w, h)


def point_light(pos, color=(1.0, 0.9, 0.8), intensity=1.2, start=1.0, end=9.0, flicker=0.0, kind=B.LIGHT_POINT):
    l = B.Light(kind).with_position(pos).with_color(color).with_intensity(intensity).with_start_distance(start).with_end_distance(end).with_flicker(flicker)
    l.direction, l.normal, l.width, l.height = (0.1, -0.9, 0.3), (0.0, -1.0, 0.2), 2.0, 1.5
    return l.compile()


PIXEL = lambda r, g, b: (T.SOURCE_PIXEL, 0, (r, g, b, 255))


def room(material=None, panel_material=(T.EMISSIVE, T.MOD_NONE, 1.0), sample_mode=0, box_source=(T.SOURCE_STATIC_TILE, 0, (0, 0, 0, 0)),
         box_repeat=0, lights=None, animation_frame=1, extra=()):
    """an 8 x 5 x 8 room (walls, floor and ceiling one outward-facing box each side: six slabs), a textured box inside, an emissive panel
    under the ceiling and two point lights; the camera of `cameras` stands inside"""
    grey, red, green = PIXEL(200, 200, 200), PIXEL(220, 60, 50), PIXEL(60, 200, 70)
    slabs = [box(0, -0.5, 0, 8, 0.5, 8, source=grey, material=material),                 # floor
             box(0, 5, 0, 8, 0.5, 8, source=grey, material=material),                    # ceiling
             box(-0.5, 0, 0, 0.5, 5, 8, source=red, material=material),                  # left
             box(8, 0, 0, 0.5, 5, 8, source=green, material=material),                   # right
             box(0, 0, 8, 8, 5, 0.5, source=grey, material=material, list=T.LIST_DYNAMIC),   # back
             box(0, 0, -0.5, 8, 5, 0.5, source=grey, material=material, list=T.LIST_CHUNK, chunk=0)]   # behind the camera
    inner = box(2.5, 0, 4, 2, 2, 2, source=box_source, repeat_mode=box_repeat, material=material)
    panel = box(3, 4.8, 3, 2, 0.2, 2, source=PIXEL(255, 240, 220), material=panel_material)
    if lights is None:
        lights = [point_light((2.0, 3.5, 2.5)), point_light((6.5, 2.0, 6.0), color=(0.5, 0.7, 1.0), intensity=2.0, flicker=0.4)]
    return dict(meshes=slabs[5:] + slabs[:5] + [inner, panel] + list(extra),   # (rxr_set_meshes order: chunk meshes first, then static, dynamic)
                static_tiles=[B.Tile([texture(5, 8, 8), texture(6, 5, 7)]), B.Tile([texture(7, 4, 4)])],
                dynamic_tiles=[B.Tile([texture(8, 6, 3, opaque=False)])], lights=lights, sample_mode=sample_mode, animation_frame=animation_frame)


def ordered(scene):
    """the scene with its meshes in rxr_set_meshes order (stable): chunk lists, static, dynamic, overlay"""
    rank = {T.LIST_CHUNK_OPACITY: 0, T.LIST_CHUNK: 0, T.LIST_CHUNK_TERRAIN: 0, T.LIST_STATIC: 1, T.LIST_DYNAMIC: 2, T.LIST_OVERLAY: 3}
    return dict(scene, meshes=sorted(scene["meshes"], key=lambda m: rank[m["list"]]))


def cameras(width, height):
    return dict(firstp=T.camera_firstp((4.0, 2.2, 0.6), (4.1, 1.9, 6.0), 70.0, width, height),
                orbit=T.camera_orbit((4.0, 1.5, 4.5), 3.6, -1.5, 0.35, 75.0, width, height),
                iso=T.camera_iso((4.0, 1.0, 4.5), 250.0, 30.0, 3.0, 2.5, width, height))


def load(tracer, scene):
    """makes `scene` the Tracer's"""
    tracer.set_textures(scene["static_tiles"], scene["dynamic_tiles"])
    tracer.set_chunk_textures(scene.get("chunks", []))
    tracer.set_meshes(scene["meshes"])
    tracer.set_scene(scene["lights"], scene["sample_mode"], scene["animation_frame"], chunks=scene.get("chunks", []))
    return tracer


MATTE_1 = (T.MATTE, T.MOD_NONE, 1.0)


def diffuse_room():
    """a matte room with one light and one emissive panel"""
    return room(material=MATTE_1, lights=[point_light((4.0, 3.0, 3.0), intensity=1.5)], box_source=PIXEL(180, 160, 90))


def diffuse_case():
    """(scene, camera, width, height, seed) of the diffuse criterion: 8 bounces, frames 0..3"""
    return diffuse_room(), cameras(24, 16)["firstp"], 24, 16, 11


def diffuse_tolerance(orc, table):
    """(the restatement of diffuse_case with cos and sin correctly rounded, the tolerance, how many pixels' paths disagree): four more
    runs move cos and sin by +-4 float32 ulps before rounding, every combination of signs -- the bound tests/test_gpu_libm_ulp.py
    asserts for the device's.  Over the pixels whose path signatures agree with the first run's in every frame, 4 times the largest
    difference of an accumulated float over the four runs is the tolerance; a pixel disagrees if it does in any of them."""
    scene, cam, w, h, seed = diffuse_case()
    zero = np.zeros((h, w, 4), F)
    a, sa = TR.trace(orc, scene, cam, w, h, 0, 4, seed, 8, zero, table, signatures=True)
    worst, disagree = 0.0, np.zeros((h, w), bool)
    for cs, sn in ((4.0, 4.0), (4.0, -4.0), (-4.0, 4.0), (-4.0, -4.0)):
        b, sb = TR.trace(orc, scene, cam, w, h, 0, 4, seed, 8, zero, table, trig=TR.trig_shifted(cs, sn), signatures=True)
        agree = np.array([all(fa[i] == fb[i] for fa, fb in zip(sa, sb)) for i in range(w * h)]).reshape(h, w)
        worst = max(worst, float(np.abs(a - b).max(axis=2)[agree].max()))
        disagree |= ~agree
    return a, 4.0 * worst, int(disagree.sum())


def mirror_scene(api, scene):
    """(Scene, Assets) of the host mirror (rusterix_amd.load()) for a scene dict whose meshes are in rxr_set_meshes order (`ordered`)"""
    sc, assets = api.Scene.empty(), api.Assets.default().textures(scene["static_tiles"])
    for tile in scene["dynamic_tiles"]:
        sc.add_dynamic_texture(tile)
    sc.lights(scene["lights"])
    sc.set_animation_frame(scene["animation_frame"])
    chunks = []
    n_chunks = max([len(scene.get("chunks", []))] + [m["chunk"] + 1 for m in scene["meshes"]])
    for c in range(n_chunks):
        ch = sc.add_chunk()
        if c < len(scene.get("chunks", [])):
            d = scene["chunks"][c]
            ch.terrain(d.get("terrain_texture"), d["origin"], d["size"])
        chunks.append(ch)
    for m in scene["meshes"]:
        kind, index, pixel = m["source"]
        b = api.Batch3D.new(m["vertices"], m["indices"], m["uvs"]).normals(m["normals"]).source(B.PixelSource(kind, index, pixel)).repeat_mode(m["repeat_mode"])
        if m.get("material") is not None:
            b.material(*m["material"])
        lst, ch = m["list"], (chunks[m["chunk"]] if m["chunk"] >= 0 else None)
        {T.LIST_CHUNK_OPACITY: lambda: ch.add_batch3d_opacity(b), T.LIST_CHUNK: lambda: ch.add_batch3d(b), T.LIST_CHUNK_TERRAIN: lambda: ch.terrain_batch3d(b),
         T.LIST_STATIC: lambda: sc.add_d3_static(b), T.LIST_DYNAMIC: lambda: sc.add_d3_dynamic(b), T.LIST_OVERLAY: lambda: sc.add_d3_overlay(b)}[lst]()
    return sc, assets


def terrain_room(origin=(2, -3), tex=None):
    """the room with its floor a terrain-sourced mesh of chunk 0 (a texture of 3 x 3 pixels a tile, part of the floor outside it: clamped)
    and its box a terrain-sourced mesh of chunk 1, which has no texture (zero)"""
    scene = room(box_source=(T.SOURCE_TERRAIN, 0, (0, 0, 0, 0)))
    scene["chunks"] = [dict(terrain_texture=tex if tex is not None else texture(22, 16, 24), origin=origin, size=8), dict(terrain_texture=None, origin=(0, 0), size=8)]
    scene["meshes"][1].update(source=(T.SOURCE_TERRAIN, 0, (0, 0, 0, 0)), list=T.LIST_CHUNK_TERRAIN, chunk=0)
    scene["meshes"][-2].update(list=T.LIST_CHUNK, chunk=1)
    return scene


def byte_rule_values(w, h):
    """accumulation values for the to_u8 rule: the first pixel (0, 0.0031308, 1, 1), then a spread over [-0.5, 2.5] with alpha away from 1,
    NaN, infinities and the values next to the linear segment's threshold"""
    rng = np.random.default_rng(77)
    a = (rng.random((h, w, 4), dtype=F) * F(3.0) - F(0.5)).astype(F)
    a[1] = (rng.random((w, 4), dtype=F) ** F(4.0)).astype(F)          # dark values, where the curve is steep
    a[2, :, 3] = np.linspace(-1.0, 2.0, w, dtype=F)
    a[0, 0] = (0.0, 0.0031308, 1.0, 1.0)
    a[0, 1] = (np.nan, np.inf, -np.inf, np.nan)
    a[0, 2] = (np.nextafter(F(0.0031308), F(0)), np.nextafter(F(0.0031308), F(1)), -0.0, 0.5)
    return a


def assert_byte_rule(got, accum):
    """a byte may differ from the float64 evaluation by one only where srgb * 255 + 0.5 lies within the pow bound of an integer"""
    a = np.asarray(accum, F).astype(np.float64)
    with np.errstate(all="ignore"):
        x = a[..., :3]
        srgb = np.where(x <= np.float64(F(0.0031308)), x * np.float64(F(12.92)), np.float64(F(1.055)) * np.power(x, 1 / 2.4) - np.float64(F(0.055)))
        v = np.concatenate([np.clip(srgb, 0, 1), np.clip(a[..., 3:], 0, 1)], axis=-1) * 255 + 0.5
    want = np.where(np.isnan(v), 0, np.floor(np.nan_to_num(v, nan=0.0)))
    near = np.abs(v - np.round(v)) < 255 * 1.055 * 16 * 2.0 ** -23     # 4 ulp of pow and the float32 roundings behind it
    diff = np.abs(np.asarray(got).astype(int) - want.astype(int))
    bad = ~((diff == 0) | ((diff == 1) & near))
    assert not bad.any(), f"{int(bad.sum())} bytes break the rule; first at {np.argwhere(bad)[0].tolist()}: got {np.asarray(got)[tuple(np.argwhere(bad)[0])]}, expected {want[tuple(np.argwhere(bad)[0])]}"
