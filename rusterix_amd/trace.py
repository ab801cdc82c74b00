"""The path tracer on the device (include/rxr.h: rxr_set_trace_scene, rxr_trace; rusterix_amd/csrc/rxr_trace.hip): the reference's
Tracer::trace (src/tracer/trace.rs) over resident meshes and textures, from Python.

    with Tracer() as tr:
        tr.set_textures(static_tiles, dynamic_tiles)          # binding.Tile lists
        tr.set_meshes(meshes)                                 # mesh dicts, rxr_set_meshes order (see `mesh`)
        tr.set_scene(lights, sample_mode, animation_frame)    # RxrLight list (binding.Light.compile())
        acc = AccumBuffer(width, height)
        tr.trace(camera_firstp(...), acc, n_frames=16, seed=1)
        rgba = tr.to_u8(acc)

The host half of the three cameras' create_ray (src/camera/d3firstp.rs:112-138, d3orbit.rs:117-153, d3iso.rs:159-182) is here: what
they compute before they look at the pixel -- position, forward, right, up, half_width, half_height -- in float32, one operation per
line.  There is no CPU path: without a device the calls fail."""
import ctypes as C

import numpy as np

from .abi import (RXR_TRACE_CAMERA_FIRSTP as CAMERA_FIRSTP, RXR_TRACE_CAMERA_ISO as CAMERA_ISO, RXR_TRACE_CAMERA_ORBIT as CAMERA_ORBIT,
                  RXR_TRACE_NO_MATERIAL as NO_MATERIAL, rxr_mesh3d as _Mesh3D, rxr_texture as _Texture, rxr_tile as _Tile)
from .binding import RxrLight
from .libs import rxr_abi

F = np.float32
MAX_BOUNCES = 8
RAY_ACCEL_OFF, RAY_ACCEL_ON, RAY_ACCEL_COUNT = 0, 1, 2   # rxr_set_ray_accel's modes (include/rxr.h)
RAY_ACCEL_INFO = ("mode", "valid", "triangles", "nodes", "levels", "wild", "builds", "batches", "tests")   # rxr_ray_accel_info's words
RAY_WAVE_OFF, RAY_WAVE_ON, RAY_WAVE_FORCE = 0, 1, 2   # rxr_set_ray_wave's modes (include/rxr.h)
RAY_WAVE_INFO = ("mode", "batches", "rays")   # rxr_ray_wave_info's words
RAY_REFRESH_FULL, RAY_REFRESH_RANGED = 0, 1   # rxr_set_ray_refresh's modes (include/rxr.h)
RAY_REFRESH_INFO = ("mode", "pending", "refreshes", "refits", "triangles", "leaves", "nodes", "route")   # rxr_ray_refresh_info's words
RAY_REFRESH_VERIFY = ("pick_words", "sorted_words", "nodes", "wild", "checked")   # rxr_ray_refresh_verify's words
MATTE, GLOSSY, METALLIC, TRANSPARENT, EMISSIVE = range(5)                       # MaterialRole, src/shapestack/material.rs:8-14
MOD_NONE, MOD_LUMINANCE, MOD_SATURATION, MOD_INV_LUMINANCE, MOD_INV_SATURATION = range(5)   # MaterialModifier::from_u8, :66-76
SOURCE_OTHER, SOURCE_STATIC_TILE, SOURCE_DYNAMIC_TILE, SOURCE_PIXEL, SOURCE_TERRAIN = range(5)
LIST_CHUNK_OPACITY, LIST_CHUNK, LIST_CHUNK_TERRAIN, LIST_STATIC, LIST_DYNAMIC, LIST_OVERLAY = range(6)


class TraceError(RuntimeError):
    def __init__(self, code, msg=""):
        super().__init__(f"trace failed with status {code}: {msg}")
        self.code = code


# ---- vek in float32 ---------------------------------------------------------------------------------------------------------------
def _v3(v):
    return np.asarray(v, F).reshape(3)


def _dot(a, b):
    return F(F(a[0] * b[0]) + F(a[1] * b[1])) + F(a[2] * b[2])


def _cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], F)


def _normalized(a):
    with np.errstate(all="ignore"):
        return (a / np.sqrt(_dot(a, a))).astype(F)


def _to_radians(deg):
    return F(deg) * F(np.pi / 180.0)    # f32::to_radians: self * (PI / 180)


def _pack(position, forward, right, up, half_width, half_height):
    return np.concatenate([_v3(position), _v3(forward), _v3(right), _v3(up), [F(half_width), F(half_height)]]).astype(F)


def camera_firstp(position, center, fov, width, height):
    """(RXR_TRACE_CAMERA_FIRSTP, the 14 floats) of a D3FirstPCamera (d3firstp.rs:112-122; `up` is not normalised there)"""
    position, center = _v3(position), _v3(center)
    aspect = F(width) / F(height)
    half_height = np.tan(_to_radians(fov) * F(0.5)).astype(F)
    half_width = half_height * aspect
    forward = _normalized(center - position)
    right = _normalized(_cross(forward, np.array([0, 1, 0], F)))
    up = _cross(right, forward)
    return CAMERA_FIRSTP, _pack(position, forward, right, up, half_width, half_height)


def camera_orbit(center, distance, azimuth, elevation, fov, width, height, up=(0.0, 1.0, 0.0)):
    """... of a D3OrbitCamera (d3orbit.rs:117-139, eye_position :188-195)"""
    center, distance, azimuth, elevation = _v3(center), F(distance), F(azimuth), F(elevation)
    eye = np.array([distance * np.cos(azimuth) * np.cos(elevation), distance * np.sin(elevation),
                    distance * np.sin(azimuth) * np.cos(elevation)], F) + center
    aspect = F(width) / F(height)
    forward = _normalized(center - eye)
    right = _cross(forward, _v3(up))
    if _dot(right, right) < F(1e-12):
        right = np.array([1, 0, 0], F)
    right = _normalized(right)
    upv = _normalized(_cross(right, forward))
    half_height = np.tan(_to_radians(fov) * F(0.5)).astype(F)
    half_width = half_height * aspect
    return CAMERA_ORBIT, _pack(eye, forward, right, upv, half_width, half_height)


def camera_iso(center, azimuth_deg, elevation_deg, distance, scale, width, height):
    """... of a D3IsoCamera (d3iso.rs:38-67, :159-181): position = its position(), forward = (center - position).normalized(), right
    and up = basis()'s, half_height = scale, half_width = scale * max(width / height, 1e-6)"""
    center = _v3(center)
    yaw, pitch = _to_radians(azimuth_deg), _to_radians(elevation_deg)
    cp, sp, cy, sy = np.cos(pitch), np.sin(pitch), np.cos(yaw), np.sin(yaw)
    fwd = _normalized(np.array([cy * cp, sp, sy * cp], F))
    right = _cross(fwd, np.array([0, 1, 0], F))
    if _dot(right, right) < F(1e-6):
        right = np.array([1, 0, 0], F)
    right = _normalized(right)
    up = _normalized(_cross(right, fwd))
    position = center + fwd * F(distance)
    half_height = F(scale)
    half_width = half_height * max(F(width) / F(height), F(1e-6))
    return CAMERA_ISO, _pack(position, _normalized(center - position), right, up, half_width, half_height)


class AccumBuffer:
    """src/tracer/buffer.rs: linear RGBA f32 [height][width][4] and the number of frames averaged into it"""

    def __init__(self, width, height):
        self.width, self.height = int(width), int(height)
        self.pixels = np.zeros((self.height, self.width, 4), F)
        self.frame = 0

    def reset(self):
        self.frame = 0


def mesh(vertices, indices, uvs, normals, list=LIST_STATIC, chunk=-1, source=(SOURCE_OTHER, 0, (0, 0, 0, 0)), repeat_mode=0, material=None):
    """one entry of Tracer.set_meshes: object-space geometry, the Scene list it is in, its PixelSource as (kind, tile index, pixel) and
    its Material as (role, modifier, value) or None"""
    return dict(vertices=np.ascontiguousarray(vertices, F).reshape(-1, 4), indices=np.ascontiguousarray(indices, np.uint32).reshape(-1, 3),
                uvs=np.ascontiguousarray(uvs, F).reshape(-1, 2), normals=np.ascontiguousarray(normals, F).reshape(-1, 3), list=int(list),
                chunk=int(chunk), source=source, repeat_mode=int(repeat_mode), material=material)


def _tiles(tiles):
    arr, keep = (_Tile * max(len(tiles), 1))(), []
    for a, t in zip(arr, tiles):
        tex = (_Texture * max(len(t.textures), 1))()
        for x, src in zip(tex, t.textures):
            x.rgba, x.width, x.height = src.data.ctypes.data, src.width, src.height
        a.textures, a.n_textures = tex, len(t.textures)
        keep.append(tex)
    return arr, keep


class Tracer:
    """a device context of its own holding one scene for the path tracer"""

    def __init__(self, device=0):
        self.rxr = rxr_abi()
        self.ctx = C.c_void_p()
        rc = self.rxr.rxr_create(C.byref(self.ctx), device)
        if rc != 0:
            raise TraceError(rc, (self.rxr.rxr_last_error(None) or b"").decode())
        self.n_meshes = 0
        self.materials = []

    def error(self):
        return (self.rxr.rxr_last_error(self.ctx) or b"").decode()

    def _check(self, rc):
        if rc != 0:
            raise TraceError(rc, self.error())

    def set_textures(self, static_tiles=(), dynamic_tiles=()):
        s, keep_s = _tiles(list(static_tiles))
        d, keep_d = _tiles(list(dynamic_tiles))
        self._check(self.rxr.rxr_set_textures(self.ctx, C.cast(s, C.c_void_p), len(static_tiles), C.cast(d, C.c_void_p), len(dynamic_tiles)))
        del keep_s, keep_d

    def set_meshes(self, meshes):
        """`meshes`: what `mesh` returns, in rxr_set_meshes order (per chunk opacity, batches, terrain; then static, dynamic, overlay)"""
        arr = (_Mesh3D * max(len(meshes), 1))()
        identity = (C.c_float * 16)(*np.eye(4, dtype=F).ravel())
        for a, m in zip(arr, meshes):
            a.vertices, a.indices, a.uvs, a.normals = (m[k].ctypes.data for k in ("vertices", "indices", "uvs", "normals"))
            a.n_vertices, a.n_triangles = len(m["vertices"]), len(m["indices"])
            a.transform_3d = identity
            a.repeat_mode = m.get("repeat_mode", 0)
            kind, index, pixel = m.get("source", (SOURCE_OTHER, 0, (0, 0, 0, 0)))
            a.source.kind, a.source.index = kind, index
            a.source.pixel[:] = pixel
            a.shader = -1
            a.has_profile_id, a.profile_id = (1, m["pid"]) if m.get("has_pid") else (0, 0)
            a.list, a.chunk = m["list"], m.get("chunk", -1)
        self._check(self.rxr.rxr_set_meshes(self.ctx, C.cast(arr, C.c_void_p), len(meshes)))
        self.n_meshes = len(meshes)
        self.materials = [m.get("material") for m in meshes]

    def set_chunk_textures(self, chunks):
        """rxr_set_chunk_textures for the terrain-sourced meshes: chunks[c] is a dict with `terrain_texture` (a binding.Texture or
        None), `origin` (x, y) and `size`; set_scene takes the same list"""
        with_tex = [c for c in chunks if c.get("terrain_texture") is not None]
        tex = (_Texture * max(len(with_tex), 1))()
        for t, c in zip(tex, with_tex):
            src = c["terrain_texture"]
            t.rgba, t.width, t.height = src.data.ctypes.data, src.width, src.height
        slots, k = [], 0
        for c in chunks:
            slots.append(k if c.get("terrain_texture") is not None else -1)
            k += c.get("terrain_texture") is not None
        terrain = np.array(slots + [-1], np.int32)
        first = np.zeros(len(chunks) + 1, np.uint32)
        self._check(self.rxr.rxr_set_chunk_textures(self.ctx, C.cast(tex, C.c_void_p), len(with_tex), terrain.ctypes.data, first.ctypes.data, None, len(chunks)))

    def set_scene(self, lights=(), sample_mode=0, animation_frame=1, materials="meshes", chunks=()):
        """rxr_set_trace_scene: `lights` are RxrLight records (scene.lights, then scene.dynamic_lights); the materials are those the
        meshes were given unless `materials` lists (role, modifier, value) / None per mesh; `chunks`: origin and size per chunk"""
        mats = self.materials if materials == "meshes" else list(materials)
        kinds = np.zeros((max(len(mats), 1), 2), np.uint32)
        values = np.zeros(max(len(mats), 1), F)
        for i, m in enumerate(mats):
            kinds[i] = (NO_MATERIAL, 0) if m is None else (m[0], m[1])
            values[i] = 0.0 if m is None else m[2]
        arr = (RxrLight * max(len(lights), 1))(*lights)
        cos = np.array([(c["origin"][0], c["origin"][1], c["size"]) for c in chunks] + [(0, 0, 0)], np.int32)
        self._check(self.rxr.rxr_set_trace_scene(self.ctx, kinds.ctypes.data, values.ctypes.data, len(mats), C.cast(arr, C.c_void_p), len(lights),
                                                 int(sample_mode), int(animation_frame), cos.ctypes.data, len(chunks)))

    @property
    def ray_accel(self):
        """rxr_set_ray_accel's mode (0 off, the default; 1 on; 2 on and counting): trace() and intersect() with more than 64 rays
        cull their ray-triangle tests with a box tree built on the device; the results are the same words"""
        return self.ray_accel_info()["mode"]

    @ray_accel.setter
    def ray_accel(self, mode):
        self._check(self.rxr.rxr_set_ray_accel(self.ctx, int(mode)))

    def ray_accel_info(self):
        """rxr_ray_accel_info as a dict: mode, valid, triangles, nodes, levels, wild, builds, batches, tests"""
        out = (C.c_uint64 * len(RAY_ACCEL_INFO))()
        self._check(self.rxr.rxr_ray_accel_info(self.ctx, out))
        return dict(zip(RAY_ACCEL_INFO, (int(x) for x in out)))

    @property
    def ray_wave(self):
        """rxr_set_ray_wave's mode (0 off, the default; 1: the batches rxr_ray_wave_takes() names walk the tree a wave per ray;
        2: every batch does) -- only with ray_accel on; the results are the same words"""
        return self.ray_wave_info()["mode"]

    @ray_wave.setter
    def ray_wave(self, mode):
        self._check(self.rxr.rxr_set_ray_wave(self.ctx, int(mode)))

    def ray_wave_info(self):
        """rxr_ray_wave_info as a dict: mode, batches, rays"""
        out = (C.c_uint64 * len(RAY_WAVE_INFO))()
        self._check(self.rxr.rxr_ray_wave_info(self.ctx, out))
        return dict(zip(RAY_WAVE_INFO, (int(x) for x in out)))

    @property
    def ray_refresh(self):
        """rxr_set_ray_refresh's mode (0 full, the default: a mesh update invalidates the pick records and the tree; 1 ranged: the
        next query rewrites the updated meshes' records and refits the tree); the results are the same words"""
        return self.ray_refresh_info()["mode"]

    @ray_refresh.setter
    def ray_refresh(self, mode):
        self._check(self.rxr.rxr_set_ray_refresh(self.ctx, int(mode)))

    def ray_refresh_info(self):
        """rxr_ray_refresh_info as a dict: mode, pending, refreshes, refits, triangles, leaves, nodes, route"""
        out = (C.c_uint64 * len(RAY_REFRESH_INFO))()
        self._check(self.rxr.rxr_ray_refresh_info(self.ctx, out))
        return dict(zip(RAY_REFRESH_INFO, (int(x) for x in out)))

    def ray_refresh_verify(self):
        """rxr_ray_refresh_verify as a dict (blocking; tests and tools): pick_words, sorted_words, nodes, wild, checked"""
        out = (C.c_uint64 * len(RAY_REFRESH_VERIFY))()
        self._check(self.rxr.rxr_ray_refresh_verify(self.ctx, out))
        return dict(zip(RAY_REFRESH_VERIFY, (int(x) for x in out)))

    def ray_accel_invalidate(self):
        """rxr_ray_accel_invalidate: the next many-ray query with the tree on builds it from scratch"""
        self._check(self.rxr.rxr_ray_accel_invalidate(self.ctx))

    def intersect(self, origins, dirs, full=False):
        """rxr_intersect over the meshes of set_meshes: a dict of t, mesh, triangle, hitpoint and, with full=True, uv and normal"""
        o = np.ascontiguousarray(np.asarray(origins, F).reshape(-1, 3))
        d = np.ascontiguousarray(np.asarray(dirs, F).reshape(-1, 3))
        n = len(o)
        out = dict(t=np.zeros(n, F), mesh=np.zeros(n, np.uint32), triangle=np.zeros(n, np.uint32), hitpoint=np.zeros((n, 3), F))
        if full:
            out["uv"], out["normal"] = np.zeros((n, 2), F), np.zeros((n, 3), F)
        self._check(self.rxr.rxr_intersect(self.ctx, o.ctypes.data, d.ctypes.data, n, 1 if full else 0, out["t"].ctypes.data, out["mesh"].ctypes.data,
                                           out["triangle"].ctypes.data, out["hitpoint"].ctypes.data, out["uv"].ctypes.data if full else None,
                                           out["normal"].ctypes.data if full else None))
        return out

    def srgb_table(self):
        out = np.zeros(256, F)
        self._check(self.rxr.rxr_trace_srgb_table(self.ctx, out.ctypes.data))
        return out

    def trace(self, camera, accum, n_frames=1, seed=0, bounces=MAX_BOUNCES):
        """Tracer::trace n_frames times: `camera` is what camera_firstp / _orbit / _iso return; accum.frame advances"""
        kind, consts = camera
        consts = np.ascontiguousarray(consts, F)
        assert accum.pixels.flags.c_contiguous and accum.pixels.dtype == F and accum.pixels.shape == (accum.height, accum.width, 4)
        self._check(self.rxr.rxr_trace(self.ctx, kind, consts.ctypes.data, accum.width, accum.height, accum.frame, n_frames, seed, bounces,
                                       accum.pixels.ctypes.data))
        accum.frame += n_frames
        return accum

    def to_u8(self, accum):
        """AccumBuffer::to_u8_vec on the device: [height][width][4] bytes"""
        out = np.zeros((accum.height, accum.width, 4), np.uint8)
        self._check(self.rxr.rxr_accum_to_rgba(self.ctx, accum.pixels.ctypes.data, accum.width, accum.height, out.ctypes.data))
        return out

    def close(self):
        if self.ctx:
            self.rxr.rxr_destroy(self.ctx)
            self.ctx = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
