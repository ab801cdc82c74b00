"""numpy float32 restatement of Tracer::trace (reference src/tracer/trace.rs:105-475) and AccumBuffer (src/tracer/buffer.rs) as
include/rxr.h states them for rxr_trace: the ground truth of tests/test_trace_cpu.py and tests/test_gpu_trace.py.

Composed of pieces already trusted: tests/intersect_ref.py for the hits (Batch3D::intersect(ray, false) folded by `hit.t < best.t`), the
oracle's texture_sample / pixel_to_vec4 / light_radiance_at / hash_u32 (tests/oracle_api.py) for texels and lights, and its own
counter-based generator.  Everything else is one IEEE float32 operation per numpy operation in the reference's order, all live paths of
a bounce at once.  The sRGB table and the camera's 14 host-computed floats are arguments (include/rxr.h: what crosses the boundary);
`trig(phi) -> (cos, sin)` replaces sample_cosine's two libm calls (default: float64 results rounded to float32).

A scene is a dict: meshes (rusterix_amd.trace.mesh dicts, rxr_set_meshes order), static_tiles / dynamic_tiles (binding.Tile lists),
lights (RxrLight list), sample_mode, animation_frame and, for terrain-sourced meshes, chunks (dicts: terrain_texture, origin, size)."""
import numpy as np

from tests import intersect_ref as R

F = np.float32
U = np.uint64
M32 = U(0xFFFFFFFF)
PI = F(np.pi)
INV_255 = F(1.0) / F(255.0)
CAMERA_FIRSTP, CAMERA_ORBIT, CAMERA_ISO = 0, 1, 2
NO_MATERIAL = 0xFFFFFFFF
MATTE, GLOSSY, METALLIC, TRANSPARENT, EMISSIVE = range(5)
SOURCE_OTHER, SOURCE_STATIC_TILE, SOURCE_DYNAMIC_TILE, SOURCE_PIXEL, SOURCE_TERRAIN = range(5)
TRACED_LISTS = (R.LIST_CHUNK, R.LIST_CHUNK_TERRAIN, R.LIST_STATIC, R.LIST_DYNAMIC)


# ---- the generator of include/rxr.h -----------------------------------------------------------------------------------------------
def pcg(v):
    """u32 -> u32, on uint64 arrays holding 32-bit values"""
    v = np.asarray(v, U)
    s = (v * U(747796405) + U(2891336453)) & M32
    w = (((s >> ((s >> U(28)) + U(4))) ^ s) * U(277803737)) & M32
    return ((w >> U(22)) ^ w) & M32


def rand_u32(seed, frame, pixel, slot):
    h = pcg(U((int(seed) + int(frame)) & 0xFFFFFFFF))
    h = pcg((h + np.asarray(pixel, U)) & M32)
    return pcg((h + np.asarray(slot, U)) & M32)


def rand_f32(seed, frame, pixel, slot):
    """rand's f32: (u32 >> 8) as f32 * 2^-24"""
    return (rand_u32(seed, frame, pixel, slot) >> U(8)).astype(F) * F(2.0 ** -24)


# ---- srgb ---------------------------------------------------------------------------------------------------------------------------
def srgb_table():
    """trace.rs:14-20 over pixel_to_vec4's 256 values with numpy's float32 pow (the device's table need only be within 1 ulp of it)"""
    c = np.arange(256, dtype=F) * INV_255
    with np.errstate(all="ignore"):
        return np.where(c <= F(0.04045), c / F(12.92), np.power((c + F(0.055)) / F(1.055), F(2.4))).astype(F)


def trig64(phi):
    return np.cos(phi.astype(np.float64)).astype(F), np.sin(phi.astype(np.float64)).astype(F)


def trig_shifted(cos_ulps, sin_ulps):
    """cos and sin moved by that many float32 ulps of the correctly rounded value before rounding (the libm bound's edge)"""
    def f(phi):
        c, s = np.cos(phi.astype(np.float64)), np.sin(phi.astype(np.float64))
        return ((c + cos_ulps * np.spacing(np.abs(c).astype(F)).astype(np.float64)).astype(F),
                (s + sin_ulps * np.spacing(np.abs(s).astype(F)).astype(np.float64)).astype(F))
    return f


def scale(a, s):
    return a * np.asarray(s, F)[..., None]


def rclamp(x, lo, hi):
    """f32::clamp: a NaN stays"""
    return np.where(x < lo, lo, np.where(x > hi, hi, x)).astype(F)


# ---- the cameras' create_ray behind their 14 host-computed floats --------------------------------------------------------------------
def camera_rays(kind, consts, width, height, jx, jy):
    consts = np.asarray(consts, F)
    pos, fwd, right, up, half_w, half_h = consts[0:3], consts[3:6], consts[6:9], consts[9:12], consts[12], consts[13]
    n = width * height
    i = np.arange(n)
    sx, sy = F(width), F(height)
    uvx = (i % width).astype(F) / sx
    uvy = F(1.0) - (i // width).astype(F) / sy
    if kind == CAMERA_FIRSTP:
        psx, psy = F(1.0) / sx, F(1.0) / sy
        lower_left = ((pos + fwd) - right * half_w) - up * half_h
        horizontal, vertical = right * (F(2.0) * half_w), up * (F(2.0) * half_h)
        sample_pos = (lower_left[None, :] + scale(horizontal[None, :], psx * jx + uvx)) + scale(vertical[None, :], psy * jy + uvy)
        return np.repeat(pos[None, :], n, axis=0), R.normalized(sample_pos - pos[None, :])
    if kind == CAMERA_ORBIT:
        psx, psy = F(1.0) / sx, F(1.0) / sy
        uvy = F(1.0) - uvy
        nx, ny = (psx * jx + uvx) * F(2.0) - F(1.0), (psy * jy + uvy) * F(2.0) - F(1.0)
        d = (fwd[None, :] + scale(right[None, :], nx) * half_w) - scale(up[None, :], ny) * half_h
        return np.repeat(pos[None, :], n, axis=0), R.normalized(d)
    horizontal, vertical = (-right) * (F(2.0) * half_w), up * (F(2.0) * half_h)
    psx, psy = F(1.0) / max(sx, F(1.0)), F(1.0) / max(sy, F(1.0))
    o = (pos[None, :] + scale(horizontal[None, :], (psx * jx + uvx) - F(0.5))) + scale(vertical[None, :], (psy * jy + uvy) - F(0.5))
    return o.astype(F), np.repeat(fwd[None, :], n, axis=0)


# ---- evaluate_hit -------------------------------------------------------------------------------------------------------------------
def texel_of(orc, scene, m, uv, world):
    """the texel's bytes of a hit on mesh dict `m` (trace.rs:386-437)"""
    kind, index, pixel = m.get("source", (SOURCE_OTHER, 0, (0, 0, 0, 0)))
    if kind == SOURCE_PIXEL:
        return np.array(pixel, np.uint8)
    if kind in (SOURCE_STATIC_TILE, SOURCE_DYNAMIC_TILE):
        tile = (scene["static_tiles"] if kind == SOURCE_STATIC_TILE else scene["dynamic_tiles"])[index]
        tex = tile.textures[scene["animation_frame"] % len(tile.textures)]
        return orc.texture_sample(tex, float(uv[0]), float(uv[1]), scene["sample_mode"], m.get("repeat_mode", 0))
    if kind == SOURCE_TERRAIN and m.get("chunk", -1) >= 0:
        # chunk.sample_terrain_texture(Vec2::new(w.x, w.z), Vec2::one()) (src/chunk.rs:135-151) with Texture::get_pixel
        chunk = scene["chunks"][m["chunk"]]
        tex = chunk.get("terrain_texture")
        if tex is None:
            return np.zeros(4, np.uint8)
        local_x = (world[0] / F(1.0)) - F(chunk["origin"][0])
        local_y = (world[2] / F(1.0)) - F(chunk["origin"][1])
        pixels_per_tile = int(tex.width / chunk["size"])     # i32 division (positive operands)
        pixel_x, pixel_y = local_x * F(pixels_per_tile), local_y * F(pixels_per_tile)
        px = int(rclamp(np.floor(pixel_x), F(0.0), F(tex.width) - F(1.0)))
        py = int(rclamp(np.floor(pixel_y), F(0.0), F(tex.height) - F(1.0)))
        return tex.data.reshape(tex.height, tex.width, 4)[py, px]
    return np.zeros(4, np.uint8)


def modify(modifier, c, strength):
    """MaterialModifier::modify (material.rs:80-110) for one texel"""
    if modifier in (1, 3):
        lum = (F(0.2126) * c[0] + F(0.7152) * c[1]) + F(0.0722) * c[2]
        return lum * strength if modifier == 1 else (F(1.0) - lum) * strength
    if modifier in (2, 4):
        mx, mn = max(c[0], max(c[1], c[2])), min(c[0], min(c[1], c[2]))
        sat = (mx - mn) / mx if mx > 0 else F(0.0)
        return sat * strength if modifier == 2 else (F(1.0) - sat) * strength
    return strength


def sample_cosine(n, r1, r2, trig):
    phi = (F(2.0) * PI) * r1
    r = np.sqrt(r2)
    c, s = trig(phi)
    lx, ly, lz = c * r, s * r, np.sqrt(F(1.0) - r2)
    w = n
    a = np.where((np.abs(w[:, 0]) > F(0.1))[:, None], np.array([0, 1, 0], F)[None, :], np.array([1, 0, 0], F)[None, :]).astype(F)
    v = R.normalized(R.cross(w, a))
    u = R.cross(v, w)
    return R.normalized((scale(u, lx) + scale(v, ly)) + scale(w, lz))


def trace(orc, scene, camera, width, height, first_frame, n_frames, seed, bounces, accum, table, trig=trig64, signatures=False):
    """rxr_trace: averages n_frames samples into `accum` [height][width][4] (a new array is returned).  signatures: also a list per
    frame of per-pixel tuples, one (mesh, triangle, branch) per bounce -- branch 'E' emissive, 'S' specular, 'D' diffuse, with a
    trailing 'r' where the roulette ended the path, and ('miss',) for a miss."""
    kind, consts = camera
    n = width * height
    meshes = scene["meshes"]
    traced = [i for i, m in enumerate(meshes) if m["list"] in TRACED_LISTS]
    plain = [dict(meshes[i], list=R.LIST_STATIC, has_pid=False) for i in traced]   # the fold is a plain `<`: profile ids play no part
    hash_anim = orc.hash_u32(scene["animation_frame"] & 0xFFFFFFFF)
    table = np.asarray(table, F)
    acc = np.array(accum, F).reshape(n, 4)
    pix = np.arange(n, dtype=U)
    sigs = []
    with np.errstate(all="ignore"):
        for k in range(n_frames):
            frame = first_frame + k
            sig = [[] for _ in range(n)]
            o, d = camera_rays(kind, consts, width, height, rand_f32(seed, frame, pix, 0), rand_f32(seed, frame, pix, 1))
            thr, ret, live = np.ones((n, 3), F), np.zeros((n, 3), F), np.ones(n, bool)
            for b in range(bounces):
                idx = np.nonzero(live)[0]
                if len(idx) == 0:
                    break
                hit = R.intersect_many(plain, o[idx], d[idx], full=True) if plain else dict(mesh=np.full(len(idx), R.MISS, np.uint32))
                missed = hit["mesh"] == R.MISS
                for j in idx[missed]:
                    sig[j].append(("miss",))
                live[idx[missed]] = False     # a miss adds nothing and ends the path
                sel = np.nonzero(~missed)[0]
                if len(sel) == 0:
                    continue
                rays = idx[sel]
                t, nrm, uv = hit["t"][sel], hit["normal"][sel], hit["uv"][sel]
                mesh_i = np.array([traced[int(x)] for x in hit["mesh"][sel]])
                tri_i = hit["triangle"][sel]
                oo, dd = o[rays], d[rays]
                world = oo + scale(dd, t)
                # evaluate_hit, a hit at a time
                tex_lin, spec_w, emissive = np.zeros((len(rays), 3), F), np.zeros(len(rays), F), np.zeros((len(rays), 3), F)
                for q in range(len(rays)):
                    m = meshes[mesh_i[q]]
                    px = texel_of(orc, scene, m, uv[q], world[q])
                    texel = orc.pixel_to_vec4(px)
                    tex_lin[q] = table[px[:3]]
                    mat = m.get("material")
                    if mat is not None:
                        role, modifier, value = mat[0], mat[1], F(mat[2])
                        val = F(modify(modifier, texel, value))
                        if role == MATTE:
                            spec_w[q] = F(1.0) - val
                        elif role in (GLOSSY, METALLIC):
                            spec_w[q] = val
                        elif role == EMISSIVE:
                            emissive[q] = (tex_lin[q] * value) * F(10.0)
                albedo = tex_lin
                em = np.any(emissive != 0, axis=1)
                ret[rays[em]] = ret[rays[em]] + emissive[em] * thr[rays[em]]
                live[rays[em]] = False
                for q in np.nonzero(em)[0]:
                    sig[rays[q]].append((int(mesh_i[q]), int(tri_i[q]), "E"))
                # direct lighting
                direct = np.zeros((len(rays), 3), F)
                for q in np.nonzero(~em)[0]:
                    for light in scene["lights"]:
                        lc = orc.light_radiance_at(light, world[q], nrm[q], hash_anim)
                        if lc is not None:
                            direct[q] = direct[q] + lc * F(10.0)
                go = ~em
                rg = rays[go]
                brdf = albedo[go] / PI
                ret[rg] = ret[rg] + direct[go] * (thr[rg] * brdf)
                # the new direction
                slot = 2 + 4 * b
                r_spec, r1 = rand_f32(seed, frame, pix[rg], slot), rand_f32(seed, frame, pix[rg], slot + 1)
                r2, r_rr = rand_f32(seed, frame, pix[rg], slot + 2), rand_f32(seed, frame, pix[rg], slot + 3)
                sw = spec_w[go]
                p_spec = rclamp(sw, F(0.0), F(1.0))
                p_diff = F(1.0) - p_spec
                choose = r_spec < p_spec
                pdf = np.where(choose, p_spec, p_diff).astype(F)
                n_g, d_g, o_g, t_g = nrm[go], dd[go], oo[go], t[go]
                reflected = d_g - scale(n_g, F(2.0) * R.dot(d_g, n_g))
                cosine = sample_cosine(n_g, r1, r2, trig)
                ndir = np.where(choose[:, None], reflected, cosine).astype(F)
                thr_spec = scale(thr[rg], sw / pdf)
                thr_diff = thr[rg] * (scale(albedo[go], p_diff) / (pdf * PI)[:, None])
                nthr = np.where(choose[:, None], thr_spec, thr_diff).astype(F)
                norigin = (o_g + scale(ndir, t_g)) + n_g * F(0.01)      # ray.at(t) along the NEW direction (trace.rs:301-309)
                p = rclamp(np.fmax(nthr[:, 0], np.fmax(nthr[:, 1], nthr[:, 2])), F(0.001), F(1.0))
                dead = r_rr > p
                nthr = scale(nthr, F(1.0) / p)
                keep = ~dead
                o[rg[keep]], d[rg[keep]], thr[rg[keep]] = norigin[keep], ndir[keep], nthr[keep]
                live[rg[dead]] = False
                gi = np.nonzero(go)[0]
                for q in range(len(rg)):
                    sig[rg[q]].append((int(mesh_i[gi[q]]), int(tri_i[gi[q]]), ("S" if choose[q] else "D") + ("r" if dead[q] else "")))
            tt = F(1.0) / (F(frame) + F(1.0))
            new = np.concatenate([ret, np.ones((n, 1), F)], axis=1)
            acc = (acc * (F(1.0) - tt) + new * tt).astype(F)
            sigs.append([tuple(s) for s in sig])
    out = acc.reshape(height, width, 4)
    return (out, sigs) if signatures else out


# ---- AccumBuffer::to_u8_vec (buffer.rs:68-91) ---------------------------------------------------------------------------------------
def srgb_before_cast(accum):
    """srgb.clamp(0, 1) * 255 + 0.5 per colour channel (float32 pow), and the alpha channel's value before its cast"""
    a = np.asarray(accum, F)
    with np.errstate(all="ignore"):
        x = a[..., :3]
        srgb = np.where(x <= F(0.0031308), x * F(12.92), F(1.055) * np.power(x, F(1.0) / F(2.4)) - F(0.055)).astype(F)
        rgb = rclamp(srgb, F(0.0), F(1.0)) * F(255.0) + F(0.5)
        alpha = rclamp(a[..., 3:], F(0.0), F(1.0)) * F(255.0) + F(0.5)
    return np.concatenate([rgb, alpha], axis=-1).astype(F)


def to_u8(accum):
    v = srgb_before_cast(accum)
    return np.where(np.isnan(v), 0, np.clip(v, 0, 255)).astype(np.uint8)   # `as u8`: saturating, truncating, NaN -> 0
