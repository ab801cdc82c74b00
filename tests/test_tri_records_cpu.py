"""The host side of the set-up records without a GPU: tests/tri_records_main.cpp compiles the shared definition (rxr_tri_records and
edges_from_xy, rusterix_amd/csrc/rxr_device.h) and the host's fetch (rxr_host_setup.h) with g++ -O2 -ffp-contract=off and runs them on
small frames full of special values; what it writes is compared with numpy float32 restatements of the reference's expressions
(Edges::new behind the winding swap, edge.rs:12-24 and batch3d.rs:706-746; 1 / z, 1 / w, uv / w and the clamped pixel box,
rasterizer.rs:989-1017, 1054-1072, 1754-1767).  The same program built with -fsanitize=address,undefined and run directly covers the
host's indexing: every section of the frame is a heap block of exactly its size."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "tri_records_main.cpp")
F = np.float32
NAN, INF = float("nan"), float("inf")
SPECIALS = [NAN, INF, -INF, 0.0, -0.0, 1e-40, 3.0e38, -3.0e38]
DB_HAS_NORMALS, DB_ALPHA_TEST, DB_SKIP, DB_OPACITY_LIST, DB_FULL_ALPHA, DB_TERRAIN = 1, 4, 8, 32, 128, 256
TS_DESC_VALID = 0x80000000
CULL_OFF, CULL_FRONT, CULL_BACK = 0, 1, 2
W, H = 171, 107


def compiled(tmp_path_factory, name, *flags):
    exe = str(tmp_path_factory.mktemp("tri_records") / name)
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", *flags, SRC, "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return compiled(tmp_path_factory, "tri_records")


@pytest.fixture(scope="module")
def program_sanitized(tmp_path_factory):
    return compiled(tmp_path_factory, "tri_records_san", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")


# ---- a frame -------------------------------------------------------------------------------------------------------------------------
def batch_word(vert_base, tri_base, n_tris, flags, tex, repeat_mode, profile_id, mode, n_verts):
    w = np.zeros(16, np.uint32)   # DevBatch (rxr_device.h)
    w[0], w[1], w[2], w[3], w[5], w[6], w[7], w[12], w[13] = vert_base, tri_base, n_tris, flags, 0xFF102030, repeat_mode, profile_id, mode, n_verts
    w[4] = np.int32(tex).astype(np.uint32) if tex < 0 else tex
    return w


TEXTURES = np.array([[100, 64, 64, 1], [5000, 8192, 2, 1], [9000, 8191, 3, 3], [0, 1, 1, 0]], np.uint32)   # offset, w, h, all_opaque
# flags, tex, repeat mode, profile id, cull mode
BATCHES = [(DB_HAS_NORMALS, 0, 1, 0, CULL_OFF), (0, -1, 0, 7, CULL_BACK), (DB_HAS_NORMALS | DB_ALPHA_TEST, 1, 2, 0, CULL_FRONT),
           (DB_HAS_NORMALS | DB_SKIP, 0, 0, 0, CULL_OFF), (DB_HAS_NORMALS, 2, 3, 9, CULL_OFF), (DB_HAS_NORMALS | DB_TERRAIN, 3, 0, 0, CULL_OFF),
           (DB_HAS_NORMALS, 3, 4, 0, CULL_BACK)]


def special_frame(seed):
    """per batch: every (field, special) triangle -- x, y, z, w of vertex 1, u, v of vertex 2 -- with shared and private vertices, then
    ordinary ones and one off screen (an empty pixel box in complete records); vertex w = 0 gives 1 / w = inf and uv / w = inf or NaN"""
    rng = np.random.default_rng([0x52585231, 808, seed])
    pv, uv, nrm, idx, tri_info, batches, cull_of = [], [], [], [], [], [], []
    vbase = tbase = 0
    for bi, (flags, tex, repeat, profile, cull) in enumerate(BATCHES):
        v_b, uv_b, idx_b = [], [], []
        cases = [(fld, s) for fld in range(6) for s in SPECIALS][bi::len(BATCHES)] + [(None, None)] * 3 + [(None, "off screen")]
        for fld, s in cases:
            c = rng.uniform([10, 10], [W - 10, H - 10]) - (400 if s == "off screen" else 0)
            v = np.concatenate([c + rng.normal(0, 25, (3, 2)), rng.uniform(0.1, 0.9, (3, 1)), rng.uniform(0.5, 4.0, (3, 1)) * rng.choice([1, 1, 1, -1], (3, 1))], axis=1).astype(F)
            t_uv = rng.uniform(-0.5, 2.0, (3, 2)).astype(F)
            if fld is not None and fld < 4:
                v[1, fld] = s
            elif fld is not None:
                t_uv[2, fld - 4] = s
            first = len(v_b)
            v_b += list(v)
            uv_b += list(t_uv)
            idx_b.append([first + 2, first, first + 1] if rng.random() < 0.3 else [first, first + 1, first + 2])
        n_v, n_t = len(v_b), len(idx_b)
        batches.append(batch_word(vbase, tbase, n_t, flags, tex, repeat, profile, cull, n_v))
        pv += v_b
        uv += uv_b
        nrm += list(rng.normal(0, 1, (n_v, 3)).astype(F))
        idx += idx_b
        tri_info += [[bi, vbase]] * n_t
        cull_of += [cull] * n_t
        vbase += n_v
        tbase += n_t
    clip = np.array([[0, W, 0, H] if b % 2 else sorted(rng.integers(0, W, 2)) + sorted(rng.integers(0, H, 2)) for b in range(len(BATCHES))], np.uint32)
    return dict(pv=np.array(pv, F), uv=np.array(uv, F), nrm=np.array(nrm, F), idx=np.array(idx, np.uint32), tri_info=np.array(tri_info, np.uint32),
                batches=np.array(batches, np.uint32), cull=cull_of, evis=(rng.random(len(idx)) < 0.85).astype(np.uint32), clip=clip)


# ---- the reference's expressions in numpy float32 --------------------------------------------------------------------------------------
def edges_new(cull, evis, p):
    (x0, y0), (x1, y1), (x2, y2) = p
    front = ((x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0)) > 0     # is_front_facing, batch3d.rs:742-746
    swap, visible = {CULL_OFF: (front, True), CULL_FRONT: (False, not front), CULL_BACK: (front, front)}[cull]
    if swap:
        x1, y1, x2, y2 = x2, y2, x1, y1
    px, py, qx, qy = [x0, x1, x2], [y0, y1, y2], [x1, x2, x0], [y1, y2, y0]
    a = [qy[i] - py[i] for i in range(3)]
    b = [px[i] - qx[i] for i in range(3)]
    c = [qx[i] * py[i] - qy[i] * px[i] for i in range(3)]
    return a, b, c, bool(evis) and bool(visible)


def as_index(x):   # `x as usize` (saturating, NaN -> 0), then the 16-bit field
    if not x > 0:
        return 0
    return 0xFFFF if x >= 65535.0 else int(x)


def bits(x):
    return int(np.array(x, F).view(np.uint32))


def expected(fr, t, edges, sample_mode, has_clip):
    """(live, 24 words, 20 words) of triangle t; `edges`: (a, b, c, visible)"""
    bi, vbase = (int(x) for x in fr["tri_info"][t])
    B = fr["batches"][bi]
    flags, tex, repeat, profile = int(B[3]), int(B[4].astype(np.int32)), int(B[6]), int(B[7])
    a, b, c, visible = edges
    if not visible or flags & DB_SKIP:
        return 0, [0] * 24, [0] * 20
    i = [int(k) + vbase for k in fr["idx"][t]]
    v, uv = fr["pv"][i], fr["uv"][i]
    n = fr["nrm"][i] if flags & DB_HAS_NORMALS else np.zeros((3, 3), F)
    one = F(1.0)
    area = (v[2, 0] - v[0, 0]) * (v[1, 1] - v[0, 1]) - (v[2, 1] - v[0, 1]) * (v[1, 0] - v[0, 0])
    iz = [one / v[k, 2] for k in range(3)]
    iw = [one / v[k, 3] for k in range(3)]
    uw = [uv[k, 0] / v[k, 3] for k in range(3)]
    vw = [uv[k, 1] / v[k, 3] for k in range(3)]
    bflags = flags
    if sample_mode != 0 and tex >= 0 and not flags & (DB_ALPHA_TEST | DB_FULL_ALPHA | DB_OPACITY_LIST):
        risky = any(not abs(x) < INF for x in iw + uw + vw)
        lo, hi = np.fmin(abs(iw[0]), np.fmin(abs(iw[1]), abs(iw[2]))), np.fmax(abs(iw[0]), np.fmax(abs(iw[1]), abs(iw[2])))
        same_sign = all(x > 0 for x in iw) or all(x < 0 for x in iw)
        if risky or not same_sign or not hi <= lo * F(1048576.0):
            bflags |= DB_ALPHA_TEST
    pad = [0, 0]
    if tex >= 0 and not flags & DB_TERRAIN and repeat < 4:
        off, tw, th, opaque = (int(x) for x in TEXTURES[tex])
        if 1 <= tw <= 8191 and 1 <= th <= 8191:
            pad = [off, TS_DESC_VALID | tw | th << 13 | repeat << 26 | (opaque & 3) << 28]
    xs, ys = v[:, 0], v[:, 1]
    min_x = as_index(np.fmax(np.floor(np.fmin(xs[0], np.fmin(xs[1], xs[2]))), F(0)))
    max_x = as_index(np.fmin(np.ceil(np.fmax(xs[0], np.fmax(xs[1], xs[2]))), F(W)))
    min_y = as_index(np.fmax(np.floor(np.fmin(ys[0], np.fmin(ys[1], ys[2]))), F(0)))
    max_y = as_index(np.fmin(np.ceil(np.fmax(ys[0], np.fmax(ys[1], ys[2]))), F(H)))
    if has_clip:
        x0, x1, y0, y1 = (int(k) for k in fr["clip"][bi])
        min_x, max_x, min_y, max_y = max(min_x, x0), min(max_x, x1), max(min_y, y0), min(max_y, y1)
    live = min_x < max_x and min_y < max_y
    S = [bits(x) for x in a + b + c] + [bits(x) for x in (v[0, 0], v[0, 1], v[1, 0], v[1, 1], v[2, 0], v[2, 1], area, *iz)]
    S += [bi, (min_x | max_x << 16) if live else 0, (min_y | max_y << 16) if live else 0, bflags, profile]
    Hh = [bits(x) for x in iw + uw + vw] + [bits(x) for x in n.reshape(-1)] + pad
    return int(live), S, Hh


def run(exe, fr, tmp_path, edgeless, has_clip, sample_mode):
    with np.errstate(all="ignore"):
        edges = [edges_new(fr["cull"][t], fr["evis"][t], fr["pv"][[int(k) + int(fr["tri_info"][t][1]) for k in fr["idx"][t]], :2]) for t in range(len(fr["idx"]))]
    if edgeless:
        edge_section = fr["evis"]
    else:
        edge_section = np.array([[bits(x) for x in a + b + c] + [int(vis)] for a, b, c, vis in edges], np.uint32)
    head = np.array([len(fr["pv"]), len(fr["idx"]), len(fr["batches"]), len(TEXTURES), int(edgeless), int(has_clip), sample_mode, W, H], np.uint32)
    sections = [head, fr["pv"], fr["uv"], fr["nrm"], fr["idx"], edge_section, fr["tri_info"], fr["batches"], TEXTURES] + ([fr["clip"]] if has_clip else [])
    src, out = tmp_path / "frame.bin", tmp_path / "records.bin"
    src.write_bytes(b"".join(np.ascontiguousarray(s).tobytes() for s in sections))
    pr = subprocess.run([exe, str(src), str(out)], capture_output=True, text=True)
    assert pr.returncode == 0, pr.stderr[-3000:]
    got = np.frombuffer(out.read_bytes(), np.uint32).reshape(len(fr["idx"]), 45)
    return edges, got


def same_word(a, b):
    """equal bit patterns; two NaNs are equal whatever their payload (numpy and the compiled code may pick different instructions)"""
    if a == b:
        return True
    fa, fb = np.array([a, b], np.uint32).view(F)
    return bool(np.isnan(fa) and np.isnan(fb))


@pytest.mark.parametrize("sample_mode", [0, 1])
@pytest.mark.parametrize("has_clip", [False, True])
@pytest.mark.parametrize("edgeless", [False, True])
def test_records_equal_the_reference_s_expressions(program, tmp_path, edgeless, has_clip, sample_mode):
    fr = special_frame(1)
    edges, got = run(program, fr, tmp_path, edgeless, has_clip, sample_mode)
    seen = dict(live=0, empty=0, hidden=0, rule=0, desc=0)
    with np.errstate(all="ignore"):
        for t in range(len(fr["idx"])):
            live, S, Hh = expected(fr, t, edges[t], sample_mode, has_clip)
            want = [live] + S + Hh
            bad = [k for k in range(45) if not same_word(int(got[t, k]), want[k])]
            # (float fields only: 1..19 of TriSetup, 25..42 of TriShade; the others must be equal as integers, which same_word asks too)
            assert not bad, f"triangle {t} (batch {fr['tri_info'][t][0]}): words {bad}: got {[hex(int(got[t, k])) for k in bad]} want {[hex(want[k]) for k in bad]}"
            seen["live"] += live
            seen["hidden"] += int(not edges[t][3])
            seen["empty"] += int(edges[t][3] and not live and any(S))
            seen["rule"] += int(any(S) and S[22] != int(fr["batches"][fr["tri_info"][t][0]][3]))
            seen["desc"] += int(Hh[19] != 0)
    assert seen["live"] > 20 and seen["empty"] > 0 and seen["hidden"] > 3 and seen["desc"] > 5, seen
    assert (seen["rule"] > 0) == (sample_mode == 1), seen


def test_the_host_s_indexing_under_the_sanitizers(program, program_sanitized, tmp_path):
    """the same frames through the build with AddressSanitizer and UndefinedBehaviorSanitizer: no report, and the same bytes"""
    for seed, edgeless, has_clip in ((1, True, True), (2, False, False), (3, True, False)):
        fr = special_frame(seed)
        _, plain = run(program, fr, tmp_path, edgeless, has_clip, 1)
        _, checked = run(program_sanitized, fr, tmp_path, edgeless, has_clip, 1)
        assert np.array_equal(plain, checked)
