"""Ground truth for the device's vertex normals (rxr_vertex_normals, include/rxr.h): the oracle's Batch3D::compute_vertex_normals
(oracle/rusterix_oracle.cpp, src/batch/batch3d.rs:771-809) over exactly the arrays given, and a numpy-float32 transcription of the
same loop that can also run the triangles in REVERSED order -- float addition is not associative, so the reversed sums differ in
their last bits, which is what makes the order tests mean something.  Nothing here uses the code under test.

A mesh is (vertices [nv][4] f32, indices [nt][3] u32)."""
import numpy as np

F = np.float32
SENTINEL = F(-7.25)          # what the tests fill the normals with before a call: no normal has this component


def oracle_normals(oracle, vertices, indices):
    """[nv][3]: oracle.Batch3D.new(v, i, uv).with_computed_normals().geometry()[3]"""
    v = np.ascontiguousarray(vertices, F).reshape(-1, 4)
    i = np.ascontiguousarray(indices, np.uint32).reshape(-1, 3)
    if not len(v):
        return np.zeros((0, 3), F)
    n = oracle.Batch3D.new(v, i, np.zeros((len(v), 2), F)).with_computed_normals().geometry()[3]
    assert n.shape == (len(v), 3)
    return n


def _normalized(x, y, z):
    """vek's normalized on arrays: the dot product left to right, a square root, three divisions -- each one f32 operation"""
    with np.errstate(all="ignore"):
        m = np.sqrt((x * x + y * y) + z * z)
        return x / m, y / m, z / m


def face_normals(vertices, indices):
    """[nt][3]: normalized(cross(p1 - p0, p2 - p0)) per triangle, vek's cross"""
    v = np.asarray(vertices, F).reshape(-1, 4)
    i = np.asarray(indices, np.uint32).reshape(-1, 3)
    p0, p1, p2 = v[i[:, 0], :3], v[i[:, 1], :3], v[i[:, 2], :3]
    with np.errstate(all="ignore"):
        a, b = p1 - p0, p2 - p0
        cx = a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1]
        cy = a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2]
        cz = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
    return np.stack(_normalized(cx, cy, cz), axis=1).astype(F)


def transcribed_normals(vertices, indices, reverse=False):
    """the reference's loop in numpy float32; reverse=True walks the triangles from the last to the first"""
    v = np.asarray(vertices, F).reshape(-1, 4)
    i = np.asarray(indices, np.uint32).reshape(-1, 3)
    fn = face_normals(v, i)
    total = np.zeros((len(v), 3), F)          # Vec3::zero(): +0.0
    counts = np.zeros(len(v), np.uint32)
    order = range(len(i) - 1, -1, -1) if reverse else range(len(i))
    with np.errstate(all="ignore"):
        for t in order:
            for k in i[t]:
                total[k] = total[k] + fn[t]
                counts[k] += 1
        used = counts > 0
        mean = total[used] / counts[used].astype(F)[:, None]
        total[used] = np.stack(_normalized(mean[:, 0], mean[:, 1], mean[:, 2]), axis=1)
    return total


def same_bits(got, want):
    """uint32 views equal, a NaN of `want` answered by any NaN"""
    got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    if got.shape != want.shape:
        return False
    nan = np.isnan(want)
    return bool((np.isnan(got) == nan).all() and (got.view(np.uint32)[~nan] == want.view(np.uint32)[~nan]).all())


def differing_vertices(a, b):
    """how many vertices differ in at least one bit (NaN against NaN counts as equal)"""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    both_nan = np.isnan(a) & np.isnan(b)
    return int(((a.view(np.uint32) != b.view(np.uint32)) & ~both_nan).any(axis=1).sum())


# ---- meshes ----------------------------------------------------------------------------------------------------------------------------
def generated(seed, nv=40, nt=120, degenerate=0):
    """seeded: coordinates uniform in +-4, triangles over three DISTINCT vertices -- except the first `degenerate` ones, which are (a, a, b)"""
    rng = np.random.default_rng(seed)
    v = np.ones((nv, 4), F)
    v[:, :3] = (rng.random((nv, 3), dtype=F) * F(8.0) - F(4.0))
    i = np.zeros((nt, 3), np.uint32)
    for t in range(nt):
        i[t] = rng.choice(nv, 3, replace=False)
    for t in range(min(degenerate, nt)):
        i[t, 1] = i[t, 0]
    return v, i


def negative_zero_triangle():
    """axis-aligned, its vertices used by no other triangle: cross((1,0,0), (0,0,-1)) = (0*-1 - 0*0, 0*0 - 1*-1, 1*0 - 0*0) =
    (-0.0, 1, +0.0), so the face normal's x is -0.0 -- and the vertex normal's x must be the +0.0 of +0.0 + -0.0"""
    return np.array([[0, 0, 0, 1], [1, 0, 0, 1], [0, 0, -1, 1]], F), np.array([[0, 1, 2]], np.uint32)


def fan(valence, seed=0):
    """an apex (vertex 0) named by `valence` triangles (0, j, j + 1) over a ragged rim"""
    rng = np.random.default_rng(1000 + seed + valence)
    v = np.ones((valence + 2, 4), F)
    ang = np.linspace(0.0, 5.5, valence + 1)
    v[1:, 0] = (np.cos(ang) * (1.0 + rng.random(valence + 1))).astype(F)
    v[1:, 2] = (np.sin(ang) * (1.0 + rng.random(valence + 1))).astype(F)
    v[1:, 1] = rng.random(valence + 1, dtype=F) - F(0.5)
    v[0, :3] = (0.03, 0.7, -0.02)
    i = np.array([(0, j, j + 1) for j in range(1, valence + 1)], np.uint32)
    return v, i


def pack(meshes, vstride=None, tstride=None):
    """the strided arrays of a call: counts [n][2], vertices [n][VS][4], indices [n][TS][3], normals [n][VS][3] filled with SENTINEL.
    Slots past a mesh's counts hold what must never be read as geometry: 1e30 vertices; their indices are 0 (in range whatever reads them)."""
    n = len(meshes)
    nv = [len(m[0]) for m in meshes]
    nt = [len(m[1]) for m in meshes]
    vs = max(nv + [0]) if vstride is None else vstride
    ts = max(nt + [0]) if tstride is None else tstride
    counts = np.array(list(zip(nv, nt)), np.uint32).reshape(n, 2)
    vertices = np.full((n, vs, 4), 1e30, F)
    indices = np.zeros((n, ts, 3), np.uint32)
    normals = np.full((n, vs, 3), SENTINEL, F)
    for k, (v, i) in enumerate(meshes):
        vertices[k, :nv[k]] = np.asarray(v, F).reshape(-1, 4)
        indices[k, :nt[k]] = np.asarray(i, np.uint32).reshape(-1, 3)
    return counts, vertices, indices, normals


def expected(oracle, meshes, vstride):
    """what `normals` must hold after the call: the oracle's normals, SENTINEL in every slot past a mesh's vertex count"""
    want = np.full((len(meshes), vstride, 3), SENTINEL, F)
    for k, (v, i) in enumerate(meshes):
        want[k, :len(v)] = oracle_normals(oracle, v, i)
    return want
