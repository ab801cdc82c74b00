// rusterix_host.cpp -- see rusterix_host.hpp.  Build with -ffp-contract=off (Rust never fuses).
#include "rusterix_host.hpp"
#include "../rxr_parallel.h"

#include <algorithm>
#include <atomic>
#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <thread>

namespace rusterix {

void *PinnedPool::take(size_t bytes, bool &pinned) {
    pinned = false;
    if (bytes >= threshold) {
        const char *pa = getenv("RXR_PINNED_ARRAYS");  // (0: ordinary memory -- tests and A-B runs)
        if (!(pa && pa[0] == '0'))
            if (void *p = rxr_alloc_pinned(bytes)) {
                pinned = true;
                return p;
            }
        any_unpinned() = true;
    }
    return malloc(bytes);
}
void PinnedPool::give(void *p, bool pinned) {
    if (pinned) rxr_free_pinned(p);
    else free(p);
}


namespace {

// f32::min / f32::max return the non-NaN operand
inline float fmin_rs(float a, float b) { return std::fmin(a, b); }
inline float fmax_rs(float a, float b) { return std::fmax(a, b); }

// Edges::new, src/edge.rs:12-24: p[i] -> q[i] for the three directed edges
inline rxr_edges make_edges(const float p[3][2], const float q[3][2], bool visible) {
    rxr_edges e{};
    for (int i = 0; i < 3; ++i) {
        e.a[i] = q[i][1] - p[i][1];
        e.b[i] = p[i][0] - q[i][0];
        e.c[i] = q[i][0] * p[i][1] - q[i][1] * p[i][0];
    }
    e.visible = visible ? 1u : 0u;
    return e;
}

inline rxr_edges triangle_edges(const float *v0, const float *v1, const float *v2, bool visible) {
    const float p[3][2] = {{v0[0], v0[1]}, {v1[0], v1[1]}, {v2[0], v2[1]}};
    const float q[3][2] = {{v1[0], v1[1]}, {v2[0], v2[1]}, {v0[0], v0[1]}};
    return make_edges(p, q, visible);
}

// src/batch/batch3d.rs:742-746
inline bool front_facing(const float *v0, const float *v1, const float *v2) {
    float orientation = (v1[0] - v0[0]) * (v2[1] - v0[1]) - (v1[1] - v0[1]) * (v2[0] - v0[0]);
    return orientation > 0.0f;
}

struct ClipVertex {
    float pos[4];
    float uv[2];
    Vec3 n;
};

}  // namespace

uint64_t next_generation() {
    static std::atomic<uint64_t> g{1};
    return g.fetch_add(1);
}

uint32_t hash_u32(uint32_t seed) {
    uint32_t state = seed;
    state = (state ^ 61u) ^ (state >> 16);
    state += state << 3;
    state ^= state >> 4;
    state *= 0x27d4eb2du;
    state ^= state >> 15;
    return state;
}

// ---- Batch3D ------------------------------------------------------------------------------------
Batch3D Batch3D::make(const float *verts4, size_t nv, const uint32_t *idx3, size_t nt, const float *uvs2) {
    Batch3D b;
    b.add(verts4, nv, idx3, nt, uvs2);
    return b;
}

void Batch3D::add(const float *verts4, size_t nv, const uint32_t *idx3, size_t nt, const float *uvs2) {
    const uint32_t base_index = (uint32_t)vertex_count();
    vertices.insert(vertices.end(), verts4, verts4 + nv * 4);
    uvs.insert(uvs.end(), uvs2, uvs2 + nv * 2);
    indices.reserve(indices.size() + nt * 3);
    for (size_t i = 0; i < nt * 3; ++i) indices.push_back(idx3[i] + base_index);
    touch();
}

Batch3D Batch3D::from_box(float x, float y, float z, float w, float h, float d) {
    const float X = x + w, Y = y + h, Z = z + d;
    // face order and winding as src/batch/batch3d.rs:141-193
    const float v[24][4] = {
        {x, y, z, 1}, {X, y, z, 1}, {X, Y, z, 1}, {x, Y, z, 1},  // front
        {x, y, Z, 1}, {X, y, Z, 1}, {X, Y, Z, 1}, {x, Y, Z, 1},  // back
        {x, y, z, 1}, {x, Y, z, 1}, {x, Y, Z, 1}, {x, y, Z, 1},  // left
        {X, y, z, 1}, {X, Y, z, 1}, {X, Y, Z, 1}, {X, y, Z, 1},  // right
        {x, Y, z, 1}, {X, Y, z, 1}, {X, Y, Z, 1}, {x, Y, Z, 1},  // top
        {x, y, z, 1}, {X, y, z, 1}, {X, y, Z, 1}, {x, y, Z, 1},  // bottom
    };
    const uint32_t idx[36] = {0, 1, 2, 0, 2, 3, 4, 6, 5, 4, 7, 6, 8, 9, 10, 8, 10, 11, 12, 14, 13, 12, 15, 14,
                              16, 17, 18, 16, 18, 19, 20, 23, 22, 20, 22, 21};
    float uv[24][2];
    for (int f = 0; f < 6; ++f) {
        const float q[4][2] = {{0, 1}, {1, 1}, {1, 0}, {0, 0}};
        memcpy(uv[f * 4], q, sizeof(q));
    }
    return make(&v[0][0], 24, idx, 12, &uv[0][0]);
}

Batch3D Batch3D::from_obj(const std::string &text) {
    // src/wavefront.rs:34-102: `v`, `vt`, `f` (first three corners, index before the first '/')
    Batch3D b;
    std::vector<float> tc;
    size_t pos = 0;
    while (pos < text.size()) {
        size_t eol = text.find('\n', pos);
        if (eol == std::string::npos) eol = text.size();
        std::string line = text.substr(pos, eol - pos);
        pos = eol + 1;
        size_t s = line.find_first_not_of(" \t\r");
        if (s == std::string::npos) continue;
        line = line.substr(s, line.find_last_not_of(" \t\r") - s + 1);
        if (line[0] == '#') continue;
        if (line.compare(0, 2, "v ") == 0) {
            float x = 0, y = 0, z = 0;
            sscanf(line.c_str() + 2, "%f %f %f", &x, &y, &z);
            const float v[4] = {x, y, z, 1.0f};
            b.vertices.insert(b.vertices.end(), v, v + 4);
        } else if (line.compare(0, 3, "vt ") == 0) {
            float u = 0, v = 0;
            sscanf(line.c_str() + 3, "%f %f", &u, &v);
            tc.push_back(u);
            tc.push_back(v);
        } else if (line.compare(0, 2, "f ") == 0) {
            char c0[64], c1[64], c2[64];
            if (sscanf(line.c_str() + 2, "%63s %63s %63s", c0, c1, c2) == 3) {
                b.indices.push_back((uint32_t)strtoul(c0, nullptr, 10) - 1u);
                b.indices.push_back((uint32_t)strtoul(c1, nullptr, 10) - 1u);
                b.indices.push_back((uint32_t)strtoul(c2, nullptr, 10) - 1u);
            }
        }
    }
    if (tc.empty()) {
        for (size_t i = 0; i < b.vertex_count(); ++i) {  // uv = (x, y), :92-95
            b.uvs.push_back(b.vertices[i * 4]);
            b.uvs.push_back(b.vertices[i * 4 + 1]);
        }
    } else {
        b.uvs = tc;
    }
    return b;
}

void Batch3D::compute_vertex_normals() {
    const size_t nv = vertex_count();
    std::vector<Vec3> acc(nv);
    std::vector<uint32_t> counts(nv, 0);
    for (size_t t = 0; t < triangle_count(); ++t) {
        const uint32_t i0 = indices[3 * t], i1 = indices[3 * t + 1], i2 = indices[3 * t + 2];
        Vec3 p0{vertices[4 * i0], vertices[4 * i0 + 1], vertices[4 * i0 + 2]};
        Vec3 p1{vertices[4 * i1], vertices[4 * i1 + 1], vertices[4 * i1 + 2]};
        Vec3 p2{vertices[4 * i2], vertices[4 * i2 + 1], vertices[4 * i2 + 2]};
        Vec3 fn = rvek::normalized(rvek::cross(p1 - p0, p2 - p0));
        acc[i0] += fn;
        acc[i1] += fn;
        acc[i2] += fn;
        ++counts[i0];
        ++counts[i1];
        ++counts[i2];
    }
    normals.assign(nv * 3, 0.0f);
    for (size_t i = 0; i < nv; ++i) {
        Vec3 n = acc[i];
        if (counts[i] > 0) {
            n = n / (float)counts[i];
            n = rvek::normalized(n);
        }
        normals[3 * i] = n.x;
        normals[3 * i + 1] = n.y;
        normals[3 * i + 2] = n.z;
    }
    touch();
}

bool Batch3D::clip_and_project(const Mat4 &view_matrix, const Mat4 &projection_matrix, float viewport_width,
                               float viewport_height) {
    const size_t nv = vertex_count(), nt = triangle_count();
    const Mat4 mvp = (projection_matrix * view_matrix) * transform_3d;

    if (nv > 0) {  // object-space AABB against the clip planes, :493-552
        float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (size_t i = 0; i < nv; ++i)
            for (int k = 0; k < 3; ++k) {
                lo[k] = fmin_rs(lo[k], vertices[4 * i + k]);
                hi[k] = fmax_rs(hi[k], vertices[4 * i + k]);
            }
        bool out_l = true, out_r = true, out_b = true, out_t = true, out_n = true, out_f = true;
        for (int c = 0; c < 8; ++c) {
            Vec4 corner{(c & 4) ? hi[0] : lo[0], (c & 2) ? hi[1] : lo[1], (c & 1) ? hi[2] : lo[2], 1.0f};
            Vec4 v = mvp * corner;
            const float w = v.w;
            out_l &= v.x < -w;
            out_r &= v.x > w;
            out_b &= v.y < -w;
            out_t &= v.y > w;
            out_n &= v.z < -w;
            out_f &= v.z > w;
        }
        if (out_l || out_r || out_b || out_t || out_n || out_f) {
            projected_vertices.clear();
            clipped_indices.clear();
            clipped_uvs.clear();
            clipped_normals.clear();
            edges.clear();
            edge_visible.clear();
            has_bounding_box = false;
            return true;
        }
    }

    const Mat4 view_model = view_matrix * transform_3d;
    std::vector<float> vs(nv * 4);  // view space
    for (size_t i = 0; i < nv; ++i) {
        Vec4 r = view_model * Vec4{vertices[4 * i], vertices[4 * i + 1], vertices[4 * i + 2], vertices[4 * i + 3]};
        vs[4 * i] = r.x; vs[4 * i + 1] = r.y; vs[4 * i + 2] = r.z; vs[4 * i + 3] = r.w;
    }

    const float near_plane = 0.1f;
    clipped_indices.assign(indices.begin(), indices.end());
    clipped_uvs.assign(uvs.begin(), uvs.end());
    clipped_normals.assign(normals.begin(), normals.end());
    std::vector<uint8_t> edge_visibility(nt, 1);
    std::vector<ClipVertex> fresh;  // vertices created by clipping, appended after the originals

    for (size_t t = 0; t < nt; ++t) {
        const uint32_t ix[3] = {indices[3 * t], indices[3 * t + 1], indices[3 * t + 2]};
        const float *v[3] = {&vs[4 * ix[0]], &vs[4 * ix[1]], &vs[4 * ix[2]]};

        if (cull_mode_ != CullMode::Off) {  // :592-600
            float orient = (v[1][0] - v[0][0]) * (v[2][1] - v[0][1]) - (v[1][1] - v[0][1]) * (v[2][0] - v[0][0]);
            bool is_front = orient > 0.0f;
            if (cull_mode_ == CullMode::Back && is_front) continue;
            if (cull_mode_ == CullMode::Front && !is_front) continue;
        }
        // the reference indexes self.normals[i] unconditionally here (:605-607)
        if (normals.size() / 3 <= ix[0] || normals.size() / 3 <= ix[1] || normals.size() / 3 <= ix[2]) return false;

        const bool inside[3] = {v[0][2] < -near_plane, v[1][2] < -near_plane, v[2][2] < -near_plane};
        if (inside[0] && inside[1] && inside[2]) continue;
        edge_visibility[t] = 0;
        if (!inside[0] && !inside[1] && !inside[2]) continue;

        // Sutherland-Hodgman against z = -near_plane, :626-669
        uint32_t poly[4];
        int np = 0;
        size_t emitted = 0;
        for (int i = 0; i < 3; ++i) {
            const int j = (i + 1) % 3;
            const float *cur = v[i], *nxt = v[j];
            const float *uvc = &uvs[2 * ix[i]], *uvn = &uvs[2 * ix[j]];
            Vec3 nc{normals[3 * ix[i]], normals[3 * ix[i] + 1], normals[3 * ix[i] + 2]};
            Vec3 nn{normals[3 * ix[j]], normals[3 * ix[j] + 1], normals[3 * ix[j] + 2]};
            if (cur[2] < -near_plane) {
                ClipVertex cv{{cur[0], cur[1], cur[2], cur[3]}, {uvc[0], uvc[1]}, nc};
                fresh.push_back(cv);
                poly[np++] = (uint32_t)(nv + fresh.size() - 1);
                ++emitted;
            }
            if ((cur[2] < -near_plane) != (nxt[2] < -near_plane)) {
                const float s = (-near_plane - cur[2]) / (nxt[2] - cur[2]);
                ClipVertex cv{};
                for (int k = 0; k < 4; ++k) cv.pos[k] = cur[k] + s * (nxt[k] - cur[k]);
                cv.uv[0] = uvc[0] + s * (uvn[0] - uvc[0]);
                cv.uv[1] = uvc[1] + s * (uvn[1] - uvc[1]);
                cv.n = rvek::normalized(nc * (1.0f - s) + nn * s);
                fresh.push_back(cv);
                poly[np++] = (uint32_t)(nv + fresh.size() - 1);
                ++emitted;
            }
        }
        for (int i = 1; i + 1 < np; ++i) {  // fan, :672-678
            clipped_indices.push_back(poly[0]);
            clipped_indices.push_back(poly[i]);
            clipped_indices.push_back(poly[i + 1]);
        }
        edge_visibility.insert(edge_visibility.end(), emitted, 1);  // one `true` per emitted vertex, :680
    }

    for (const ClipVertex &cv : fresh) {  // :684-686
        vs.insert(vs.end(), cv.pos, cv.pos + 4);
        clipped_uvs.push_back(cv.uv[0]);
        clipped_uvs.push_back(cv.uv[1]);
        clipped_normals.push_back(cv.n.x);
        clipped_normals.push_back(cv.n.y);
        clipped_normals.push_back(cv.n.z);
    }

    const size_t nvp = vs.size() / 4;
    projected_vertices.resize(nvp * 4);
    float min_x = INFINITY, max_x = -INFINITY, min_y = INFINITY, max_y = -INFINITY;
    for (size_t i = 0; i < nvp; ++i) {  // :689-700 and :749-768
        Vec4 r = projection_matrix * Vec4{vs[4 * i], vs[4 * i + 1], vs[4 * i + 2], vs[4 * i + 3]};
        const float w = r.w;
        float *o = &projected_vertices[4 * i];
        o[0] = ((r.x / w) * 0.5f + 0.5f) * viewport_width;
        o[1] = ((-r.y / w) * 0.5f + 0.5f) * viewport_height;
        o[2] = r.z / w;
        o[3] = w;
        min_x = fmin_rs(min_x, o[0]);
        max_x = fmax_rs(max_x, o[0]);
        min_y = fmin_rs(min_y, o[1]);
        max_y = fmax_rs(max_y, o[1]);
    }
    has_bounding_box = true;
    bounding_box = Rect{min_x, min_y, max_x - min_x, max_y - min_y};

    const size_t ntc = clipped_indices.size() / 3;
    edges.resize(ntc);
    edge_visible.resize(ntc);
    for (size_t t = 0; t < ntc; ++t) {  // :706-739
        const float *v0 = &projected_vertices[4 * clipped_indices[3 * t]];
        const float *v1 = &projected_vertices[4 * clipped_indices[3 * t + 1]];
        const float *v2 = &projected_vertices[4 * clipped_indices[3 * t + 2]];
        const bool front = front_facing(v0, v1, v2);
        bool visible, swap;
        switch (cull_mode_) {
            case CullMode::Off: swap = front; visible = true; break;
            case CullMode::Front: swap = false; visible = !front; break;
            default: swap = front; visible = front; break;  // Back
        }
        const bool ev = t < edge_visibility.size() ? edge_visibility[t] != 0 : true;
        edges[t] = swap ? triangle_edges(v0, v2, v1, ev && visible) : triangle_edges(v0, v1, v2, ev && visible);
        edge_visible[t] = (ev && visible) ? 1u : 0u;
    }
    return true;
}

// ---- Batch2D ------------------------------------------------------------------------------------
Batch2D Batch2D::make(const float *verts2, size_t nv, const uint32_t *idx3, size_t nt, const float *uvs2) {
    Batch2D b;
    b.vertices.assign(verts2, verts2 + nv * 2);
    b.uvs.assign(uvs2, uvs2 + nv * 2);
    b.indices.assign(idx3, idx3 + nt * 3);
    return b;
}

Batch2D Batch2D::from_rectangle(float x, float y, float w, float h) {
    const float v[8] = {x, y, x, y + h, x + w, y + h, x + w, y};
    const uint32_t idx[6] = {0, 1, 2, 0, 2, 3};
    const float uv[8] = {0, 0, 0, 1, 1, 1, 1, 0};
    return make(v, 4, idx, 2, uv);
}

void Batch2D::project(const Mat3 *matrix) {
    const size_t nv = vertices.size() / 2;
    projected_vertices.resize(nv * 2);
    float min_x = INFINITY, max_x = -INFINITY, min_y = INFINITY, max_y = -INFINITY;
    for (size_t i = 0; i < nv; ++i) {
        float px = vertices[2 * i], py = vertices[2 * i + 1];
        if (matrix) {
            Vec3 r = (*matrix) * Vec3{px, py, 1.0f};
            px = r.x;
            py = r.y;
        }
        min_x = fmin_rs(min_x, px);
        max_x = fmax_rs(max_x, px);
        min_y = fmin_rs(min_y, py);
        max_y = fmax_rs(max_y, py);
        projected_vertices[2 * i] = px;
        projected_vertices[2 * i + 1] = py;
    }
    has_bounding_box = true;
    bounding_box = Rect{min_x, min_y, max_x - min_x, max_y - min_y};
    const size_t nt = indices.size() / 3;
    edges.resize(nt);
    // Lines batches index only .0/.1 meaningfully; the reference still builds Edges from all three
    for (size_t t = 0; t < nt; ++t) {
        const uint32_t i0 = indices[3 * t], i1 = indices[3 * t + 1], i2 = indices[3 * t + 2];
        if (i0 >= nv || i1 >= nv || i2 >= nv) {
            edges[t] = rxr_edges{};
            continue;
        }
        edges[t] = triangle_edges(&projected_vertices[2 * i0], &projected_vertices[2 * i1], &projected_vertices[2 * i2], true);
    }
}

// ---- Scene --------------------------------------------------------------------------------------
// src/scene.rs:155-215: every batch list is projected with rayon's par_iter_mut -- the batches are independent.  Here: one job per
// batch through the worker pool (rxr_parallel.h), largest lists first come out of the atomic cursor in submission order; frames with
// little geometry run inline.
namespace {
struct ProjectJobs {
    std::vector<Batch2D *> d2;
    std::vector<Batch3D *> d3;
    size_t weight = 0;
    void add(std::vector<Batch2D> &l) {
        for (Batch2D &b : l) {
            d2.push_back(&b);
            weight += b.vertices.size() / 2 + b.indices.size();
        }
    }
    void add(std::vector<Batch3D> &l) {
        for (Batch3D &b : l) {
            d3.push_back(&b);
            weight += 4 * (b.vertices.size() / 4 + b.indices.size());  // clipping, Edges::new, bounding box
        }
    }
};
}  // namespace

std::vector<const Batch3D *> Scene::batches3d_in_order() const {
    std::vector<const Batch3D *> out;
    for (const Chunk &c : chunks) {
        for (const Batch3D &b : c.batches3d_opacity) out.push_back(&b);
        for (const Batch3D &b : c.batches3d) out.push_back(&b);
        for (const Batch3D &b : c.terrain_batch3d) out.push_back(&b);
    }
    for (const Batch3D &b : d3_static) out.push_back(&b);
    for (const Batch3D &b : d3_dynamic) out.push_back(&b);
    for (const Batch3D &b : d3_overlay) out.push_back(&b);
    return out;
}

bool Scene::project(const Mat3 *m2d, const Mat4 &view, const Mat4 &proj, float w, float h,
                    const std::function<void(size_t, const Batch3D &)> *on_projected3d) {
    ProjectJobs jobs;
    for (Chunk &c : chunks) {
        jobs.add(c.batches2d);
        jobs.add(c.terrain_batch2d);
        jobs.add(c.batches3d_opacity);
        jobs.add(c.batches3d);
        jobs.add(c.terrain_batch3d);
    }
    jobs.add(d2_static);
    jobs.add(d2_dynamic);
    jobs.add(d3_static);
    jobs.add(d3_dynamic);
    jobs.add(d3_overlay);
    std::atomic<bool> ok{true};
    const size_t n3 = jobs.d3.size();
    rxr_parallel::run(n3 + jobs.d2.size(), jobs.weight, [&](size_t i) {
        if (i < n3) {
            if (!jobs.d3[i]->clip_and_project(view, proj, w, h)) ok.store(false, std::memory_order_relaxed);
            else if (on_projected3d) (*on_projected3d)(i, *jobs.d3[i]);  // (jobs.d3 is in submission order: batches3d_in_order())
        } else {
            jobs.d2[i - n3]->project(m2d);
        }
    });
    return ok.load();
}

void Scene::project_2d(const Mat3 *m2d) {
    ProjectJobs jobs;
    for (Chunk &c : chunks) {
        jobs.add(c.batches2d);
        jobs.add(c.terrain_batch2d);
    }
    jobs.add(d2_static);
    jobs.add(d2_dynamic);
    rxr_parallel::run(jobs.d2.size(), jobs.weight, [&](size_t i) { jobs.d2[i]->project(m2d); });
}

// ---- device context -----------------------------------------------------------------------------
// The host layer keeps ONE device context (plain or multi-device) and its upload caches per process.  In the reference
// every Rasterizer is an independent value; here Rasterizers on different threads share that context, so every entry point
// that touches it (context, set_device(s), Rasterizer::upload / rasterize) holds g_mu for its whole duration: calls from
// several threads are serialised, never interleaved.
namespace {
std::recursive_mutex g_mu;
rxr_ctx *g_ctx = nullptr;
int g_device = -1;
std::vector<int> g_devices;  // more than one entry: rxr_create_multi
std::string g_error;
uint64_t g_tex_static_gen = 0, g_tex_dynamic_gen = 0;
uint64_t g_shaders_gen = 0, g_shader_env_gen = 0;
uint64_t g_terrain_gen = 0;   // the Terrain::generation the context's resident terrain was registered from (0: none)
uint64_t g_heights_gen = 0;   // the Terrain::heights_generation the context's resident heights were registered from (0: none)
uint64_t g_flatten_gen = 0;   // the Terrain::flatten_generation the context's resident flatten ops were registered from (0: none)
uint64_t g_processed_heights_gen = 0, g_processed_flatten_gen = 0;   // the pair every chunk of the processed grid was last flattened under (0: none)
uint64_t g_heights_registrations = 0, g_flatten_registrations = 0;
uint64_t g_generator_gen = 0; // the TerrainGenerator::generation the context's resident generator records were registered from (0: none)
uint64_t g_exclusion_gen = 0; // ... and the one its resident excluded sectors were registered from (0: none)
uint64_t g_tiles_gen = 0;     // ... and the one its resident tile overrides were registered from (0: none)
// (RXR_DEVICE_PROJECTION=1 in the environment makes device projection the initial choice, as in the Rust shim: shim/.../lib.rs)
bool g_device_projection = [] { const char *e = getenv("RXR_DEVICE_PROJECTION"); return e && e[0] == '1'; }();
bool g_device_edges = !(getenv("RXR_HOST_EDGES") && atoi(getenv("RXR_HOST_EDGES")) != 0);
// the form this thread's current frame takes across the ABI (every 3D batch of a frame the same: rxr.h): without Edges records, unless the
// setting says otherwise or the page-locked streaming hand-over can only be promised for the records (see Rasterizer::upload)
thread_local bool t_frame_edgeless = true;
int g_light_math = RXR_LIGHT_MATH_RELAXED;  // the library's default
uint64_t g_mesh_fingerprint = 0;
uint64_t g_mesh_geometry_fingerprint = 0;  // what rxr_intersect reads of the registered meshes (Scene::intersect)
std::vector<rxr_source> g_mesh_sources;    // the resolved sources the registration was made with (register_meshes), mesh by mesh
uint64_t g_mesh2d_fingerprint = 0;
// resident chunk textures: the Chunk::textures_generation of every chunk the context's registration was made from (g_ctex_held: there is one)
bool g_ctex_held = false;
std::vector<uint64_t> g_ctex_gens;
uint64_t g_ctex_registrations = 0;
}  // namespace

uint64_t chunk_texture_registrations() { return g_ctex_registrations; }
uint64_t terrain_height_registrations() { return g_heights_registrations; }
uint64_t terrain_flatten_registrations() { return g_flatten_registrations; }

void set_device_projection(bool on) { g_device_projection = on; }
bool device_projection() { return g_device_projection; }
void set_device_edges(bool on) { g_device_edges = on; }
bool device_edges() { return g_device_edges; }
void set_light_math(bool exact) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    g_light_math = exact ? RXR_LIGHT_MATH_EXACT : RXR_LIGHT_MATH_RELAXED;
    if (g_ctx) (void)rxr_set_light_math(g_ctx, g_light_math);
}
bool light_math_exact() { return g_light_math == RXR_LIGHT_MATH_EXACT; }

const std::string &last_error() { return g_error; }

namespace {
void drop_context_locked() {
    if (g_ctx) rxr_destroy(g_ctx);
    g_ctx = nullptr;
    g_mesh_fingerprint = g_mesh_geometry_fingerprint = 0;
    g_mesh2d_fingerprint = 0;
    g_tex_static_gen = g_tex_dynamic_gen = 0;
    g_shaders_gen = g_shader_env_gen = 0;
    g_terrain_gen = 0;
    g_heights_gen = 0;
    g_flatten_gen = g_processed_heights_gen = g_processed_flatten_gen = 0;
    g_generator_gen = 0;
    g_exclusion_gen = 0;
    g_tiles_gen = 0;
    g_ctex_held = false;
    g_ctex_gens.clear();
}
}  // namespace

void set_device(int device) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (g_ctx && (device != g_device || g_devices.size() > 1)) drop_context_locked();
    g_device = device;
    g_devices.clear();
}

void set_devices(const int *devices, int n) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    std::vector<int> want(devices, devices + (n > 0 ? n : 0));
    if (want.size() <= 1) {
        set_device(want.empty() ? -1 : want[0]);
        return;
    }
    if (g_ctx && want != g_devices) drop_context_locked();
    if (g_ctx && g_devices.empty()) drop_context_locked();
    g_devices = want;
    g_device = want[0];
}

rxr_ctx *context(std::string *error) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (!g_ctx) {
        int dev = g_device;
        if (dev < 0) {
            const char *e = getenv("RXR_DEVICE");
            if (!e) e = getenv("LOCAL_RANK");
            dev = e ? atoi(e) : 0;
            int n = rxr_device_count();
            if (n > 0) dev %= n;
        }
        int rc = g_devices.size() > 1 ? rxr_create_multi(&g_ctx, g_devices.data(), (int)g_devices.size()) : rxr_create(&g_ctx, dev);
        if (rc != RXR_OK) {
            g_error = rxr_last_error(nullptr);
            if (error) *error = g_error;
            g_ctx = nullptr;
            return nullptr;
        }
        g_device = dev;
        (void)rxr_set_light_math(g_ctx, g_light_math);
    }
    return g_ctx;
}

// ---- Rasterizer ---------------------------------------------------------------------------------
Rasterizer Rasterizer::setup(const Mat3 *m2d, const Mat4 &view, const Mat4 &proj) {
    Rasterizer r;
    r.inverse_view_matrix = rvek::inverted(view);
    r.camera_pos = Vec3{r.inverse_view_matrix.m[12], r.inverse_view_matrix.m[13], r.inverse_view_matrix.m[14]};
    if (m2d) {
        r.has_m2d = true;
        r.projection_matrix_2d = *m2d;
        r.translationd2 = Vec2{m2d->at(0, 2), m2d->at(1, 2)};
        r.scaled2 = m2d->at(0, 0);
    }
    r.inverse_projection_matrix = rvek::inverted(proj);
    r.view_matrix = view;
    r.projection_matrix = proj;
    return r;
}

namespace {

void tile_views(const std::vector<Tile> &tiles, std::vector<rxr_texture> &texs, std::vector<rxr_tile> &out) {
    size_t n = 0;
    for (const Tile &t : tiles) n += t.textures.size();
    texs.clear();
    texs.reserve(n);
    out.clear();
    for (const Tile &t : tiles) {
        rxr_tile rt{};
        rt.textures = texs.data() + texs.size();
        rt.n_textures = (uint32_t)t.textures.size();
        for (const Texture &x : t.textures) texs.push_back(rxr_texture{x.data.data(), x.width, x.height});
        out.push_back(rt);
    }
}

// EntityTile(id, index) / ItemTile(id, index) -> what the device gets: the tile's slot among the dynamic tiles, or
// RXR_SOURCE_MISSING where the reference's two lookups fail (rasterizer.rs:1140-1187, :705-748, :1548-1595)
struct SequenceSlots {
    std::map<std::pair<uint32_t, uint32_t>, uint32_t> entity, item;
    rxr_source resolve(const PixelSource &p) const {
        rxr_source o{};
        o.kind = p.kind;
        o.index = p.index;
        memcpy(o.pixel, p.pixel, 4);
        if (p.kind == RXR_HOST_SOURCE_ENTITY_TILE || p.kind == RXR_HOST_SOURCE_ITEM_TILE) {
            const auto &m = p.kind == RXR_HOST_SOURCE_ENTITY_TILE ? entity : item;
            const auto it = m.find({p.index, p.seq});
            o.kind = it == m.end() ? (uint32_t)RXR_SOURCE_MISSING : (uint32_t)RXR_SOURCE_DYNAMIC_TILE;
            o.index = it == m.end() ? 0u : it->second;
        }
        return o;
    }
};

rxr_batch3d view3d(const Batch3D &b, uint32_t list, int chunk, const SequenceSlots &slots) {
    rxr_batch3d o{};
    o.projected_vertices = b.projected_vertices.data();
    o.clipped_uvs = b.clipped_uvs.data();
    o.clipped_normals = b.normals.empty() ? nullptr : b.clipped_normals.data();
    o.clipped_indices = b.clipped_indices.data();
    o.edges = t_frame_edgeless ? nullptr : b.edges.data();
    o.edge_visible = b.edge_visible.data();
    o.cull_mode = (uint32_t)b.cull_mode_;
    o.n_vertices = (uint32_t)(b.projected_vertices.size() / 4);
    o.n_triangles = (uint32_t)b.edges.size();
    o.has_bounding_box = b.has_bounding_box ? 1u : 0u;
    o.bounding_box[0] = b.bounding_box.x; o.bounding_box[1] = b.bounding_box.y;
    o.bounding_box[2] = b.bounding_box.width; o.bounding_box[3] = b.bounding_box.height;
    o.repeat_mode = b.repeat_mode_;
    o.source = slots.resolve(b.source_);
    o.ambient_color[0] = b.ambient_color_.x; o.ambient_color[1] = b.ambient_color_.y; o.ambient_color[2] = b.ambient_color_.z;
    o.shader = b.shader_;
    o.has_profile_id = b.has_profile_id ? 1u : 0u;
    o.profile_id = b.profile_id_;
    o.list = list;
    o.chunk = chunk;
    return o;
}

rxr_batch2d view2d(const Batch2D &b, int chunk, const SequenceSlots &slots) {
    rxr_batch2d o{};
    o.projected_vertices = b.projected_vertices.data();
    o.uvs = b.uvs.data();
    o.indices = b.indices.data();
    o.edges = t_frame_edgeless ? nullptr : b.edges.data();  // (ABI 5: the library builds Batch2D::project's records itself)
    o.n_vertices = (uint32_t)(b.projected_vertices.size() / 2);
    o.n_triangles = (uint32_t)(b.indices.size() / 3);
    o.has_bounding_box = b.has_bounding_box ? 1u : 0u;
    o.bounding_box[0] = b.bounding_box.x; o.bounding_box[1] = b.bounding_box.y;
    o.bounding_box[2] = b.bounding_box.width; o.bounding_box[3] = b.bounding_box.height;
    o.mode = b.mode_;
    o.repeat_mode = b.repeat_mode_;
    o.source = slots.resolve(b.source_);
    o.receives_light = b.receives_light_ ? 1u : 0u;
    o.shader = b.shader_;
    o.chunk = chunk;
    return o;
}

}  // namespace

namespace {

// The scene's 3D batches as object-space meshes in submission order -- per chunk opacity, chunk, terrain; then static, dynamic, overlay
// (the order of Rasterizer::upload's frame and of Scene::intersect, src/scene.rs:216-276) -- and two FNV-1a fingerprints: `full` over
// everything rxr_set_meshes copies (transforms travel per frame), `geometry` over what rxr_intersect reads of it.  slots == nullptr
// (an intersect without a frame): sources are left unresolved; they are not read by rxr_intersect.  false: a batch with triangles but
// without normals (clip_and_project panics at batch3d.rs:605, and rxr_set_meshes refuses it).
// sources (with slots == nullptr): the resolved sources of an earlier registration, mesh by mesh, in place of the unresolved ones -- `full` is
// then what an upload with unchanged assets computes (Scene::rebuild_* after rxr_resize_meshes_to).
bool scene_meshes(const Scene &scene, const SequenceSlots *slots, std::vector<rxr_mesh3d> &meshes, std::vector<float> *transforms,
                  uint64_t &full, uint64_t &geometry, const std::vector<rxr_source> *sources = nullptr) {
    full = geometry = 1469598103934665603ull;
    auto mix = [](uint64_t &fp, const void *p, size_t n) {
        const uint8_t *q = (const uint8_t *)p;
        for (size_t i = 0; i < n; ++i) fp = (fp ^ q[i]) * 1099511628211ull;
    };
    auto add = [&](const Batch3D &b, uint32_t list, int chunk) -> bool {
        if (!b.indices.empty() && b.normals.size() / 3 < b.vertex_count()) return false;  // batch3d.rs:605 panics
        rxr_mesh3d m{};
        m.vertices = b.vertices.data();
        m.indices = b.indices.data();
        m.uvs = b.uvs.data();
        m.normals = b.normals.empty() ? nullptr : b.normals.data();
        m.n_vertices = (uint32_t)b.vertex_count();
        m.n_triangles = (uint32_t)b.triangle_count();
        memcpy(m.transform_3d, b.transform_3d.m, 64);
        m.cull_mode = (uint32_t)b.cull_mode_;
        m.repeat_mode = b.repeat_mode_;
        if (slots) m.source = slots->resolve(b.source_);
        else if (sources && meshes.size() < sources->size()) m.source = (*sources)[meshes.size()];
        m.ambient_color[0] = b.ambient_color_.x; m.ambient_color[1] = b.ambient_color_.y; m.ambient_color[2] = b.ambient_color_.z;
        m.shader = b.shader_;
        m.has_profile_id = b.has_profile_id ? 1u : 0u;
        m.profile_id = b.profile_id_;
        m.list = list;
        m.chunk = chunk;
        meshes.push_back(m);
        if (transforms) transforms->insert(transforms->end(), b.transform_3d.m, b.transform_3d.m + 16);
        const uint32_t meta[12] = {m.n_vertices, m.n_triangles, m.cull_mode, m.repeat_mode, m.source.kind, m.source.index,
                                   (uint32_t)m.shader, m.has_profile_id, m.profile_id, m.list, (uint32_t)m.chunk,
                                   (uint32_t)b.normals.size()};
        mix(full, meta, sizeof(meta));
        mix(full, m.source.pixel, 4);
        mix(full, m.ambient_color, 12);
        mix(full, &b.geometry_stamp, 8);  // geometry identity (Batch3D::touch)
        const uint32_t gmeta[7] = {m.n_vertices, m.n_triangles, m.has_profile_id, m.profile_id, m.list, (uint32_t)m.chunk,
                                   (uint32_t)b.normals.size()};
        mix(geometry, gmeta, sizeof(gmeta));
        mix(geometry, &b.geometry_stamp, 8);
        return true;
    };
    bool ok = true;
    for (size_t c = 0; c < scene.chunks.size(); ++c) {
        for (const Batch3D &b : scene.chunks[c].batches3d_opacity) ok = ok && add(b, RXR_LIST_CHUNK_OPACITY, (int)c);
        for (const Batch3D &b : scene.chunks[c].batches3d) ok = ok && add(b, RXR_LIST_CHUNK, (int)c);
        for (const Batch3D &b : scene.chunks[c].terrain_batch3d) ok = ok && add(b, RXR_LIST_CHUNK_TERRAIN, (int)c);
    }
    for (const Batch3D &b : scene.d3_static) ok = ok && add(b, RXR_LIST_STATIC, -1);
    for (const Batch3D &b : scene.d3_dynamic) ok = ok && add(b, RXR_LIST_DYNAMIC, -1);
    for (const Batch3D &b : scene.d3_overlay) ok = ok && add(b, RXR_LIST_OVERLAY, -1);
    return ok;
}

// rxr_set_meshes + the two fingerprints of what the context now holds (full: 0 = not known, the next upload registers again)
int register_meshes(rxr_ctx *ctx, const std::vector<rxr_mesh3d> &meshes, uint64_t full, uint64_t geometry) {
    const int rc = rxr_set_meshes(ctx, meshes.data(), (uint32_t)meshes.size());
    if (rc != RXR_OK) {
        g_error = rxr_last_error(ctx);
        g_mesh_fingerprint = g_mesh_geometry_fingerprint = 0;
        return rc;
    }
    g_mesh_fingerprint = full;
    g_mesh_geometry_fingerprint = geometry;
    g_mesh_sources.clear();
    for (const rxr_mesh3d &m : meshes) g_mesh_sources.push_back(m.source);
    return RXR_OK;
}

// Scene::resize_meshes: the context's registration was resized on the device (rxr_resize_meshes_to).  The host batches take the new
// COUNTS -- their arrays keep whatever they held, cut or zero-filled, with every index 0: stale like after an in-place update, but
// still a mesh rxr_set_meshes accepts -- and the fingerprints become what the next upload of this scene computes, so that it sends
// matrices only.  The stamps stay.
void adopt_counts(Batch3D &b, size_t nv, size_t nt) {
    b.vertices.resize(nv * 4, 0.0f);
    b.uvs.resize(nv * 2, 0.0f);
    b.normals.resize(nv * 3, 0.0f);
    b.indices.assign(nt * 3, 0u);
}
void refingerprint_meshes(const Scene &scene) {
    std::vector<rxr_mesh3d> meshes;
    uint64_t full = 0, geometry = 0;
    if (scene_meshes(scene, nullptr, meshes, nullptr, full, geometry, &g_mesh_sources) && meshes.size() == g_mesh_sources.size()) {
        g_mesh_fingerprint = full;
        g_mesh_geometry_fingerprint = geometry;
    } else {
        g_mesh_fingerprint = g_mesh_geometry_fingerprint = 0;   // (the next upload registers again)
    }
}

}  // namespace

namespace {

// Makes the scene's Rusteria programs, the pattern banks and the palette of `assets` the context's resident set (rxr_set_shaders) unless
// they already are.  One table: scene.shaders first, then every chunk's shaders; chunk_program_base[c] is where chunk c's begin
// (rxr_chunk.program_base points into it).
int ensure_shaders(rxr_ctx *ctx, const Scene &scene, const Assets &assets, std::vector<uint32_t> &chunk_program_base) {
    std::vector<const Program *> all_programs;
    for (const Program &p : scene.shaders) all_programs.push_back(&p);
    chunk_program_base.assign(scene.chunks.size(), 0);
    for (size_t c = 0; c < scene.chunks.size(); ++c) {
        chunk_program_base[c] = (uint32_t)all_programs.size();
        for (const Program &p : scene.chunks[c].shaders) all_programs.push_back(&p);
    }
    if (g_shaders_gen != scene.shaders_generation || g_shader_env_gen != assets.shader_env_generation) {
        std::vector<std::vector<rxr_function>> fns(all_programs.size());
        std::vector<rxr_program> progs(all_programs.size());
        for (size_t i = 0; i < all_programs.size(); ++i) {
            const Program &p = *all_programs[i];
            for (const auto &f : p.user_functions) fns[i].push_back(rxr_function{f.data(), (uint32_t)f.size()});
            progs[i] = rxr_program{p.globals, p.shade_index, p.shade_locals, fns[i].data(), (uint32_t)fns[i].size()};
        }
        auto views = [](const std::vector<Pattern> &src) {
            std::vector<rxr_pattern> v;
            for (const Pattern &t : src) v.push_back(rxr_pattern{t.rgb.data(), t.width, t.height});
            return v;
        };
        std::vector<rxr_pattern> pv = views(assets.patterns), pn = views(assets.patterns_normal);
        rxr_shader_set set{};
        set.programs = progs.data();
        set.n_programs = (uint32_t)progs.size();
        set.patterns = pv.data();
        set.n_patterns = (uint32_t)pv.size();
        set.normal_patterns = pn.data();
        set.n_normal_patterns = (uint32_t)pn.size();
        set.palette_rgb = assets.palette_rgb.data();
        set.palette_present = assets.palette_present.data();
        set.n_palette = (uint32_t)assets.palette_present.size();
        int rc = rxr_set_shaders(ctx, &set);
        if (rc != RXR_OK) {
            g_error = rxr_last_error(ctx);
            g_shaders_gen = 0;
            return rc;
        }
        g_shaders_gen = scene.shaders_generation;
        g_shader_env_gen = assets.shader_env_generation;
    }
    return RXR_OK;
}

}  // namespace

int Scene::bake_shaders(const Assets &assets, const uint32_t *programs, uint32_t n, uint32_t width, uint32_t height, float *pixels, uint8_t *rgba) const {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    std::string err;
    rxr_ctx *ctx = context(&err);
    if (!ctx) return RXR_ERR_NO_DEVICE;
    std::vector<uint32_t> chunk_program_base;
    int rc = ensure_shaders(ctx, *this, assets, chunk_program_base);
    if (rc != RXR_OK) return rc;
    rc = rxr_bake_shaders(ctx, programs, n, width, height, pixels, rgba);
    if (rc != RXR_OK) g_error = rxr_last_error(ctx);
    return rc;
}

int Scene::chunk_add_shader(size_t chunk, Program program, const Assets &assets) {
    if (chunk >= chunks.size()) {
        g_error = "Chunk::add_shader: no such chunk";
        return RXR_ERR_INVALID;
    }
    const bool has_shade = program.shade_index >= 0;
    chunks[chunk].shaders.push_back(std::move(program));
    shaders_generation = next_generation();
    Texture tex;
    if (has_shade) {   // chunk.rs:107-122: 64 x 64, as_rgba_bytes
        uint32_t index = (uint32_t)shaders.size();   // the program's place in the context's table (ensure_shaders)
        for (size_t c = 0; c < chunk; ++c) index += (uint32_t)chunks[c].shaders.size();
        index += (uint32_t)chunks[chunk].shaders.size() - 1u;
        tex.width = tex.height = 64;
        tex.data.resize((size_t)64 * 64 * 4);
        const int rc = bake_shaders(assets, &index, 1, 64, 64, nullptr, tex.data.data());
        if (rc != RXR_OK) {   // nothing is added: the caller bakes elsewhere or does without the program
            chunks[chunk].shaders.pop_back();
            shaders_generation = next_generation();
            return rc;
        }
    }
    chunks[chunk].shader_textures.push_back(std::move(tex));
    chunks[chunk].shader_texture_present.push_back(has_shade ? 1 : 0);
    chunks[chunk].touch_textures();
    return (int)chunks[chunk].shaders.size() - 1;
}

int Scene::intersect(const float *origins, const float *dirs, uint32_t n, uint32_t flags, float *t, uint32_t *mesh, uint32_t *triangle,
                     float *hitpoint, float *uv, float *normal) const {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    std::string err;
    rxr_ctx *ctx = context(&err);
    if (!ctx) return RXR_ERR_NO_DEVICE;
    // registered again only when the geometry changed: rxr_set_meshes drops a frame that was uploaded but not yet rendered
    std::vector<rxr_mesh3d> meshes;
    uint64_t full = 0, geometry = 0;
    if (!scene_meshes(*this, nullptr, meshes, nullptr, full, geometry)) {
        g_error = "Scene::intersect: a batch with triangles but without normals cannot be registered (rxr_set_meshes)";
        return RXR_ERR_INVALID;
    }
    if (geometry != g_mesh_geometry_fingerprint || !g_mesh_geometry_fingerprint) {
        int rc = register_meshes(ctx, meshes, 0, geometry);  // (sources unresolved: the next device-projected upload registers again)
        if (rc != RXR_OK) return rc;
    }
    int rc = rxr_set_ray_accel(ctx, ray_accel);
    if (rc == RXR_OK) rc = rxr_set_ray_wave(ctx, ray_wave);
    if (rc == RXR_OK) rc = rxr_set_ray_refresh(ctx, ray_refresh);
    if (rc == RXR_OK) rc = rxr_intersect(ctx, origins, dirs, n, flags, t, mesh, triangle, hitpoint, uv, normal);
    if (rc != RXR_OK) g_error = rxr_last_error(ctx);
    return rc;
}

int Scene::ray_wave_info(uint64_t *out) const {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    std::string err;
    rxr_ctx *ctx = context(&err);
    if (!ctx) return RXR_ERR_NO_DEVICE;
    const int rc = rxr_ray_wave_info(ctx, out);
    if (rc != RXR_OK) g_error = rxr_last_error(ctx);
    return rc;
}

int Scene::ray_accel_info(uint64_t *out) const {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    std::string err;
    rxr_ctx *ctx = context(&err);
    if (!ctx) return RXR_ERR_NO_DEVICE;
    const int rc = rxr_ray_accel_info(ctx, out);
    if (rc != RXR_OK) g_error = rxr_last_error(ctx);
    return rc;
}

int Scene::ray_refresh_info(uint64_t *out) const {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    std::string err;
    rxr_ctx *ctx = context(&err);
    if (!ctx) return RXR_ERR_NO_DEVICE;
    const int rc = rxr_ray_refresh_info(ctx, out);
    if (rc != RXR_OK) g_error = rxr_last_error(ctx);
    return rc;
}

// ---- Tracer (src/tracer/trace.rs, src/tracer/buffer.rs) ------------------------------------------------------------------------
// The CPU path is the loop of rxr_trace.hip (include/rxr.h states it) a pixel at a time: the same operations in the same order on the
// scene's own arrays, the library's generator and sRGB table.  tests/test_trace_cpu.py holds it to tests/trace_ref.py bit for bit.
namespace {
struct T3 {
    float x, y, z;
};
inline T3 t_add(T3 a, T3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
inline T3 t_sub(T3 a, T3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
inline T3 t_mul(T3 a, T3 b) { return {a.x * b.x, a.y * b.y, a.z * b.z}; }
inline T3 t_scale(T3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }
inline T3 t_div(T3 a, float s) { return {a.x / s, a.y / s, a.z / s}; }
inline float t_dot(T3 a, T3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
inline T3 t_cross(T3 a, T3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
inline T3 t_normalized(T3 a) { return t_div(a, std::sqrt(t_dot(a, a))); }
inline T3 t_arr(const float *p) { return {p[0], p[1], p[2]}; }
inline float t_clamp(float x, float lo, float hi) { return x < lo ? lo : (x > hi ? hi : x); }   // f32::clamp: a NaN stays
inline uint32_t t_as_u32(float x) {   // Rust's `as u32`
    if (!(x > 0.0f)) return 0u;
    return x >= 4294967296.0f ? 0xFFFFFFFFu : (uint32_t)x;
}
constexpr float T_PI = 3.14159265358979323846f;

// Texture::sample (texture.rs:203-232, :307-323, :414-460), colour channels
void t_sample(const Texture &tex, float u, float v, uint32_t sample_mode, uint32_t repeat_mode, uint32_t rgb[3]) {
    auto frac = [](float x) { return x - std::floor(x); };
    switch (repeat_mode) {
        case RXR_REPEAT_CLAMP_XY: u = t_clamp(u, 0.0f, 1.0f), v = t_clamp(v, 0.0f, 1.0f); break;
        case RXR_REPEAT_REPEAT_XY: u = frac(u), v = frac(v); break;
        case RXR_REPEAT_REPEAT_X: u = frac(u), v = t_clamp(v, 0.0f, 1.0f); break;
        default: u = t_clamp(u, 0.0f, 1.0f), v = frac(v); break;
    }
    const uint32_t w = tex.width, h = tex.height;
    auto at = [&](uint32_t x, uint32_t y, int c) { return (float)tex.data[((size_t)y * w + x) * 4 + c]; };
    if (sample_mode == RXR_SAMPLE_NEAREST) {
        const uint32_t tx = std::min(t_as_u32(std::round(u * ((float)w - 1.0f))), w - 1u);
        const uint32_t ty = std::min(t_as_u32(std::round(v * ((float)h - 1.0f))), h - 1u);
        for (int c = 0; c < 3; ++c) rgb[c] = (uint32_t)at(tx, ty, c);
        return;
    }
    const float x = u * ((float)w - 1.0f), y = v * ((float)h - 1.0f);
    const float fx = std::floor(x), fy = std::floor(y);
    const uint32_t x0 = std::min(t_as_u32(fx), w - 1u), y0 = std::min(t_as_u32(fy), h - 1u);
    const uint32_t x1 = std::min(x0 + 1u, w - 1u), y1 = std::min(y0 + 1u, h - 1u);
    const float dx = x - fx, dy = y - fy;
    for (int c = 0; c < 3; ++c) {
        const float a = at(x0, y0, c) + dx * (at(x1, y0, c) - at(x0, y0, c));
        const float b = at(x0, y1, c) + dx * (at(x1, y1, c) - at(x0, y1, c));
        rgb[c] = std::min(t_as_u32(std::round(a + dy * (b - a))), 255u);
    }
}

float t_smoothstep(float e0, float e1, float x) {
    const float t = t_clamp((x - e0) / (e1 - e0), 0.0f, 1.0f);
    return t * t * (3.0f - 2.0f * t);
}
T3 t_flicker(const rxr_light &l, float intensity, uint32_t hash) {
    float ff = 1.0f;
    if (l.flicker > 0.0f) {
        const uint32_t combined = hash + (t_as_u32(l.position[0]) + t_as_u32(l.position[1]) + t_as_u32(l.position[2])) * 100u;
        ff = 1.0f - t_clamp((float)combined / 4294967296.0f, 0.0f, 1.0f) * l.flicker;
    }
    return {l.color[0] * intensity * ff, l.color[1] * intensity * ff, l.color[2] * intensity * ff};
}
// CompiledLight::radiance_at(point, Some(normal), hash) over color_at(point, hash, false) (map/light.rs:491-677)
bool t_radiance(const rxr_light &l, T3 point, T3 n, uint32_t hash, T3 &out) {
    if (!l.emitting) return false;
    const T3 lp = t_arr(l.position), tp = t_sub(point, lp);
    const float distance = std::sqrt(t_dot(tp, tp));
    bool lambert = true;
    switch (l.light_type) {
        case RXR_LIGHT_POINT:
            if (distance >= l.end_distance) return false;
            out = distance <= l.start_distance ? t_flicker(l, l.intensity, hash)
                                               : t_flicker(l, l.intensity * t_smoothstep(l.end_distance, l.start_distance, distance), hash);
            break;
        case RXR_LIGHT_AMBIENT:
        case RXR_LIGHT_AMBIENT_DAYLIGHT:
            out = t_flicker(l, l.intensity, hash);
            lambert = false;
            break;
        case RXR_LIGHT_SPOT: {
            if (distance >= l.end_distance) return false;
            const float att = distance <= l.start_distance ? 1.0f : 1.0f - ((distance - l.start_distance) / (l.end_distance - l.start_distance));
            if (std::acos(t_dot(t_arr(l.direction), t_normalized(tp))) > l.cone_angle) return false;
            out = t_flicker(l, l.intensity * att, hash);
            break;
        }
        case RXR_LIGHT_AREA: {
            if (distance >= l.end_distance) return false;
            if (distance < 0.1f) {
                out = t_arr(l.color);
                break;
            }
            const float datt = distance <= l.start_distance ? 1.0f : t_smoothstep(l.end_distance, l.start_distance, distance);
            const float area = l.width * l.height;
            const T3 direction = t_normalized(tp);
            const float att = l.from_linedef ? datt * area * l.intensity : std::fmax(t_dot(t_arr(l.normal), direction), 0.0f) * datt * area * l.intensity;
            out = {l.color[0] * att, l.color[1] * att, l.color[2] * att};
            break;
        }
        default: {   // Daylight
            if (distance >= l.end_distance) return false;
            const float aa = std::fmax(t_dot(t_arr(l.normal), t_normalized(tp)), 0.0f);
            const float datt = distance <= l.start_distance ? 1.0f : t_smoothstep(l.end_distance, l.start_distance, distance);
            const float att = aa * datt * l.intensity;
            out = {l.color[0] * att, l.color[1] * att, l.color[2] * att};
            lambert = false;
            break;
        }
    }
    if (lambert) out = t_scale(out, std::fmax(t_dot(n, t_normalized(t_sub(lp, point))), 0.0f));
    return true;
}

float t_modify(uint32_t modifier, T3 c, float strength) {   // MaterialModifier::modify, shapestack/material.rs:80-110
    if (modifier == 1 || modifier == 3) {
        const float lum = (0.2126f * c.x + 0.7152f * c.y) + 0.0722f * c.z;
        return modifier == 1 ? lum * strength : (1.0f - lum) * strength;
    }
    if (modifier == 2 || modifier == 4) {
        const float mx = std::fmax(c.x, std::fmax(c.y, c.z)), mn = std::fmin(c.x, std::fmin(c.y, c.z));
        const float sat = mx > 0.0f ? (mx - mn) / mx : 0.0f;
        return modifier == 2 ? sat * strength : (1.0f - sat) * strength;
    }
    return strength;
}

struct TracedBatch {
    const Batch3D *b;
    const Chunk *chunk;
};

struct CpuTrace {
    uint32_t kind, width, height, seed, bounces, sample_mode, hash_anim;
    T3 pos, fwd, right, up;
    float half_w, half_h;
    const Scene *scene;
    const Assets *assets;
    std::vector<TracedBatch> batches;
    std::vector<rxr_light> lights;
    float srgb[256];

    // one sample of pixel i of frame `frame` (trace.rs:169-351)
    T3 sample(uint32_t i, uint32_t frame) const {
        const float sx = (float)width, sy = (float)height;
        const float uvx = (float)(i % width) / sx;
        float uvy = 1.0f - (float)(i / width) / sy;
        const float jx = rxr_trace_rand(seed, frame, i, 0u), jy = rxr_trace_rand(seed, frame, i, 1u);
        T3 o = pos, d;
        if (kind == RXR_TRACE_CAMERA_FIRSTP) {
            const float psx = 1.0f / sx, psy = 1.0f / sy;
            const T3 lower_left = t_sub(t_sub(t_add(pos, fwd), t_scale(right, half_w)), t_scale(up, half_h));
            const T3 horizontal = t_scale(right, 2.0f * half_w), vertical = t_scale(up, 2.0f * half_h);
            d = t_normalized(t_sub(t_add(t_add(lower_left, t_scale(horizontal, psx * jx + uvx)), t_scale(vertical, psy * jy + uvy)), pos));
        } else if (kind == RXR_TRACE_CAMERA_ORBIT) {
            const float psx = 1.0f / sx, psy = 1.0f / sy;
            uvy = 1.0f - uvy;
            const float nx = (psx * jx + uvx) * 2.0f - 1.0f, ny = (psy * jy + uvy) * 2.0f - 1.0f;
            d = t_normalized(t_sub(t_add(fwd, t_scale(t_scale(right, nx), half_w)), t_scale(t_scale(up, ny), half_h)));
        } else {
            const T3 horizontal = t_scale({-right.x, -right.y, -right.z}, 2.0f * half_w), vertical = t_scale(up, 2.0f * half_h);
            const float psx = 1.0f / std::fmax(sx, 1.0f), psy = 1.0f / std::fmax(sy, 1.0f);
            o = t_add(t_add(pos, t_scale(horizontal, (psx * jx + uvx) - 0.5f)), t_scale(vertical, (psy * jy + uvy) - 0.5f));
            d = fwd;
        }
        T3 ret{0.0f, 0.0f, 0.0f}, thr{1.0f, 1.0f, 1.0f};
        for (uint32_t bounce = 0; bounce < bounces; ++bounce) {
            // the closest hit: Batch3D::intersect per batch (batch3d.rs:844-948), folded by a strict `<`
            const T3 ld = t_normalized(d);
            float best_t = FLT_MAX, bu = 0.0f, bv = 0.0f;
            const TracedBatch *hit = nullptr;
            size_t htri = 0;
            for (const TracedBatch &tb : batches) {
                const Batch3D &B = *tb.b;
                for (size_t k = 0; k < B.triangle_count(); ++k) {
                    const T3 p0 = t_arr(&B.vertices[4 * (size_t)B.indices[3 * k]]);
                    const T3 e1 = t_sub(t_arr(&B.vertices[4 * (size_t)B.indices[3 * k + 1]]), p0), e2 = t_sub(t_arr(&B.vertices[4 * (size_t)B.indices[3 * k + 2]]), p0);
                    const T3 h = t_cross(ld, e2);
                    const float a = t_dot(e1, h);
                    if (std::fabs(a) < 1e-6f) continue;
                    const float f = 1.0f / a;
                    const T3 s = t_sub(o, p0);
                    const float u = f * t_dot(s, h);
                    if (!(u >= 0.0f && u <= 1.0f)) continue;
                    const T3 q = t_cross(s, e1);
                    const float v = f * t_dot(ld, q);
                    if (v < 0.0f || u + v > 1.0f) continue;
                    const float t = f * t_dot(e2, q);
                    if (t > 1e-4f && t < best_t) best_t = t, bu = u, bv = v, hit = &tb, htri = k;
                }
            }
            if (!hit) break;   // a miss adds nothing and ends the path
            const Batch3D &B = *hit->b;
            const float w = (1.0f - bu) - bv;
            const uint32_t i0 = B.indices[3 * htri], i1 = B.indices[3 * htri + 1], i2 = B.indices[3 * htri + 2];
            const float uvhx = (w * B.uvs[2 * i0] + bu * B.uvs[2 * i1]) + bv * B.uvs[2 * i2];
            const float uvhy = (w * B.uvs[2 * i0 + 1] + bu * B.uvs[2 * i1 + 1]) + bv * B.uvs[2 * i2 + 1];
            const T3 n0 = t_arr(&B.normals[3 * i0]), n1 = t_arr(&B.normals[3 * i1]), n2 = t_arr(&B.normals[3 * i2]);
            T3 n = t_normalized({(n0.x * w + n1.x * bu) + n2.x * bv, (n0.y * w + n1.y * bu) + n2.y * bv, (n0.z * w + n1.z * bu) + n2.z * bv});
            if (t_dot(n, d) > 0.0f) n = {-n.x, -n.y, -n.z};
            const T3 world = t_add(o, t_scale(d, best_t));
            // evaluate_hit (trace.rs:377-475)
            uint32_t px[3] = {0u, 0u, 0u};
            const PixelSource &src = B.source_;
            if (src.kind == RXR_SOURCE_PIXEL) {
                for (int c = 0; c < 3; ++c) px[c] = src.pixel[c];
            } else if (src.kind == RXR_SOURCE_STATIC_TILE || src.kind == RXR_SOURCE_DYNAMIC_TILE) {
                const Tile &tile = src.kind == RXR_SOURCE_STATIC_TILE ? assets->tile_list[src.index] : scene->dynamic_textures[src.index];
                t_sample(tile.textures[scene->animation_frame % tile.textures.size()], uvhx, uvhy, sample_mode, B.repeat_mode_, px);
            } else if (src.kind == RXR_SOURCE_TERRAIN && hit->chunk && hit->chunk->has_terrain_texture) {   // chunk.rs:133-151
                const Chunk &C = *hit->chunk;
                const Texture &tex = C.terrain_texture;
                const float ppt = (float)((int32_t)tex.width / C.size);
                const float pixel_x = ((world.x / 1.0f) - (float)C.origin[0]) * ppt, pixel_y = ((world.z / 1.0f) - (float)C.origin[1]) * ppt;
                const uint32_t tx = std::min(t_as_u32(t_clamp(std::floor(pixel_x), 0.0f, (float)tex.width - 1.0f)), tex.width - 1u);
                const uint32_t ty = std::min(t_as_u32(t_clamp(std::floor(pixel_y), 0.0f, (float)tex.height - 1.0f)), tex.height - 1u);
                for (int c = 0; c < 3; ++c) px[c] = tex.data[((size_t)ty * tex.width + tx) * 4 + c];
            }
            const T3 tex_lin = {srgb[px[0]], srgb[px[1]], srgb[px[2]]};
            float specular_weight = 0.0f;
            T3 emissive{0.0f, 0.0f, 0.0f};
            if (B.has_material) {
                const float inv = 1.0f / 255.0f;
                const float value = t_modify(B.material_modifier, {(float)px[0] * inv, (float)px[1] * inv, (float)px[2] * inv}, B.material_value);
                if (B.material_role == 0) specular_weight = 1.0f - value;
                else if (B.material_role == 1 || B.material_role == 2) specular_weight = value;
                else if (B.material_role == 4) emissive = t_scale(t_scale(tex_lin, B.material_value), 10.0f);
            }
            const T3 albedo = tex_lin;
            if (emissive.x != 0.0f || emissive.y != 0.0f || emissive.z != 0.0f) {
                ret = t_add(ret, t_mul(emissive, thr));
                break;
            }
            T3 direct{0.0f, 0.0f, 0.0f};
            for (const rxr_light &l : lights) {
                T3 lc;
                if (t_radiance(l, world, n, hash_anim, lc)) direct = t_add(direct, t_scale(lc, 10.0f));
            }
            ret = t_add(ret, t_mul(direct, t_mul(thr, t_div(albedo, T_PI))));
            const uint32_t slot = 2u + 4u * bounce;
            const float r_spec = rxr_trace_rand(seed, frame, i, slot), r1 = rxr_trace_rand(seed, frame, i, slot + 1u);
            const float r2 = rxr_trace_rand(seed, frame, i, slot + 2u), r_roulette = rxr_trace_rand(seed, frame, i, slot + 3u);
            const float p_spec = t_clamp(specular_weight, 0.0f, 1.0f), p_diff = 1.0f - p_spec;
            const bool choose_spec = r_spec < p_spec;
            const float pdf = choose_spec ? p_spec : p_diff;
            T3 nd;
            if (choose_spec) {
                nd = t_sub(d, t_scale(n, 2.0f * t_dot(d, n)));
                thr = t_scale(thr, specular_weight / pdf);
            } else {   // sample_cosine (trace.rs:493-512)
                const float phi = (2.0f * T_PI) * r1, r = std::sqrt(r2);
                const T3 local = {std::cos(phi) * r, std::sin(phi) * r, std::sqrt(1.0f - r2)};
                const T3 a = std::fabs(n.x) > 0.1f ? T3{0.0f, 1.0f, 0.0f} : T3{1.0f, 0.0f, 0.0f};
                const T3 v = t_normalized(t_cross(n, a)), u = t_cross(v, n);
                nd = t_normalized(t_add(t_add(t_scale(u, local.x), t_scale(v, local.y)), t_scale(n, local.z)));
                thr = t_mul(thr, t_div(t_scale(albedo, p_diff), pdf * T_PI));
            }
            o = t_add(t_add(o, t_scale(nd, best_t)), t_scale(n, 0.01f));   // ray.at(t) along the NEW direction (trace.rs:301-309)
            d = nd;
            const float p = t_clamp(std::fmax(thr.x, std::fmax(thr.y, thr.z)), 0.001f, 1.0f);
            if (r_roulette > p) break;
            thr = t_scale(thr, 1.0f / p);
        }
        return ret;
    }
};
}  // namespace

std::vector<uint8_t> AccumBuffer::to_u8_vec() const {
    std::vector<uint8_t> out(pixels.size());
    auto as_u8 = [](float x) { return (uint8_t)std::min(t_as_u32(x), 255u); };
    for (size_t i = 0; i < pixels.size(); ++i) {
        const float x = pixels[i];
        if (i % 4 == 3) {
            out[i] = as_u8(t_clamp(x, 0.0f, 1.0f) * 255.0f + 0.5f);
        } else {
            const float srgb = x <= 0.0031308f ? x * 12.92f : 1.055f * std::pow(x, 1.0f / 2.4f) - 0.055f;
            out[i] = as_u8(t_clamp(srgb, 0.0f, 1.0f) * 255.0f + 0.5f);
        }
    }
    return out;
}

int Tracer::trace(uint32_t camera_kind, const float *camera, const Scene &scene, AccumBuffer &accum, const Assets &assets, uint32_t n_frames,
                  uint32_t seed, uint32_t bounces, bool cpu, unsigned threads) const {
    if (!camera || !accum.width || !accum.height || accum.pixels.size() != accum.width * accum.height * 4 || !n_frames || camera_kind > RXR_TRACE_CAMERA_ISO) {
        g_error = "Tracer::trace: NULL camera, an unknown camera kind, an empty buffer or no frames";
        return RXR_ERR_INVALID;
    }
    if (bounces > RXR_TRACE_MAX_BOUNCES) {
        g_error = "Tracer::trace: more than RXR_TRACE_MAX_BOUNCES bounces";
        return RXR_ERR_UNSUPPORTED;
    }
    std::vector<rxr_light> lights(scene.lights);
    lights.insert(lights.end(), scene.dynamic_lights.begin(), scene.dynamic_lights.end());
    if (cpu) {
        CpuTrace T{};
        T.kind = camera_kind, T.width = (uint32_t)accum.width, T.height = (uint32_t)accum.height, T.seed = seed, T.bounces = bounces;
        T.sample_mode = sample_mode;
        uint32_t h = (uint32_t)scene.animation_frame;   // hash_u32 (trace.rs:119-128)
        h = (h ^ 61u) ^ (h >> 16), h = h + (h << 3), h ^= h >> 4, h = h * 0x27d4eb2du, h ^= h >> 15;
        T.hash_anim = h;
        T.pos = t_arr(camera), T.fwd = t_arr(camera + 3), T.right = t_arr(camera + 6), T.up = t_arr(camera + 9);
        T.half_w = camera[12], T.half_h = camera[13];
        T.scene = &scene, T.assets = &assets, T.lights = lights;
        (void)rxr_trace_srgb_table(nullptr, T.srgb);
        auto add = [&](const Batch3D &b, const Chunk *c) -> bool {
            if (b.triangle_count() && b.normals.size() / 3 < b.vertex_count()) return false;
            if (b.source_.kind == RXR_SOURCE_STATIC_TILE || b.source_.kind == RXR_SOURCE_DYNAMIC_TILE) {
                const std::vector<Tile> &tiles = b.source_.kind == RXR_SOURCE_STATIC_TILE ? assets.tile_list : scene.dynamic_textures;
                if (b.triangle_count() && (b.source_.index >= tiles.size() || tiles[b.source_.index].textures.empty())) return false;
            }
            if (b.source_.kind == RXR_SOURCE_TERRAIN && c && c->has_terrain_texture && c->size < 1) return false;
            T.batches.push_back({&b, c});
            return true;
        };
        bool ok = true;
        for (const Chunk &c : scene.chunks) {   // (the opacity and overlay lists take no part)
            for (const Batch3D &b : c.batches3d) ok = ok && add(b, &c);
            for (const Batch3D &b : c.terrain_batch3d) ok = ok && add(b, &c);
        }
        for (const Batch3D &b : scene.d3_static) ok = ok && add(b, nullptr);
        for (const Batch3D &b : scene.d3_dynamic) ok = ok && add(b, nullptr);
        if (!ok) {
            g_error = "Tracer::trace: a batch without normals, with a tile that does not exist or in a chunk of size 0 (the reference panics)";
            return RXR_ERR_INVALID;
        }
        const uint32_t n = T.width * T.height;
        unsigned nt = threads ? threads : std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
        nt = std::max(1u, std::min(nt, n));
        for (uint32_t k = 0; k < n_frames; ++k) {
            const uint32_t frame = (uint32_t)accum.frame;
            const float t = 1.0f / ((float)accum.frame + 1.0f), keep = 1.0f - t;
            auto rows = [&](unsigned worker) {
                for (uint32_t i = worker; i < n; i += nt) {   // (interleaved: neighbouring pixels cost alike)
                    const T3 ret = T.sample(i, frame);
                    float *p = &accum.pixels[4 * (size_t)i];
                    p[0] = p[0] * keep + ret.x * t, p[1] = p[1] * keep + ret.y * t, p[2] = p[2] * keep + ret.z * t, p[3] = p[3] * keep + 1.0f * t;
                }
            };
            std::vector<std::thread> pool;
            for (unsigned w = 1; w < nt; ++w) pool.emplace_back(rows, w);
            rows(0);
            for (std::thread &th : pool) th.join();
            accum.frame += 1;
        }
        return RXR_OK;
    }
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    std::string err;
    rxr_ctx *ctx = context(&err);
    if (!ctx) return RXR_ERR_NO_DEVICE;
    // the tiles and the 3D batches, as Rasterizer::upload registers them
    SequenceSlots slots;
    std::vector<const Tile *> dyn_tiles;
    for (const Tile &t : scene.dynamic_textures) dyn_tiles.push_back(&t);
    for (int pass = 0; pass < 2; ++pass)
        for (const auto &kv : pass == 0 ? assets.entity_tiles : assets.item_tiles)
            for (size_t k = 0; k < kv.second.size(); ++k) {
                (pass == 0 ? slots.entity : slots.item)[{kv.first, (uint32_t)k}] = (uint32_t)dyn_tiles.size();
                dyn_tiles.push_back(&kv.second[k]);
            }
    if (g_tex_static_gen != assets.generation || g_tex_dynamic_gen != scene.dynamic_textures_generation) {
        std::vector<rxr_texture> ts, td;
        std::vector<rxr_tile> tiles_s, tiles_d;
        tile_views(assets.tile_list, ts, tiles_s);
        size_t nd = 0;
        for (const Tile *t : dyn_tiles) nd += t->textures.size();
        td.reserve(nd);
        for (const Tile *t : dyn_tiles) {
            rxr_tile rt{};
            rt.textures = td.data() + td.size();
            rt.n_textures = (uint32_t)t->textures.size();
            for (const Texture &x : t->textures) td.push_back(rxr_texture{x.data.data(), x.width, x.height});
            tiles_d.push_back(rt);
        }
        const int rc = rxr_set_textures(ctx, tiles_s.data(), (uint32_t)tiles_s.size(), tiles_d.data(), (uint32_t)tiles_d.size());
        if (rc != RXR_OK) {
            g_error = rxr_last_error(ctx);
            return rc;
        }
        g_tex_static_gen = assets.generation;
        g_tex_dynamic_gen = scene.dynamic_textures_generation;
    }
    std::vector<rxr_mesh3d> meshes;
    uint64_t full = 0, geometry = 0;
    if (!scene_meshes(scene, &slots, meshes, nullptr, full, geometry)) {
        g_error = "Tracer::trace: a batch with triangles but without normals cannot be registered (rxr_set_meshes)";
        return RXR_ERR_INVALID;
    }
    if (full != g_mesh_fingerprint || !g_mesh_fingerprint) {
        const int rc = register_meshes(ctx, meshes, full, geometry);
        if (rc != RXR_OK) return rc;
    }
    std::vector<uint32_t> kinds;
    std::vector<float> values;
    for (const Batch3D *b : scene.batches3d_in_order()) {
        kinds.push_back(b->has_material ? b->material_role : RXR_TRACE_NO_MATERIAL);
        kinds.push_back(b->has_material ? b->material_modifier : 0u);
        values.push_back(b->material_value);
    }
    std::vector<int32_t> chunk_rec;
    for (const Chunk &c : scene.chunks) chunk_rec.insert(chunk_rec.end(), {c.origin[0], c.origin[1], c.size});
    int rc = rxr_set_trace_scene(ctx, kinds.data(), values.data(), (uint32_t)meshes.size(), lights.data(), (uint32_t)lights.size(), sample_mode,
                                 (uint64_t)scene.animation_frame, chunk_rec.data(), (uint32_t)scene.chunks.size());
    if (rc == RXR_OK) rc = rxr_set_ray_accel(ctx, scene.ray_accel);
    if (rc == RXR_OK) rc = rxr_set_ray_wave(ctx, scene.ray_wave);
    if (rc == RXR_OK) rc = rxr_set_ray_refresh(ctx, scene.ray_refresh);
    if (rc == RXR_OK) rc = rxr_trace(ctx, camera_kind, camera, (uint32_t)accum.width, (uint32_t)accum.height, (uint32_t)accum.frame, n_frames, seed, bounces, accum.pixels.data());
    if (rc != RXR_OK) {
        g_error = rxr_last_error(ctx);
        return rc;
    }
    accum.frame += n_frames;
    return RXR_OK;
}

// ---- Terrain --------------------------------------------------------------------------------------
namespace {
int32_t div_euclid(int32_t a, int32_t b) {
    int32_t q = a / b;
    if (a % b < 0) q -= 1;   // (b > 0)
    return q;
}
// Rust's `x as i32` / `x as usize` / `x as u8`: saturating, NaN -> 0
int32_t as_i32(float x) {
    if (x != x) return 0;
    if (x <= -2147483648.0f) return INT32_MIN;
    if (x >= 2147483648.0f) return INT32_MAX;
    return (int32_t)x;
}
size_t as_usize(float x) {
    if (!(x > 0.0f)) return 0;
    if (x >= 18446744073709551616.0f) return SIZE_MAX;
    return (size_t)x;
}
uint8_t as_u8(float x) {
    if (!(x > 0.0f)) return 0;
    if (x >= 255.0f) return 255;
    return (uint8_t)x;
}

// the read side of a Terrain for one bake
struct TerrainSampler {
    const Terrain &t;
    const Terrain::Cell *cell(int32_t x, int32_t y) const {
        auto it = t.cells.find({x, y});
        return it == t.cells.end() ? nullptr : &it->second;
    }
    // sample_source, src/terrain/mod.rs:197-245
    bool sample_source(float wx, float wy, uint8_t px[4]) const {
        const float qx = wx / t.scale[0], qy = wy / t.scale[1];
        const int32_t x = as_i32(std::floor(qx)), y = as_i32(std::floor(qy));
        float u = qx - std::trunc(qx), v = qy - std::trunc(qy);   // f32::fract
        if (u < 0.0f) u = u + 1.0f;
        if (v < 0.0f) v = v + 1.0f;
        const Terrain::Cell *c = cell(x, y);
        if (c && c->has_source && c->texture >= 0) {
            const Texture &tex = t.textures[(size_t)c->texture];   // Texture::sample_nearest, src/texture.rs:307-323
            size_t tx = as_usize(std::round(u * ((float)tex.width - 1.0f))), ty = as_usize(std::round(v * ((float)tex.height - 1.0f)));
            tx = std::min<size_t>(tx, tex.width - 1);
            ty = std::min<size_t>(ty, tex.height - 1);
            memcpy(px, tex.data.data() + (ty * tex.width + tx) * 4, 4);
            return true;
        }
        const uint8_t g = (((x & 1) ^ (y & 1)) == 0) ? 135 : 120;
        px[0] = px[1] = px[2] = g;
        px[3] = 255;
        return false;
    }
    // sample_source_blended_radius, :247-298
    void blended(float wx, float wy, float radius, uint8_t px[4]) const {
        Vec3 sum{0.0f, 0.0f, 0.0f};
        float weight_sum = 0.0f;
        const float step = std::min(t.scale[0], t.scale[1]) * 0.5f;
        const float radius_squared = radius * radius;
        const int32_t steps = as_i32(std::ceil(radius / step));
        for (int32_t dy = -steps; dy <= steps; ++dy)
            for (int32_t dx = -steps; dx <= steps; ++dx) {
                const float ox = (float)dx * step, oy = (float)dy * step;
                const float dist2 = ox * ox + oy * oy;
                if (dist2 > radius_squared) continue;
                uint8_t p[4];
                if (sample_source(wx + ox, wy + oy, p)) {
                    const float tt = 1.0f - (dist2 / radius_squared);
                    const float weight = tt * tt;
                    sum += Vec3{(float)p[0], (float)p[1], (float)p[2]} * weight;
                    weight_sum += weight;
                }
            }
        if (weight_sum > 0.0f) {
            const Vec3 avg = sum / weight_sum;
            px[0] = as_u8(std::round(avg.x));
            px[1] = as_u8(std::round(avg.y));
            px[2] = as_u8(std::round(avg.z));
        } else {
            const int32_t x = as_i32(std::floor(wx / t.scale[0])), y = as_i32(std::floor(wy / t.scale[1]));
            px[0] = px[1] = px[2] = (((x ^ y) & 1) == 0) ? 120 : 135;
        }
        px[3] = 255;
    }
};
}  // namespace

void Terrain::set_source(int32_t x, int32_t y, const Texture *texture) {
    Cell &c = cells[{x, y}];
    c.has_source = true;
    c.texture = -1;
    if (texture && texture->width && texture->height) {
        size_t i = 0;
        for (; i < textures.size(); ++i)
            if (textures[i].width == texture->width && textures[i].height == texture->height && textures[i].data == texture->data) break;
        if (i == textures.size()) textures.push_back(*texture);
        c.texture = (int32_t)i;
    }
    chunks.insert({div_euclid(x, chunk_size), div_euclid(y, chunk_size)});
    touch();
}

void Terrain::set_blend_mode(int32_t x, int32_t y, uint32_t kind, uint32_t radius, float offset_x, float offset_y) {
    Cell &c = cells[{x, y}];
    c.blend = kind == RXR_TERRAIN_BLEND_NONE ? RXR_TERRAIN_BLEND_NONE : (kind | (radius & 255u) << 8);
    c.offset[0] = kind == RXR_TERRAIN_BLEND_OFFSET ? offset_x : 0.0f;
    c.offset[1] = kind == RXR_TERRAIN_BLEND_OFFSET ? offset_y : 0.0f;
    chunks.insert({div_euclid(x, chunk_size), div_euclid(y, chunk_size)});
    touch();
}

void Terrain::flatten(std::vector<int32_t> &xy, std::vector<int32_t> &texture, std::vector<uint32_t> &blend, std::vector<float> &offset) const {
    for (const auto &kv : cells) {
        xy.push_back(kv.first.first);
        xy.push_back(kv.first.second);
        texture.push_back(kv.second.has_source ? kv.second.texture : -1);
        blend.push_back(kv.second.blend);
        offset.push_back(kv.second.offset[0]);
        offset.push_back(kv.second.offset[1]);
    }
}

int Terrain::bake_chunk(int32_t cx, int32_t cy, int32_t ppt, std::vector<uint8_t> &rgba) const {
    if (!(std::isfinite(scale[0]) && std::isfinite(scale[1]) && scale[0] > 0.0f && scale[1] > 0.0f) || chunk_size < 1 || ppt < 1) {
        g_error = "Terrain::bake_chunk: scale must be finite and > 0, chunk_size and pixels_per_tile at least 1";
        return RXR_ERR_INVALID;
    }
    const int64_t min_x = (int64_t)cx * chunk_size, min_y = (int64_t)cy * chunk_size, side = (int64_t)chunk_size * ppt;
    if (min_x < INT32_MIN || min_x > INT32_MAX || min_y < INT32_MIN || min_y > INT32_MAX || side > RXR_BAKE_MAX_DIM) {
        g_error = "Terrain::bake_chunk: chunk coordinates or texture size out of range";
        return RXR_ERR_INVALID;
    }
    std::lock_guard<std::recursive_mutex> lk(g_mu);   // (the worker pool runs one job at a time)
    rgba.assign((size_t)side * side * 4, 0);
    const TerrainSampler S{*this};
    rxr_parallel::run((size_t)side, (size_t)side * side * 16, [&](size_t y) {   // :331-366, one row per item
        uint8_t *line = rgba.data() + y * (size_t)side * 4;
        for (int64_t x = 0; x < side; ++x) {
            const float tile_x = (float)(int32_t)min_x + ((float)x / (float)ppt), tile_y = (float)(int32_t)min_y + ((float)y / (float)ppt);
            const float world_x = tile_x * scale[0], world_y = tile_y * scale[1];
            const Cell *c = S.cell(as_i32(std::floor(tile_x)), as_i32(std::floor(tile_y)));
            const uint32_t kind = c ? (c->blend & 255u) : RXR_TERRAIN_BLEND_NONE;
            uint8_t *px = line + x * 4;
            if (kind == RXR_TERRAIN_BLEND_NONE) (void)S.sample_source(world_x, world_y, px);
            else if (kind == RXR_TERRAIN_BLEND_RADIUS) S.blended(world_x, world_y, (float)((c->blend >> 8) & 255u), px);
            else S.blended(world_x + c->offset[0], world_y + c->offset[1], (float)((c->blend >> 8) & 255u), px);
        }
    });
    return RXR_OK;
}

namespace {
// rxr_set_terrain unless the context holds this generation of the terrain
int register_terrain(rxr_ctx *ctx, const Terrain &T) {
    if (g_terrain_gen == T.generation) return RXR_OK;
    std::vector<int32_t> xy, texture;
    std::vector<uint32_t> blend;
    std::vector<float> offset;
    T.flatten(xy, texture, blend, offset);
    std::vector<rxr_texture> tex;
    for (const Texture &t : T.textures) tex.push_back(rxr_texture{t.data.data(), t.width, t.height});
    const int rc = rxr_set_terrain(ctx, T.scale, T.chunk_size, xy.data(), texture.data(), blend.data(), offset.data(), (uint32_t)texture.size(), tex.data(),
                                   (uint32_t)tex.size());
    if (rc != RXR_OK) {
        g_error = rxr_last_error(ctx);
        return rc;
    }
    g_terrain_gen = T.generation;
    return RXR_OK;
}
}  // namespace

int Terrain::bake_chunks(const int32_t *coords, uint32_t n, int32_t ppt, uint8_t *rgba) const {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    std::string err;
    rxr_ctx *ctx = context(&err);
    if (!ctx) return RXR_ERR_NO_DEVICE;
    if (const int rc = register_terrain(ctx, *this); rc != RXR_OK) return rc;
    const int rc = rxr_bake_terrain(ctx, coords, n, ppt, rgba);
    if (rc != RXR_OK) g_error = rxr_last_error(ctx);
    return rc;
}

int Terrain::build_chunk_at(int32_t cx, int32_t cy, int32_t ppt, Chunk &chunk) const {
    if (chunk_size < 1 || ppt < 1 || (int64_t)chunk_size * ppt > RXR_BAKE_MAX_DIM) {
        g_error = "Terrain::build_chunk_at: chunk_size and pixels_per_tile must be at least 1 and their product at most RXR_BAKE_MAX_DIM";
        return RXR_ERR_INVALID;
    }
    const uint32_t side = (uint32_t)(chunk_size * ppt);
    // (re-stamped on entry: where the call ends without assigning, a registration made again is the safe side)
    chunk.touch_textures();
    Texture baked;
    baked.width = baked.height = side;
    baked.data.resize((size_t)side * side * 4);
    const int32_t coord[2] = {cx, cy};
    const int rc = bake_chunks(coord, 1, ppt, baked.data.data());
    if (rc != RXR_OK) return rc;
    if (!chunks.count({cx, cy})) return RXR_OK;   // :383-391: baked, but the terrain has no chunk there: nothing is set
    chunk.terrain_texture = std::move(baked);
    chunk.has_terrain_texture = true;
    chunk.terrain_texture_stale = false;
    return RXR_OK;
}

// (rxr_api.hip; see Scene::rebuild_terrain_meshes)
extern "C" void *rxr_mirror_scratch(rxr_ctx *ctx, size_t bytes);
extern "C" int rxr_mirror_read(rxr_ctx *ctx, void *host, const void *dev, size_t bytes);

namespace {
// does the context hold the registration made from exactly these chunks' textures?
bool chunk_textures_current(const Scene &scene) {
    if (!g_ctex_held || g_ctex_gens.size() != scene.chunks.size()) return false;
    for (size_t c = 0; c < scene.chunks.size(); ++c)
        if (g_ctex_gens[c] != scene.chunks[c].textures_generation) return false;
    return true;
}
}  // namespace

int Scene::refresh_chunk_textures() {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    bool any = false;
    for (const Chunk &c : chunks) any = any || c.terrain_texture_stale;
    if (!any) return RXR_OK;
    std::string err;
    rxr_ctx *ctx = context(&err);
    if (!ctx) return RXR_ERR_NO_DEVICE;
    for (Chunk &c : chunks) {
        if (!c.terrain_texture_stale) continue;
        if (!g_ctex_held || c.slot_registration != g_ctex_registrations) {
            g_error = "Scene::refresh_chunk_textures: the context no longer holds this scene's chunk textures (another scene was uploaded): build the chunks again";
            return RXR_ERR_INVALID;
        }
        const int rc = rxr_read_chunk_texture(ctx, (uint32_t)c.terrain_slot, nullptr, nullptr, c.terrain_texture.data.data());
        if (rc != RXR_OK) {
            g_error = rxr_last_error(ctx);
            return rc;
        }
        c.terrain_texture_stale = false;
    }
    return RXR_OK;
}

int Terrain::rebuild_chunk_textures(Scene &scene, const int32_t *coords, uint32_t n, const uint32_t *chunks_, int32_t ppt) const {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    std::string err;
    rxr_ctx *ctx = context(&err);
    if (!ctx) return RXR_ERR_NO_DEVICE;
    if (!n) return 0;
    if (!coords || !chunks_) {
        g_error = "Terrain::rebuild_chunk_textures: NULL array";
        return RXR_ERR_INVALID;
    }
    if (chunk_size < 1 || ppt < 1 || (int64_t)chunk_size * ppt > RXR_BAKE_MAX_DIM) {
        g_error = "Terrain::rebuild_chunk_textures: chunk_size and pixels_per_tile must be at least 1 and their product at most RXR_BAKE_MAX_DIM";
        return RXR_ERR_INVALID;
    }
    for (uint32_t i = 0; i < n; ++i)
        if (chunks_[i] >= scene.chunks.size()) {
            g_error = "Terrain::rebuild_chunk_textures: chunks[" + std::to_string(i) + "] = " + std::to_string(chunks_[i]) + ": no such chunk";
            return RXR_ERR_INVALID;
        }
    const uint32_t side = (uint32_t)(chunk_size * ppt);
    bool fast = scene.resident_chunk_textures && rxr_member_count(ctx) == 1 && chunk_textures_current(scene);
    std::vector<uint32_t> slots(n);
    for (uint32_t i = 0; i < n && fast; ++i) {
        const Chunk &c = scene.chunks[chunks_[i]];
        fast = c.has_terrain_texture && c.terrain_slot >= 0 && c.terrain_texture.width == side && c.terrain_texture.height == side && this->chunks.count({coords[2 * i], coords[2 * i + 1]}) != 0;
        slots[i] = (uint32_t)c.terrain_slot;
    }
    if (fast) {
        int rc = register_terrain(ctx, *this);
        if (rc != RXR_OK) return rc;
        uint8_t *d = (uint8_t *)rxr_mirror_scratch(ctx, (size_t)n * side * side * 4);
        if (!d) {
            g_error = rxr_last_error(ctx);
            return RXR_ERR_OOM;
        }
        rc = rxr_bake_terrain_to(ctx, coords, n, ppt, d, nullptr);
        if (rc == RXR_OK) rc = rxr_update_chunk_textures_to(ctx, slots.data(), n, d, nullptr);   // (the same stream: the context's)
        if (rc == RXR_OK) {
            for (uint32_t i = 0; i < n; ++i) {   // the registration holds the new version: it stays current
                Chunk &c = scene.chunks[chunks_[i]];
                c.touch_textures();
                c.terrain_texture_stale = true;
                g_ctex_gens[chunks_[i]] = c.textures_generation;
            }
            return 0;
        }
        if (rc != RXR_ERR_INVALID) {
            g_error = rxr_last_error(ctx);
            return rc;
        }
        // refused (a chunk named twice): nothing was changed on the device
    }
    // the host copies that are rebuilt are not read back first; the others are, by the next upload's registration
    for (uint32_t i = 0; i < n; ++i) {
        const int rc = build_chunk_at(coords[2 * i], coords[2 * i + 1], ppt, scene.chunks[chunks_[i]]);
        if (rc != RXR_OK) return rc;
    }
    return 1;
}

// ---- heights and the editor's pick ----
void Terrain::set_height(int32_t x, int32_t y, float height) {
    heights[{x, y}] = height;
    chunks.insert({div_euclid(x, chunk_size), div_euclid(y, chunk_size)});
    heights_generation = next_generation();
}

void Terrain::remove_height(int32_t x, int32_t y) {
    // (the cell leaves the chunk's mesh; the chunk itself stays listed even when this was its last height)
    if (heights.erase({x, y})) heights_generation = next_generation();
}

void Terrain::flatten_heights(std::vector<int32_t> &xy, std::vector<float> &height) const {
    for (const auto &kv : heights) {
        xy.push_back(kv.first.first);
        xy.push_back(kv.first.second);
        height.push_back(kv.second);
    }
}

const Terrain::HeightGrid &Terrain::height_grid() const {
    HeightGrid &g = height_grid_;
    if (g.generation == heights_generation) return g;
    g = HeightGrid{};
    if (!heights.empty()) {
        int64_t lo[2] = {INT32_MAX, INT32_MAX}, hi[2] = {INT32_MIN, INT32_MIN};
        for (const auto &kv : heights) {
            lo[0] = std::min<int64_t>(lo[0], kv.first.first);
            hi[0] = std::max<int64_t>(hi[0], kv.first.first);
            lo[1] = std::min<int64_t>(lo[1], kv.first.second);
            hi[1] = std::max<int64_t>(hi[1], kv.first.second);
        }
        const int64_t w = hi[0] - lo[0] + 1, h = hi[1] - lo[1] + 1;
        if (w * h <= (int64_t)RXR_TERRAIN_MAX_CELLS) {   // (else w == 0: get_height reads the map)
            g.x0 = lo[0];
            g.y0 = lo[1];
            g.w = w;
            g.h = h;
            g.cells.assign((size_t)(w * h), 0.0f);
            for (const auto &kv : heights) g.cells[(size_t)((kv.first.second - lo[1]) * w + (kv.first.first - lo[0]))] = kv.second;
        }
    }
    g.generation = heights_generation;
    return g;
}

float Terrain::get_height(int32_t x, int32_t y) const {
    const HeightGrid &g = height_grid();
    if (g.w || heights.empty()) {
        const int64_t gx = (int64_t)x - g.x0, gy = (int64_t)y - g.y0;
        return (gx >= 0 && gy >= 0 && gx < g.w && gy < g.h) ? g.cells[(size_t)(gy * g.w + gx)] : 0.0f;
    }
    auto it = heights.find({x, y});
    return it == heights.end() ? 0.0f : it->second;
}

float Terrain::sample_height(float x, float y) const { return get_height(as_i32(std::round(x)), as_i32(std::round(y))); }

float Terrain::sample_height_bilinear(float x, float y) const {
    const int32_t x0 = as_i32(std::floor(x)), y0 = as_i32(std::floor(y));
    const int32_t x1 = (int32_t)((uint32_t)x0 + 1u), y1 = (int32_t)((uint32_t)y0 + 1u);   // (wraps, as a release build does)
    const float tx = x - (float)x0, ty = y - (float)y0;
    const float h00 = get_height(x0, y0), h10 = get_height(x1, y0), h01 = get_height(x0, y1), h11 = get_height(x1, y1);
    const float h0 = h00 * (1.0f - tx) + h10 * tx;
    const float h1 = h01 * (1.0f - tx) + h11 * tx;
    return h0 * (1.0f - ty) + h1 * ty;
}

bool Terrain::ray_terrain_hit(const float origin[3], const float dir[3], float max_distance, Hit &hit) const {
    const Vec3 o{origin[0], origin[1], origin[2]}, d{dir[0], dir[1], dir[2]};
    float t = 0.0f;
    const float step_size = 0.1f;
    for (int i = 0; i < (int)RXR_TERRAIN_MARCH_STEPS; ++i) {
        const Vec3 point = o + d * t;
        const float terrain_height = sample_height(point.x, point.z);
        if (point.y - terrain_height < 0.01f) {
            float low = std::fmax(t - step_size, 0.0f), high = t;
            for (int j = 0; j < 4; ++j) {
                const float mid = (low + high) * 0.5f;
                const Vec3 point_mid = o + d * mid;
                if (point_mid.y - sample_height_bilinear(point_mid.x, point_mid.z) < 0.01f) high = mid;
                else low = mid;
            }
            const float t_hit = (low + high) * 0.5f;
            const Vec3 hit_point = o + d * t_hit;
            const float terrain_hit_height = sample_height_bilinear(hit_point.x, hit_point.z);
            hit.t = t_hit;
            hit.world_pos[0] = hit_point.x;
            hit.world_pos[1] = terrain_hit_height;
            hit.world_pos[2] = hit_point.z;
            hit.grid_pos[0] = as_i32(std::floor(hit_point.x / scale[0]));
            hit.grid_pos[1] = as_i32(std::floor(hit_point.z / scale[1]));
            hit.height = terrain_hit_height;
            return true;
        }
        t += step_size;
        if (t > max_distance) break;
    }
    return false;
}

namespace {
void store_hit(bool found, const Terrain::Hit &h, size_t i, uint32_t *hit, float *t, float *world_pos, int32_t *grid_pos) {
    hit[i] = found ? 1u : 0u;
    if (t) t[i] = found ? h.t : FLT_MAX;
    for (int a = 0; a < 3; ++a)
        if (world_pos) world_pos[3 * i + a] = found ? h.world_pos[a] : 0.0f;
    for (int a = 0; a < 2; ++a)
        if (grid_pos) grid_pos[2 * i + a] = found ? h.grid_pos[a] : 0;
}
}  // namespace

void Terrain::ray_terrain_hits_cpu(const float *origins, const float *dirs, uint32_t n, float max_distance, uint32_t *hit, float *t, float *world_pos,
                                   int32_t *grid_pos) const {
    std::lock_guard<std::recursive_mutex> lk(g_mu);   // (the worker pool runs one job at a time)
    (void)height_grid();                              // (built once, before the workers read it)
    const size_t per = 256, items = ((size_t)n + per - 1) / per;
    rxr_parallel::run(items, (size_t)n * 1500, [&](size_t item) {
        for (size_t i = item * per; i < std::min<size_t>((item + 1) * per, n); ++i) {
            Hit h;
            const bool found = ray_terrain_hit(origins + 3 * i, dirs + 3 * i, max_distance, h);
            store_hit(found, h, i, hit, t, world_pos, grid_pos);
        }
    });
}

int Terrain::ray_terrain_hits(const float *origins, const float *dirs, uint32_t n, float max_distance, uint32_t *hit, float *t, float *world_pos,
                              int32_t *grid_pos) const {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    std::string err;
    rxr_ctx *ctx = context(&err);
    if (!ctx) return RXR_ERR_NO_DEVICE;
    int rc = register_heights(ctx);
    if (rc != RXR_OK) return rc;
    rc = rxr_terrain_hits(ctx, origins, dirs, n, max_distance, hit, t, world_pos, grid_pos);
    if (rc != RXR_OK) g_error = rxr_last_error(ctx);
    return rc;
}

int Terrain::register_heights(rxr_ctx *ctx) const {
    if (g_heights_gen == heights_generation) return RXR_OK;
    std::vector<int32_t> xy;
    std::vector<float> height;
    flatten_heights(xy, height);
    const int rc = rxr_set_terrain_heights(ctx, scale, xy.data(), height.data(), (uint32_t)height.size());
    if (rc != RXR_OK) {
        g_error = rxr_last_error(ctx);
        return rc;
    }
    g_heights_gen = heights_generation;
    g_processed_heights_gen = 0;   // (the registration reset the processed grid)
    ++g_heights_registrations;
    return RXR_OK;
}

// ---- the chunk mesh ----
Batch3D Terrain::build_mesh(int32_t cx, int32_t cy) const {
    std::vector<float> vertices, uvs;
    std::vector<uint32_t> indices;
    std::map<std::pair<int32_t, int32_t>, uint32_t> vertex_map;
    const int64_t ox = (int64_t)cx * chunk_size, oy = (int64_t)cy * chunk_size;
    for (int64_t ly = 0; ly < chunk_size; ++ly)
        for (int64_t lx = 0; lx < chunk_size; ++lx) {
            const int64_t wx = ox + lx, wy = oy + ly;
            if (wx < INT32_MIN || wx >= INT32_MAX || wy < INT32_MIN || wy >= INT32_MAX) continue;   // (no such key)
            if (!heights.count({(int32_t)wx, (int32_t)wy})) continue;
            uint32_t i[4];
            const int d[4][2] = {{0, 0}, {1, 0}, {0, 1}, {1, 1}};
            for (int k = 0; k < 4; ++k) {
                const int32_t px = (int32_t)wx + d[k][0], py = (int32_t)wy + d[k][1];
                auto it = vertex_map.find({px, py});
                if (it == vertex_map.end()) {
                    it = vertex_map.emplace(std::make_pair(px, py), (uint32_t)(vertices.size() / 4)).first;
                    const float v[4] = {(float)px * scale[0], get_height(px, py), (float)py * scale[1], 1.0f};
                    vertices.insert(vertices.end(), v, v + 4);
                    uvs.push_back(0.0f);
                    uvs.push_back(0.0f);
                }
                i[k] = it->second;
            }
            const uint32_t t[6] = {i[0], i[2], i[1], i[1], i[2], i[3]};
            indices.insert(indices.end(), t, t + 6);
        }
    Batch3D b = Batch3D::make(vertices.data(), vertices.size() / 4, indices.data(), indices.size() / 3, uvs.data());
    b.source_ = PixelSource::Terrain();
    b.compute_vertex_normals();
    return b;
}

void Terrain::build_meshes_cpu(const int32_t *coords, uint32_t n, std::vector<Batch3D> &out) const {
    std::lock_guard<std::recursive_mutex> lk(g_mu);   // (the worker pool runs one job at a time)
    (void)height_grid();                              // (built once, before the workers read it)
    out.assign(n, Batch3D());
    rxr_parallel::run(n, (size_t)n * chunk_size * chunk_size * 64, [&](size_t i) { out[i] = build_mesh(coords[2 * i], coords[2 * i + 1]); });
}

namespace {
// Terrain::device_modifiers: RXR_TERRAIN_HEIGHTS_PROCESSED for the length of a call (the choice is made when a launch is queued)
struct ProcessedSource {
    rxr_ctx *ctx;
    bool on;
    ProcessedSource(rxr_ctx *c, bool o) : ctx(c), on(o) {
        if (on) (void)rxr_set_terrain_height_source(ctx, RXR_TERRAIN_HEIGHTS_PROCESSED);
    }
    ~ProcessedSource() {
        if (on) (void)rxr_set_terrain_height_source(ctx, RXR_TERRAIN_HEIGHTS_REGISTERED);
    }
};
}  // namespace

int Terrain::build_meshes(const int32_t *coords, uint32_t n, std::vector<Batch3D> &out) const {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    std::string err;
    rxr_ctx *ctx = context(&err);
    if (!ctx) return RXR_ERR_NO_DEVICE;
    int rc = register_heights(ctx);
    if (rc != RXR_OK) return rc;
    out.clear();
    ProcessedSource processed(ctx, device_modifiers);   // (device_modifiers: the mesh kernels read the processed grid until this returns)
    if (device_modifiers && (rc = flatten_resident(ctx, coords, n)) != RXR_OK) return rc;
    if (chunk_size < 1 || chunk_size > RXR_TERRAIN_MESH_MAX_CHUNK_SIZE) {   // (the strides below need a size the library takes: its own answer)
        rc = rxr_terrain_meshes(ctx, coords, n, chunk_size, nullptr, nullptr, nullptr, nullptr);
        if (rc != RXR_OK) g_error = rxr_last_error(ctx);
        return rc;
    }
    const size_t VS = (size_t)(chunk_size + 1) * (chunk_size + 1), TS = 2 * (size_t)chunk_size * chunk_size;
    std::vector<uint32_t> counts(2 * (size_t)n), indices((size_t)n * TS * 3);
    std::vector<float> vertices((size_t)n * VS * 4), normals((size_t)n * VS * 3);
    rc = rxr_terrain_meshes(ctx, coords, n, chunk_size, counts.data(), vertices.data(), indices.data(), normals.data());
    if (rc != RXR_OK) {
        g_error = rxr_last_error(ctx);
        return rc;
    }
    out.reserve(n);
    for (uint32_t i = 0; i < n; ++i) {
        const size_t nv = counts[2 * (size_t)i], nt = counts[2 * (size_t)i + 1];
        const std::vector<float> uvs(nv * 2, 0.0f);   // all [0, 0] in the reference: they do not cross the ABI
        Batch3D b = Batch3D::make(vertices.data() + i * VS * 4, nv, indices.data() + i * TS * 3, nt, uvs.data());
        b.source_ = PixelSource::Terrain();
        b.normals.assign(normals.begin() + i * VS * 3, normals.begin() + i * VS * 3 + nv * 3);
        out.push_back(std::move(b));
    }
    return RXR_OK;
}

// ---- processed_heights: the Height pass of process_batch_modifiers ----
namespace {
// src/map/bbox.rs
struct BBox {
    float min_x, min_y, max_x, max_y;
    bool contains(float x, float y) const { return x >= min_x && x <= max_x && y >= min_y && y <= max_y; }
    bool intersects(const BBox &o) const { return min_x <= o.max_x && max_x >= o.min_x && min_y <= o.max_y && max_y >= o.min_y; }
    BBox expanded(float amount) const { return BBox{min_x - amount * 0.5f, min_y - amount * 0.5f, max_x + amount * 0.5f, max_y + amount * 0.5f}; }
};
// f32::clamp(0.0, 1.0): a NaN stays
float flat_clamp01(float t) {
    if (t < 0.0f) t = 0.0f;
    if (t > 1.0f) t = 1.0f;
    return t;
}
// ShapeFX::smoothstep (src/shapestack/shapefx.rs:2258-2261)
float flat_smoothstep(float edge0, float edge1, float x) {
    const float t = flat_clamp01((x - edge0) / (edge1 - edge0));
    return t * t * (3.0f - 2.0f * t);
}
float flat_magnitude(float x, float y) { return std::sqrt(x * x + y * y); }

// Sector::signed_distance (src/map/sector.rs:308-333) with is_inside (:272-305) over the op's edges
float flat_signed_distance(const Terrain::FlattenOp &op, float px, float py) {
    const size_t n = op.records.size() / RXR_TERRAIN_FLATTEN_RECORD_FLOATS;
    float min_dist = std::numeric_limits<float>::max();
    for (size_t i = 0; i < n; ++i) {
        const float *r = op.records.data() + RXR_TERRAIN_FLATTEN_RECORD_FLOATS * i;
        const float ex = r[2] - r[0], ey = r[3] - r[1];
        const float tx = px - r[0], ty = py - r[1];
        const float t = (tx * ex + ty * ey) / (ex * ex + ey * ey);
        const float t_clamped = flat_clamp01(t);
        const float cx = r[0] + ex * t_clamped, cy = r[1] + ey * t_clamped;
        const float dist = flat_magnitude(px - cx, py - cy);
        min_dist = std::fmin(min_dist, dist);   // f32::min drops a NaN operand
    }
    bool inside = false;
    if (n >= 3) {
        size_t j = n - 1;
        for (size_t i = 0; i < n; ++i) {
            const float *pi = op.records.data() + RXR_TERRAIN_FLATTEN_RECORD_FLOATS * i, *pj = op.records.data() + RXR_TERRAIN_FLATTEN_RECORD_FLOATS * j;
            if ((pi[1] > py) != (pj[1] > py) && px < (pj[0] - pi[0]) * (py - pi[1]) / (pj[1] - pi[1]) + pi[0]) inside = !inside;
            j = i;
        }
    }
    return inside ? -min_dist : min_dist;
}
}  // namespace

int Terrain::set_flatten_ops(const uint32_t *kinds, const float *params, const uint32_t *ranges, uint32_t n_ops, const float *records, uint32_t n_records) {
    char message[256] = "";
    const int rc = rxr_check_terrain_flatten(kinds, params, ranges, n_ops, records, n_records, message, sizeof message);
    if (rc != RXR_OK) {
        std::lock_guard<std::recursive_mutex> lk(g_mu);
        g_error = std::string("Terrain::set_flatten_ops: ") + message;
        return rc;
    }
    flatten_ops.assign(n_ops, FlattenOp());
    for (uint32_t i = 0; i < n_ops; ++i) {
        FlattenOp &op = flatten_ops[i];
        const float *p = params + RXR_TERRAIN_FLATTEN_OP_FLOATS * (size_t)i;
        op.kind = kinds[i];
        op.bevel = p[0], op.floor_height = p[1];
        for (int k = 0; k < 4; ++k) op.box[k] = p[2 + k];
        const float *r = records + RXR_TERRAIN_FLATTEN_RECORD_FLOATS * (size_t)ranges[2 * (size_t)i];
        op.records.assign(r, r + RXR_TERRAIN_FLATTEN_RECORD_FLOATS * (size_t)ranges[2 * (size_t)i + 1]);
    }
    touch_flatten();
    return RXR_OK;
}

void Terrain::flatten_op_arrays(std::vector<uint32_t> &kinds, std::vector<float> &params, std::vector<uint32_t> &ranges, std::vector<float> &records) const {
    for (const FlattenOp &op : flatten_ops) {
        kinds.push_back(op.kind);
        const float p[RXR_TERRAIN_FLATTEN_OP_FLOATS] = {op.bevel, op.floor_height, op.box[0], op.box[1], op.box[2], op.box[3]};
        params.insert(params.end(), p, p + RXR_TERRAIN_FLATTEN_OP_FLOATS);
        ranges.push_back((uint32_t)(records.size() / RXR_TERRAIN_FLATTEN_RECORD_FLOATS));
        ranges.push_back((uint32_t)(op.records.size() / RXR_TERRAIN_FLATTEN_RECORD_FLOATS));
        records.insert(records.end(), op.records.begin(), op.records.end());
    }
}

void Terrain::process_chunk_cpu(int32_t cx, int32_t cy, std::map<std::pair<int32_t, int32_t>, float> &processed) const {
    const int64_t ox = (int64_t)cx * chunk_size, oy = (int64_t)cy * chunk_size;
    // let mut processed_heights = self.heights.clone() -- keyed by local cell
    for (auto it = heights.lower_bound({(int32_t)std::max<int64_t>(ox, INT32_MIN), INT32_MIN}); it != heights.end() && it->first.first < ox + chunk_size; ++it)
        if (it->first.second >= oy && it->first.second < oy + chunk_size) processed[{(int32_t)(it->first.first - ox), (int32_t)(it->first.second - oy)}] = it->second;
    auto unprocessed = [&](int64_t x, int64_t y, float &h) {   // terrain.get_height_unprocessed
        if (x < INT32_MIN || x > INT32_MAX || y < INT32_MIN || y > INT32_MAX) return false;
        auto it = heights.find({(int32_t)x, (int32_t)y});
        if (it == heights.end()) return false;
        h = it->second;
        return true;
    };
    // TerrainChunk::bounds (:130-134)
    const float size_f = (float)chunk_size - 1.0f;
    const BBox bbox{(float)ox, (float)oy, (float)ox + size_f, (float)oy + size_f};
    for (const FlattenOp &op : flatten_ops) {
        const float bevel = op.bevel;
        const size_t n_records = op.records.size() / RXR_TERRAIN_FLATTEN_RECORD_FLOATS;
        if (op.kind == RXR_TERRAIN_FLATTEN_SECTOR) {
            const BBox sector_box{op.box[0], op.box[1], op.box[2], op.box[3]};
            if (!bbox.intersects(sector_box.expanded(2.0f))) continue;
            // ShapeFX::sector_modify_heightmap (src/shapestack/shapefx.rs:414-478), the Height pass
            const float floor_height = op.floor_height;
            const BBox expanded_bbox = bbox.expanded(bevel);
            const BBox chunk_bbox = bbox;
            const BBox bounds = sector_box.expanded(bevel);
            int64_t min_x = as_i32(std::floor(bounds.min_x)), max_x = as_i32(std::ceil(bounds.max_x));
            int64_t min_y = as_i32(std::floor(bounds.min_y)), max_y = as_i32(std::ceil(bounds.max_y));
            // (the clip the header states: no cell farther than this from the chunk passes chunk_bbox.contains)
            min_x = std::max(min_x, ox - 130), max_x = std::min(max_x, ox + chunk_size + 130);
            min_y = std::max(min_y, oy - 130), max_y = std::min(max_y, oy + chunk_size + 130);
            for (int64_t y = min_y; y <= max_y; ++y)
                for (int64_t x = min_x; x <= max_x; ++x) {
                    const float px = (float)x, py = (float)y;
                    if (!expanded_bbox.contains(px, py)) continue;
                    const float sd = flat_signed_distance(op, px, py);
                    if (sd < bevel * 4.0f) {
                        const float s = flat_smoothstep(0.0f, bevel, bevel - sd);
                        float original;
                        if (!unprocessed(x, y, original)) original = floor_height;
                        const float new_height = original * (1.0f - s) + floor_height * s;
                        if (chunk_bbox.contains((float)x, (float)y)) processed[{(int32_t)(x - ox), (int32_t)(y - oy)}] = new_height;
                    }
                }
        } else {
            // the group's linedefs whose bounding_box.expanded(2.0) intersects the chunk (:181-191), then linedef_modify_heightmap (:682-820)
            std::vector<const float *> segments;
            for (size_t i = 0; i < n_records; ++i) {
                const float *r = op.records.data() + RXR_TERRAIN_FLATTEN_RECORD_FLOATS * i;
                if (bbox.intersects(BBox{r[6], r[7], r[8], r[9]}.expanded(2.0f))) segments.push_back(r);
            }
            if (segments.empty()) continue;
            const BBox chunk_bbox = bbox;
            const float min_fx = bbox.min_x - bevel * scale[0], min_fy = bbox.min_y - bevel * scale[1];
            const float max_fx = bbox.max_x + bevel * scale[0], max_fy = bbox.max_y + bevel * scale[1];
            const int64_t tile_min_x = as_i32(std::floor(min_fx / scale[0])), tile_min_y = as_i32(std::floor(min_fy / scale[1]));
            const int64_t tile_max_x = as_i32(std::ceil(max_fx / scale[0])), tile_max_y = as_i32(std::ceil(max_fy / scale[1]));
            for (int64_t ty = tile_min_y; ty < tile_max_y; ++ty)
                for (int64_t tx = tile_min_x; tx < tile_max_x; ++tx) {
                    const float center_x = ((float)tx + 0.5f) * scale[0], center_y = ((float)ty + 0.5f) * scale[1];
                    // closest_segment (:721-738) over point_to_line_segment (:711-719)
                    const float *seg = nullptr;
                    float best_dist = 0.0f, best_t = 0.0f;
                    for (const float *r : segments) {
                        const float abx = r[2] - r[0], aby = r[3] - r[1];
                        const float apx = center_x - r[0], apy = center_y - r[1];
                        const float t = (apx * abx + apy * aby) / (abx * abx + aby * aby);
                        const float t_clamped = flat_clamp01(t);
                        const float qx = r[0] + abx * t_clamped, qy = r[1] + aby * t_clamped;
                        const float dist = flat_magnitude(center_x - qx, center_y - qy);
                        if (!seg || dist < best_dist) seg = r, best_dist = dist, best_t = t_clamped;
                    }
                    if (best_dist > bevel) continue;
                    const float height = seg[4] * (1.0f - best_t) + seg[5] * best_t;
                    const float blend = flat_smoothstep(0.0f, bevel, bevel - best_dist);
                    if (chunk_bbox.contains((float)tx, (float)ty)) {
                        float original;
                        if (!unprocessed(tx, ty, original)) original = height;
                        processed[{(int32_t)(tx - ox), (int32_t)(ty - oy)}] = original * (1.0f - blend) + height * blend;
                    }
                }
        }
    }
}

void Terrain::process_heights_cpu(const int32_t *coords, uint32_t n, float *out_heights, uint8_t *out_present) const {
    std::lock_guard<std::recursive_mutex> lk(g_mu);   // (the worker pool runs one job at a time)
    if (chunk_size < 1) return;
    const size_t per = (size_t)chunk_size * (size_t)chunk_size;
    rxr_parallel::run(n, (size_t)n * per * 64 * std::max<size_t>(flatten_ops.size(), 1), [&](size_t i) {
        std::map<std::pair<int32_t, int32_t>, float> processed;
        process_chunk_cpu(coords[2 * i], coords[2 * i + 1], processed);
        if (out_heights) std::fill(out_heights + i * per, out_heights + (i + 1) * per, 0.0f);
        if (out_present) std::fill(out_present + i * per, out_present + (i + 1) * per, (uint8_t)0);
        for (const auto &kv : processed) {
            const int32_t lx = kv.first.first, ly = kv.first.second;
            if (lx < 0 || ly < 0 || lx >= chunk_size || ly >= chunk_size) continue;   // (a neighbour's cell, beyond +-2^24: include/rxr.h)
            if (out_heights) out_heights[i * per + (size_t)ly * chunk_size + lx] = kv.second;
            if (out_present) out_present[i * per + (size_t)ly * chunk_size + lx] = 1;
        }
    });
}

int Terrain::register_flatten(rxr_ctx *ctx) const {
    if (g_flatten_gen == flatten_generation) return RXR_OK;
    std::vector<uint32_t> kinds, ranges;
    std::vector<float> params, records;
    flatten_op_arrays(kinds, params, ranges, records);
    const int rc = rxr_set_terrain_flatten(ctx, kinds.data(), params.data(), ranges.data(), (uint32_t)kinds.size(), records.data(),
                                           (uint32_t)(records.size() / RXR_TERRAIN_FLATTEN_RECORD_FLOATS));
    if (rc != RXR_OK) {
        g_error = rxr_last_error(ctx);
        return rc;
    }
    g_flatten_gen = flatten_generation;
    ++g_flatten_registrations;
    return RXR_OK;
}

int Terrain::process_heights(const int32_t *coords, uint32_t n, float *out_heights, uint8_t *out_present) const {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    std::string err;
    rxr_ctx *ctx = context(&err);
    if (!ctx) return RXR_ERR_NO_DEVICE;
    int rc = register_heights(ctx);
    if (rc == RXR_OK) rc = register_flatten(ctx);
    if (rc != RXR_OK) return rc;
    rc = rxr_flatten_terrain(ctx, coords, n, chunk_size, out_heights, out_present);
    if (rc != RXR_OK) g_error = rxr_last_error(ctx);
    return rc;
}

int Terrain::flatten_resident(rxr_ctx *ctx, const int32_t *coords, uint32_t n) const {
    int rc = register_heights(ctx);
    if (rc == RXR_OK) rc = register_flatten(ctx);
    if (rc != RXR_OK) return rc;
    std::vector<int32_t> all;
    if (g_processed_heights_gen != heights_generation || g_processed_flatten_gen != flatten_generation) {
        // a registration reset the processed grid, or the ops changed: every chunk of the terrain, the named ones among them
        std::set<std::pair<int32_t, int32_t>> every(chunks);
        for (uint32_t i = 0; i < n; ++i) every.insert({coords[2 * (size_t)i], coords[2 * (size_t)i + 1]});
        for (const auto &c : every) {
            bool fits = true;
            for (const int32_t v : {c.first, c.second}) {
                const int64_t lo = (int64_t)v * chunk_size;
                fits = fits && lo >= -(1ll << 30) && lo + chunk_size - 1 <= (1ll << 30);
            }
            if (fits) all.push_back(c.first), all.push_back(c.second);
        }
        coords = all.data();
        n = (uint32_t)(all.size() / 2);
    }
    rc = rxr_flatten_terrain_to(ctx, coords, n, chunk_size, nullptr, nullptr, nullptr);   // (the context's stream)
    if (rc != RXR_OK) {
        g_error = rxr_last_error(ctx);
        return rc;
    }
    g_processed_heights_gen = heights_generation;
    g_processed_flatten_gen = flatten_generation;
    return RXR_OK;
}

// (rxr_api.hip; not part of include/rxr.h: this mirror links no HIP runtime, so its device scratch comes from the device library -- a
// host with an allocator of its own hands rxr_terrain_meshes_to / rxr_update_meshes_to its own memory)
extern "C" void *rxr_mirror_scratch(rxr_ctx *ctx, size_t bytes);

int Scene::rebuild_terrain_meshes(const Terrain &terrain, const int32_t *coords, uint32_t n, const uint32_t *chunks_) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    std::string err;
    rxr_ctx *ctx = context(&err);
    if (!ctx) return RXR_ERR_NO_DEVICE;
    if (!g_device_projection) {
        g_error = "Scene::rebuild_terrain_meshes: device projection is off (set_device_projection): there are no registered meshes to update";
        return RXR_ERR_UNSUPPORTED;
    }
    if (!n) return 0;
    if (!coords || !chunks_) {
        g_error = "Scene::rebuild_terrain_meshes: NULL array";
        return RXR_ERR_INVALID;
    }
    // each batch's position in batches3d_in_order(): per chunk opacity, batches, terrain
    std::vector<uint32_t> first_of_chunk(chunks.size() + 1, 0);
    for (size_t c = 0; c < chunks.size(); ++c)
        first_of_chunk[c + 1] = first_of_chunk[c] + (uint32_t)(chunks[c].batches3d_opacity.size() + chunks[c].batches3d.size() + chunks[c].terrain_batch3d.size());
    std::vector<uint32_t> mesh_index(n);
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t c = chunks_[i];
        if (c >= chunks.size() || chunks[c].terrain_batch3d.size() != 1) {
            g_error = "Scene::rebuild_terrain_meshes: chunks[" + std::to_string(i) + "] = " + std::to_string(c) + " is not a chunk with one terrain_batch3d";
            return RXR_ERR_INVALID;
        }
        mesh_index[i] = first_of_chunk[c + 1] - 1u;
    }
    const int32_t cs = terrain.chunk_size;
    std::vector<rxr_mesh3d> meshes;
    uint64_t full = 0, geometry = 0;
    // the fast path needs a registration made by a device-projected upload (sources resolved) of exactly this geometry; one made by
    // Scene::intersect alone is registered again by the next upload, from the host arrays
    const bool held = scene_meshes(*this, nullptr, meshes, nullptr, full, geometry) && g_mesh_fingerprint != 0 && geometry == g_mesh_geometry_fingerprint;
    if (held && rxr_member_count(ctx) == 1 && cs >= 1 && cs <= RXR_TERRAIN_MESH_MAX_CHUNK_SIZE) {
        int rc = terrain.register_heights(ctx);
        if (rc != RXR_OK) return rc;
        // device_modifiers: flatten -> meshes (with their normals) -> update, one after the other on the context's stream
        ProcessedSource processed(ctx, terrain.device_modifiers);
        if (terrain.device_modifiers && (rc = terrain.flatten_resident(ctx, coords, n)) != RXR_OK) return rc;
        const size_t VS = (size_t)(cs + 1) * (cs + 1), TS = 2 * (size_t)cs * cs;
        auto up = [](size_t x) { return (x + 255) / 256 * 256; };
        const size_t o_v = up((size_t)n * 8), o_i = o_v + up((size_t)n * VS * 16), o_n = o_i + up((size_t)n * TS * 12), total = o_n + up((size_t)n * VS * 12);
        uint8_t *d = (uint8_t *)rxr_mirror_scratch(ctx, total);
        if (!d) {
            g_error = rxr_last_error(ctx);
            return RXR_ERR_OOM;
        }
        uint32_t *dc = (uint32_t *)d, *di = (uint32_t *)(d + o_i);
        float *dv = (float *)(d + o_v), *dn = (float *)(d + o_n);
        rc = rxr_terrain_meshes_to(ctx, coords, n, cs, dc, dv, di, dn, nullptr);
        if (rc == RXR_OK) rc = rxr_update_meshes_to(ctx, mesh_index.data(), n, dc, dv, di, dn, (uint32_t)VS, (uint32_t)TS, nullptr);   // (the same stream: the context's)
        if (rc == RXR_OK) return 0;
        if (rc != RXR_ERR_INVALID) {
            g_error = rxr_last_error(ctx);
            return rc;
        }
        // refused (counts changed): nothing was changed on the device
        if (resize_meshes) {
            // the same arrays on the same stream, uvs absent (TerrainChunk::build_mesh's are [0, 0]); the counts come back for the batches
            std::vector<uint32_t> got(2 * (size_t)n);
            rc = rxr_resize_meshes_to(ctx, mesh_index.data(), n, dc, dv, nullptr, di, dn, (uint32_t)VS, (uint32_t)TS, nullptr);
            if (rc == RXR_OK) rc = rxr_mirror_read(ctx, got.data(), dc, got.size() * sizeof(uint32_t));
            if (rc != RXR_OK) {
                g_error = rxr_last_error(ctx);
                return rc;
            }
            for (uint32_t i = 0; i < n; ++i) adopt_counts(chunks[chunks_[i]].terrain_batch3d[0], got[2 * (size_t)i], got[2 * (size_t)i + 1]);
            refingerprint_meshes(*this);
            return 2;
        }
    }
    std::vector<Batch3D> built;
    const int rc = terrain.build_meshes(coords, n, built);
    if (rc != RXR_OK) return rc;
    for (uint32_t i = 0; i < n; ++i) {
        Batch3D &b = chunks[chunks_[i]].terrain_batch3d[0];   // (material, transform and cull mode stay the batch's own)
        b.vertices = std::move(built[i].vertices);
        b.indices = std::move(built[i].indices);
        b.uvs = std::move(built[i].uvs);
        b.normals = std::move(built[i].normals);
        b.touch();
    }
    return 1;
}

int Scene::rebuild_generated_tile_meshes(const TerrainGenerator &gen, const float *boxes, uint32_t n, const uint32_t *chunks_, uint32_t max_groups) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    const std::string who = "Scene::rebuild_generated_tile_meshes: ";
    std::string err;
    rxr_ctx *ctx = context(&err);
    if (!ctx) return RXR_ERR_NO_DEVICE;
    if (!g_device_projection) {
        g_error = who + "device projection is off (set_device_projection): there are no registered meshes to update";
        return RXR_ERR_UNSUPPORTED;
    }
    if (!n) return 0;
    if (!boxes || !chunks_ || !max_groups) {
        g_error = who + "NULL array or max_groups == 0";
        return RXR_ERR_INVALID;
    }
    // each batch's position in batches3d_in_order(): per chunk opacity, batches, terrain; a named chunk's `batches3d` are its tile
    // groups in ascending slot (terrain_batch3d is the reference's Option<Batch3D>: it holds one batch)
    std::vector<uint32_t> first_of_chunk(chunks.size() + 1, 0);
    for (size_t c = 0; c < chunks.size(); ++c)
        first_of_chunk[c + 1] = first_of_chunk[c] + (uint32_t)(chunks[c].batches3d_opacity.size() + chunks[c].batches3d.size() + chunks[c].terrain_batch3d.size());
    bool all_full = true;
    size_t VS = 0, TS = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t c = chunks_[i];
        if (c >= chunks.size() || chunks[c].batches3d.size() > max_groups) {
            g_error = who + "chunks[" + std::to_string(i) + "] = " + std::to_string(c) + " is not a chunk with at most max_groups batches3d";
            return RXR_ERR_INVALID;
        }
        all_full = all_full && chunks[c].batches3d.size() == max_groups;
        int32_t sx, sy;
        gen.grid_steps(boxes + 4 * (size_t)i, sx, sy);
        const size_t points = (sx > 0 && sy > 0) ? (size_t)sx * (size_t)sy : 0, cells = (sx > 1 && sy > 1) ? (size_t)(sx - 1) * (size_t)(sy - 1) : 0;
        VS = std::max(VS, std::max(points, 6 * cells)), TS = std::max(TS, 2 * cells);
    }
    if (VS > 0xFFFFFFFFull || TS > 0xFFFFFFFFull) {
        g_error = who + "a box has more vertices or triangles than the device call counts";
        return RXR_ERR_INVALID;
    }
    const size_t M = (size_t)n * max_groups;
    std::vector<rxr_mesh3d> meshes;
    uint64_t full = 0, geometry = 0;
    // the fast path needs a registration made by a device-projected upload of exactly this geometry (rebuild_terrain_meshes)
    const bool held = scene_meshes(*this, nullptr, meshes, nullptr, full, geometry) && g_mesh_fingerprint != 0 && geometry == g_mesh_geometry_fingerprint;
    if (held && rxr_member_count(ctx) == 1) {
        int rc = gen.register_records(ctx);
        if (rc != RXR_OK || (rc = gen.register_exclusions(ctx)) != RXR_OK || (rc = gen.register_tiles(ctx)) != RXR_OK) return rc;
        auto up = [](size_t x) { return (x + 255) / 256 * 256; };
        const size_t o_c = up((size_t)n * 16), o_g = o_c + up(M * 8), o_v = o_g + up(M * 4), o_u = o_v + up(M * VS * 16), o_i = o_u + up(M * VS * 8), o_n = o_i + up(M * TS * 12),
                     total = o_n + up(M * VS * 12);
        uint8_t *d = (uint8_t *)rxr_mirror_scratch(ctx, total);
        if (!d) {
            g_error = rxr_last_error(ctx);
            return RXR_ERR_OOM;
        }
        uint32_t *db = (uint32_t *)d, *dc = (uint32_t *)(d + o_c), *dg = (uint32_t *)(d + o_g), *di = (uint32_t *)(d + o_i);
        float *dv = (float *)(d + o_v), *du = (float *)(d + o_u), *dn = (float *)(d + o_n);
        // one stream (the context's): tile meshes -> vertex normals -> update; no geometry crosses PCIe
        rc = rxr_generated_tile_meshes_to(ctx, boxes, n, gen.subdivisions, max_groups, (uint32_t)VS, (uint32_t)TS, db, dc, dg, dv, du, di, nullptr);
        // box_counts and counts come back (16 bytes a box, 8 a mesh slot) and are held against the chunks' batches BEFORE anything is
        // written over a registered mesh: a chunk whose number of groups changed is refused here, and counts that changed send the
        // whole call to the host path with nothing committed
        std::vector<uint32_t> got(o_g / 4);
        if (rc == RXR_OK) rc = rxr_mirror_read(ctx, got.data(), d, o_g);
        if (rc != RXR_OK) {
            g_error = rxr_last_error(ctx);
            return rc;
        }
        bool same_counts = true;
        for (uint32_t i = 0; i < n; ++i) {
            const Chunk &c = chunks[chunks_[i]];
            const uint32_t n_groups = got[4 * (size_t)i + 3];
            if (n_groups != c.batches3d.size()) {
                g_error = who + "chunks[" + std::to_string(i) + "] has " + std::to_string(c.batches3d.size()) + " batches3d and its box " + std::to_string(n_groups) +
                          " tile groups: which tile a new batch shows is the caller's to say";
                return RXR_ERR_INVALID;
            }
            for (size_t g = 0; g < c.batches3d.size(); ++g) {
                const uint32_t *mc = got.data() + o_c / 4 + 2 * ((size_t)i * max_groups + g);
                same_counts = same_counts && mc[0] == c.batches3d[g].vertex_count() && mc[1] == c.batches3d[g].triangle_count();
            }
        }
        const bool resize = !same_counts && resize_meshes;   // (Scene::resize_meshes: counts that changed are resized on the device)
        if (same_counts || resize) rc = rxr_vertex_normals_to(ctx, (uint32_t)M, dc, dv, di, dn, nullptr, (uint32_t)VS, (uint32_t)TS, nullptr);
        if (rc != RXR_OK) {
            g_error = rxr_last_error(ctx);
            return rc;
        }
        if (!same_counts && !resize) rc = RXR_ERR_INVALID;   // (the host path below)
        // a chunk's registered meshes are its groups; a chunk with fewer than max_groups of them leaves mesh slots no mesh answers to,
        // so the update is one call when every chunk is full and one call per chunk otherwise
        std::vector<uint32_t> mesh_index;
        for (uint32_t i = 0; i < n && rc == RXR_OK; ++i) {
            const Chunk &c = chunks[chunks_[i]];
            for (size_t g = 0; g < c.batches3d.size(); ++g) mesh_index.push_back(first_of_chunk[chunks_[i]] + (uint32_t)c.batches3d_opacity.size() + (uint32_t)g);
            if (all_full && i + 1 < n) continue;
            const size_t m0 = all_full ? 0 : (size_t)i * max_groups;
            if (!mesh_index.empty())
                rc = resize ? rxr_resize_meshes_to(ctx, mesh_index.data(), (uint32_t)mesh_index.size(), dc + 2 * m0, dv + m0 * VS * 4, du + m0 * VS * 2, di + m0 * TS * 3,
                                                   dn + m0 * VS * 3, (uint32_t)VS, (uint32_t)TS, nullptr)
                            : rxr_update_meshes_to(ctx, mesh_index.data(), (uint32_t)mesh_index.size(), dc + 2 * m0, dv + m0 * VS * 4, di + m0 * TS * 3, dn + m0 * VS * 3,
                                                   (uint32_t)VS, (uint32_t)TS, nullptr);
            mesh_index.clear();
        }
        if (resize) {
            if (rc != RXR_OK) {   // (a call of several may have gone through: the next upload registers again)
                g_error = rxr_last_error(ctx);
                g_mesh_fingerprint = g_mesh_geometry_fingerprint = 0;
                return rc;
            }
            for (uint32_t i = 0; i < n; ++i) {
                Chunk &c = chunks[chunks_[i]];
                for (size_t g = 0; g < c.batches3d.size(); ++g) {
                    const uint32_t *mc = got.data() + o_c / 4 + 2 * ((size_t)i * max_groups + g);
                    adopt_counts(c.batches3d[g], mc[0], mc[1]);
                }
            }
            refingerprint_meshes(*this);
            return 2;
        }
        if (rc == RXR_OK) return 0;
        if (rc != RXR_ERR_INVALID) {
            g_error = rxr_last_error(ctx);
            return rc;
        }
        // refused (counts changed): the host path below replaces every named chunk's batches, and the next upload registers them again
    }
    std::vector<uint32_t> box_counts(4 * (size_t)n), counts(2 * M), group_tiles(M), indices(M * TS * 3);
    std::vector<float> vertices(M * VS * 4), uvs(M * VS * 2);
    gen.generate_tile_meshes_cpu(boxes, n, max_groups, (uint32_t)VS, (uint32_t)TS, box_counts.data(), counts.data(), group_tiles.data(), vertices.data(), uvs.data(), indices.data());
    for (uint32_t i = 0; i < n; ++i)
        if (box_counts[4 * (size_t)i + 3] != chunks[chunks_[i]].batches3d.size()) {
            g_error = who + "chunks[" + std::to_string(i) + "] has " + std::to_string(chunks[chunks_[i]].batches3d.size()) + " batches3d and its box " +
                      std::to_string(box_counts[4 * (size_t)i + 3]) + " tile groups (or more than max_groups): which tile a new batch shows is the caller's to say";
            return RXR_ERR_INVALID;
        }
    for (uint32_t i = 0; i < n; ++i)
        for (size_t g = 0; g < chunks[chunks_[i]].batches3d.size(); ++g) {
            Batch3D &b = chunks[chunks_[i]].batches3d[g];   // (material, transform and cull mode stay the batch's own)
            const size_t m = (size_t)i * max_groups + g, nv = counts[2 * m], nt = counts[2 * m + 1];
            b.vertices.assign(vertices.begin() + m * VS * 4, vertices.begin() + (m * VS + nv) * 4);
            b.uvs.assign(uvs.begin() + m * VS * 2, uvs.begin() + (m * VS + nv) * 2);
            b.indices.assign(indices.begin() + m * TS * 3, indices.begin() + (m * TS + nt) * 3);
            b.compute_vertex_normals();
            b.touch();
        }
    return 1;
}

int Scene::compute_normals(std::vector<Batch3D> &batches, int route) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);   // (the worker pool runs one job at a time)
    const size_t n = batches.size();
    if (route == NORMALS_CPU) {
        for (Batch3D &b : batches) b.compute_vertex_normals();
        return RXR_OK;
    }
    if (route == NORMALS_POOL) {
        size_t work = 0;
        for (const Batch3D &b : batches) work += b.triangle_count() * 64 + b.vertex_count() * 32;
        rxr_parallel::run(n, work, [&](size_t i) { batches[i].compute_vertex_normals(); });
        return RXR_OK;
    }
    if (route != NORMALS_DEVICE) {
        g_error = "Scene::compute_normals: no such route";
        return RXR_ERR_INVALID;
    }
    std::string err;
    rxr_ctx *ctx = context(&err);
    if (!ctx) return RXR_ERR_NO_DEVICE;
    if (!n) return RXR_OK;
    size_t VS = 0, TS = 0;
    for (const Batch3D &b : batches) VS = std::max(VS, b.vertex_count()), TS = std::max(TS, b.triangle_count());
    if (n > 0xFFFFFFFFull || VS > 0xFFFFFFFFull || TS > 0xFFFFFFFFull) {
        g_error = "Scene::compute_normals: more batches, vertices or triangles than the device call counts";
        return RXR_ERR_INVALID;
    }
    std::vector<uint32_t> counts(2 * n), indices(n * TS * 3, 0u);
    std::vector<float> vertices(n * VS * 4, 0.0f), normals(n * VS * 3, 0.0f);
    for (size_t i = 0; i < n; ++i) {
        const Batch3D &b = batches[i];
        counts[2 * i] = (uint32_t)b.vertex_count();
        counts[2 * i + 1] = (uint32_t)b.triangle_count();
        std::copy(b.vertices.begin(), b.vertices.begin() + b.vertex_count() * 4, vertices.begin() + i * VS * 4);
        std::copy(b.indices.begin(), b.indices.begin() + b.triangle_count() * 3, indices.begin() + i * TS * 3);
    }
    const int rc = rxr_vertex_normals(ctx, (uint32_t)n, counts.data(), vertices.data(), indices.data(), normals.data(), (uint32_t)VS, (uint32_t)TS);
    if (rc != RXR_OK) {
        g_error = rxr_last_error(ctx);
        return rc;
    }
    for (size_t i = 0; i < n; ++i) {
        Batch3D &b = batches[i];
        b.normals.assign(normals.begin() + i * VS * 3, normals.begin() + i * VS * 3 + b.vertex_count() * 3);
        b.touch();
    }
    return RXR_OK;
}

void Rasterizer::screen_ray(float x, float y, float origin[3], float dir[3]) const {
    const float ndc_x = 2.0f * (x / width) - 1.0f;
    const float ndc_y = 1.0f - 2.0f * (y / height);  // flip y
    Vec4 view_near = inverse_projection_matrix * Vec4{ndc_x, ndc_y, -1.0f, 1.0f};
    Vec4 view_far = inverse_projection_matrix * Vec4{ndc_x, ndc_y, 1.0f, 1.0f};
    view_near = view_near / view_near.w;
    view_far = view_far / view_far.w;
    const Vec4 world_near = inverse_view_matrix * view_near, world_far = inverse_view_matrix * view_far;
    const Vec3 o{world_near.x, world_near.y, world_near.z}, target{world_far.x, world_far.y, world_far.z};
    const Vec3 d = rvek::normalized(target - o);
    origin[0] = o.x, origin[1] = o.y, origin[2] = o.z;
    dir[0] = d.x, dir[1] = d.y, dir[2] = d.z;
}

int Rasterizer::upload(Scene &scene, size_t w, size_t h, size_t tile_size, const Assets &assets) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    std::string err;
    rxr_ctx *ctx = context(&err);
    if (!ctx) return RXR_ERR_NO_DEVICE;

    width = (float)w;
    height = (float)h;
    hash_anim = hash_u32((uint32_t)scene.animation_frame);  // :208

    const bool on_device = g_device_projection;
    t_frame_edgeless = g_device_edges;
    if (on_device) {
        // both halves of Scene::project run on the GPU (rxr_set_meshes / rxr_set_meshes2d below)
    } else {
        const auto tp = std::chrono::steady_clock::now();
        // Large scenes on a plain context: every 3D batch is handed to the device as soon as it is projected (rxr_stream_batch3d) --
        // the copy into pinned memory and the PCIe transfer of the batches that are done run under the projection of the rest.
        // RXR_STREAM_UPLOAD=0 keeps the plain sequence (project everything, then rxr_upload_frame copies everything).
        std::function<void(size_t, const Batch3D &)> hand_over;
        const char *su = getenv("RXR_STREAM_UPLOAD");  // (read per frame: tests switch it)
        const bool stream_off = su && su[0] == '0', stream_forced = su && su[0] == 'f';
        if (!stream_off && rxr_member_count(ctx) == 1) {
            const std::vector<const Batch3D *> order = scene.batches3d_in_order();
            size_t elements = 0;
            std::vector<uint32_t> cap_v(order.size()), cap_t(order.size());
            for (size_t i = 0; i < order.size(); ++i) {
                const size_t nv = order[i]->vertex_count(), nt = order[i]->triangle_count();
                cap_v[i] = (uint32_t)std::min<size_t>(nv + 4 * nt, 0x7FFFFFFFu);  // the near-plane clip appends at most 4 vertices and
                cap_t[i] = (uint32_t)std::min<size_t>(3 * nt, 0x7FFFFFFFu);       // 2 triangles per triangle (batch3d.rs:627-686)
                elements += nv + nt;
            }
            // the promise of rxr_stream_begin_pinned is made when the buffers every batch projected into LAST frame are page-locked
            // (clip_and_project refills the same vectors; the first frame of a scene, whose vectors do not exist yet, copies).  It is
            // checked again per batch at hand-over: a vector that had to grow into ordinary memory is not handed over, and the frame
            // then goes the plain way.
            // (the `visible` words are a tenth of the records: in batches of fewer than 2048 triangles they stay below the size from which
            // the vectors are page-locked at all.  The frame then promises -- and sends -- the records, as rounds 1-3 did)
            auto arrays_pinned_with = [](const Batch3D &b, bool edgeless) {
                return is_pinned(b.projected_vertices) && is_pinned(b.clipped_uvs) && is_pinned(b.clipped_indices) &&
                       (edgeless ? is_pinned(b.edge_visible) : is_pinned(b.edges)) && (b.normals.empty() || is_pinned(b.clipped_normals));
            };
            bool pinned = true, pinned_records = true;
            for (size_t i = 0; i < order.size() && (pinned || pinned_records); ++i) {
                pinned = pinned && arrays_pinned_with(*order[i], t_frame_edgeless);
                pinned_records = pinned_records && arrays_pinned_with(*order[i], false);
            }
            if (!pinned && pinned_records && t_frame_edgeless) {
                t_frame_edgeless = false;
                pinned = true;
            }
            const bool edgeless = t_frame_edgeless;
            auto arrays_pinned = [arrays_pinned_with, edgeless](const Batch3D &b) { return arrays_pinned_with(b, edgeless); };
            const bool large = (order.size() >= 8 && elements >= (1u << 20)) || (stream_forced && order.size() >= 2);
            const int began = !large ? RXR_ERR_UNSUPPORTED
                              : pinned ? rxr_stream_begin_pinned(ctx, (uint32_t)order.size(), cap_v.data(), cap_t.data())
                                       : rxr_stream_begin(ctx, (uint32_t)order.size(), cap_v.data(), cap_t.data());
            if (began == RXR_OK) {
                hand_over = [ctx, pinned, arrays_pinned, edgeless](size_t i, const Batch3D &b) {
                    if (pinned && b.edges.size() && !arrays_pinned(b)) return;  // (the promise does not hold for this batch: not handed over)
                    rxr_batch3d v{};
                    v.projected_vertices = b.projected_vertices.data();
                    v.clipped_uvs = b.clipped_uvs.data();
                    v.clipped_normals = b.normals.empty() ? nullptr : b.clipped_normals.data();
                    v.clipped_indices = b.clipped_indices.data();
                    v.edges = edgeless ? nullptr : b.edges.data();
                    v.edge_visible = b.edge_visible.data();
                    v.cull_mode = (uint32_t)b.cull_mode_;
                    v.n_vertices = (uint32_t)(b.projected_vertices.size() / 4);
                    v.n_triangles = (uint32_t)b.edges.size();
                    (void)rxr_stream_batch3d(ctx, (uint32_t)i, &v);  // (a refusal makes rxr_upload_frame hand the frame over from scratch)
                };
            }
        }
        static const bool timing0 = getenv("RXR_E2E_TIMING") != nullptr;
        if (timing0) fprintf(stderr, "rxr_e2e_timing before project (stream set-up) %.3f ms\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tp).count());
        if (!scene.project(has_m2d ? &projection_matrix_2d : nullptr, view_matrix, projection_matrix, width, height, hand_over ? &hand_over : nullptr)) {  // :210
            g_error = "clip_and_project: batch without normals (the reference panics at batch3d.rs:605)";
            return RXR_ERR_INVALID;
        }
        static const bool timing = getenv("RXR_E2E_TIMING") != nullptr;
        if (timing) fprintf(stderr, "rxr_e2e_timing project_ms=%.3f\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tp).count());
    }
    for (const Chunk &c : scene.chunks)  // :219-223
        for (const CompiledLight &l : c.lights) scene.dynamic_lights.push_back(l);

    // the dynamic tiles the device sees: scene.dynamic_textures, then every sequence tile of assets.entity_tiles and
    // assets.item_tiles (ids ascending, sequences in insertion order); EntityTile / ItemTile sources are resolved to these slots
    SequenceSlots slots;
    std::vector<const Tile *> dyn_tiles;
    for (const Tile &t : scene.dynamic_textures) dyn_tiles.push_back(&t);
    for (int pass = 0; pass < 2; ++pass)
        for (const auto &kv : pass == 0 ? assets.entity_tiles : assets.item_tiles)
            for (size_t k = 0; k < kv.second.size(); ++k) {
                (pass == 0 ? slots.entity : slots.item)[{kv.first, (uint32_t)k}] = (uint32_t)dyn_tiles.size();
                dyn_tiles.push_back(&kv.second[k]);
            }

    // textures: re-upload only when the asset set changed
    if (g_tex_static_gen != assets.generation || g_tex_dynamic_gen != scene.dynamic_textures_generation) {
        std::vector<rxr_texture> ts, td;
        std::vector<rxr_tile> tiles_s, tiles_d;
        tile_views(assets.tile_list, ts, tiles_s);
        {
            size_t n = 0;
            for (const Tile *t : dyn_tiles) n += t->textures.size();
            td.reserve(n);
            for (const Tile *t : dyn_tiles) {
                rxr_tile rt{};
                rt.textures = td.data() + td.size();
                rt.n_textures = (uint32_t)t->textures.size();
                for (const Texture &x : t->textures) td.push_back(rxr_texture{x.data.data(), x.width, x.height});
                tiles_d.push_back(rt);
            }
        }
        int rc = rxr_set_textures(ctx, tiles_s.data(), (uint32_t)tiles_s.size(), tiles_d.data(), (uint32_t)tiles_d.size());
        if (rc != RXR_OK) {
            g_error = rxr_last_error(ctx);
            return rc;
        }
        g_tex_static_gen = assets.generation;
        g_tex_dynamic_gen = scene.dynamic_textures_generation;
    }

    // Rusteria programs, patterns, palette: re-sent only when they changed
    std::vector<uint32_t> chunk_program_base;
    {
        int rc = ensure_shaders(ctx, scene, assets, chunk_program_base);
        if (rc != RXR_OK) return rc;
    }

    // flatten in submission order (:314-405, :503-552)
    std::vector<rxr_batch3d> b3;
    std::vector<rxr_batch2d> b2;
    std::vector<rxr_chunk> chunks;
    std::vector<std::vector<rxr_texture>> chunk_shader_textures(scene.chunks.size());
    std::vector<rxr_texture> chunk_terrain_textures(scene.chunks.size());
    for (size_t c = 0; c < scene.chunks.size(); ++c) {
        const Chunk &ch = scene.chunks[c];
        for (const Batch3D &b : ch.batches3d_opacity) b3.push_back(view3d(b, RXR_LIST_CHUNK_OPACITY, (int)c, slots));
        for (const Batch3D &b : ch.batches3d) b3.push_back(view3d(b, RXR_LIST_CHUNK, (int)c, slots));
        for (const Batch3D &b : ch.terrain_batch3d) b3.push_back(view3d(b, RXR_LIST_CHUNK_TERRAIN, (int)c, slots));  // :343-356
        for (const Batch2D &b : ch.batches2d) b2.push_back(view2d(b, (int)c, slots));
        for (const Batch2D &b : ch.terrain_batch2d) b2.push_back(view2d(b, (int)c, slots));  // :515-525
        rxr_chunk rc{};
        rc.occluders = ch.occluded_sectors.data();
        rc.n_occluders = (uint32_t)ch.occluded_sectors.size();
        rc.program_base = chunk_program_base[c];
        rc.n_programs = (uint32_t)ch.shaders.size();
        for (size_t k = 0; k < ch.shader_textures.size(); ++k) {
            const Texture &t = ch.shader_textures[k];
            chunk_shader_textures[c].push_back(rxr_texture{ch.shader_texture_present[k] ? t.data.data() : nullptr, (uint32_t)t.width, (uint32_t)t.height});
        }
        rc.shader_textures = chunk_shader_textures[c].data();
        rc.n_shader_textures = (uint32_t)chunk_shader_textures[c].size();
        if (ch.has_terrain_texture) {
            chunk_terrain_textures[c] = rxr_texture{ch.terrain_texture.data.data(), (uint32_t)ch.terrain_texture.width, (uint32_t)ch.terrain_texture.height};
            rc.terrain_texture = &chunk_terrain_textures[c];
        }
        rc.origin[0] = ch.origin[0];
        rc.origin[1] = ch.origin[1];
        rc.size = ch.size;
        chunks.push_back(rc);
    }
    if (scene.resident_chunk_textures && !scene.chunks.empty()) {
        // the chunks' textures are registered once (rxr_set_chunk_textures) and the frames go without them
        if (!chunk_textures_current(scene)) {
            int rc = scene.refresh_chunk_textures();   // (host copies the held registration has newer bytes of)
            if (rc != RXR_OK) return rc;
            std::vector<rxr_texture> tex;
            std::vector<int32_t> terrain_slot, shader_slots;
            std::vector<uint32_t> shader_first{0u};
            for (Chunk &ch : scene.chunks) {
                ch.terrain_slot = ch.has_terrain_texture ? (int32_t)tex.size() : -1;
                terrain_slot.push_back(ch.terrain_slot);
                if (ch.has_terrain_texture) tex.push_back(rxr_texture{ch.terrain_texture.data.data(), (uint32_t)ch.terrain_texture.width, (uint32_t)ch.terrain_texture.height});
                for (size_t k = 0; k < ch.shader_textures.size(); ++k) {
                    shader_slots.push_back(ch.shader_texture_present[k] ? (int32_t)tex.size() : -1);
                    if (ch.shader_texture_present[k]) tex.push_back(rxr_texture{ch.shader_textures[k].data.data(), (uint32_t)ch.shader_textures[k].width, (uint32_t)ch.shader_textures[k].height});
                }
                shader_first.push_back((uint32_t)shader_slots.size());
            }
            g_ctex_held = false;
            rc = rxr_set_chunk_textures(ctx, tex.data(), (uint32_t)tex.size(), terrain_slot.data(), shader_first.data(), shader_slots.data(), (uint32_t)scene.chunks.size());
            if (rc != RXR_OK) {
                g_error = rxr_last_error(ctx);
                (void)rxr_set_chunk_textures(ctx, nullptr, 0, nullptr, nullptr, nullptr, 0);   // (the frames below would not match what was held before)
                return rc;
            }
            ++g_ctex_registrations;
            g_ctex_held = true;
            g_ctex_gens.clear();
            for (Chunk &ch : scene.chunks) {
                g_ctex_gens.push_back(ch.textures_generation);
                ch.slot_registration = g_ctex_registrations;
            }
        }
        for (rxr_chunk &rc : chunks) {
            rc.terrain_texture = nullptr;
            rc.shader_textures = nullptr;
            rc.n_shader_textures = 0;
        }
    } else if (g_ctex_held) {
        (void)rxr_set_chunk_textures(ctx, nullptr, 0, nullptr, nullptr, nullptr, 0);
        g_ctex_held = false;
        g_ctex_gens.clear();
    }
    for (const Batch3D &b : scene.d3_static) b3.push_back(view3d(b, RXR_LIST_STATIC, -1, slots));
    for (const Batch3D &b : scene.d3_dynamic) b3.push_back(view3d(b, RXR_LIST_DYNAMIC, -1, slots));
    for (const Batch3D &b : scene.d3_overlay) b3.push_back(view3d(b, RXR_LIST_OVERLAY, -1, slots));

    // device-side projection: the same batches in the same order, as object-space meshes
    std::vector<rxr_mesh3d> meshes;
    std::vector<float> mesh_transforms;
    if (on_device) {
        uint64_t fp = 0, fp_geometry = 0;
        if (!scene_meshes(scene, &slots, meshes, &mesh_transforms, fp, fp_geometry)) {
            g_error = "clip_and_project: batch without normals (the reference panics at batch3d.rs:605)";
            return RXR_ERR_INVALID;
        }
        if (fp != g_mesh_fingerprint) {
            int rc = register_meshes(ctx, meshes, fp, fp_geometry);
            if (rc != RXR_OK) return rc;
        }
        b3.clear();
    }
    for (const Batch2D &b : scene.d2_static) b2.push_back(view2d(b, -1, slots));
    for (const Batch2D &b : scene.d2_dynamic) b2.push_back(view2d(b, -1, slots));
    if (on_device) {
        // the 2D batches in the same order, as object-space meshes; registered again when anything Batch2D::project reads has changed
        // (2D batches are small: the fingerprint covers their contents)
        std::vector<rxr_mesh2d> m2;
        uint64_t fp = 1469598103934665603ull;
        auto mix = [&](const void *p, size_t n) {
            const uint8_t *q = (const uint8_t *)p;
            for (size_t i = 0; i < n; ++i) fp = (fp ^ q[i]) * 1099511628211ull;
        };
        auto add2 = [&](const Batch2D &b, int chunk) {
            rxr_mesh2d m{};
            m.vertices = b.vertices.data();
            m.indices = b.indices.data();
            m.uvs = b.uvs.data();
            m.n_vertices = (uint32_t)(b.vertices.size() / 2);
            m.n_triangles = (uint32_t)(b.indices.size() / 3);
            m.mode = b.mode_;
            m.repeat_mode = b.repeat_mode_;
            m.source = slots.resolve(b.source_);
            m.receives_light = b.receives_light_ ? 1u : 0u;
            m.shader = b.shader_;
            m.chunk = chunk;
            m2.push_back(m);
            const uint32_t meta[9] = {m.n_vertices, m.n_triangles, m.mode, m.repeat_mode, m.source.kind, m.source.index, m.receives_light, (uint32_t)m.shader, (uint32_t)m.chunk};
            mix(meta, sizeof(meta));
            mix(m.source.pixel, 4);
            mix(b.vertices.data(), b.vertices.size() * 4);
            mix(b.uvs.data(), b.uvs.size() * 4);
            mix(b.indices.data(), b.indices.size() * 4);
        };
        for (size_t c = 0; c < scene.chunks.size(); ++c) {
            for (const Batch2D &b : scene.chunks[c].batches2d) add2(b, (int)c);
            for (const Batch2D &b : scene.chunks[c].terrain_batch2d) add2(b, (int)c);
        }
        for (const Batch2D &b : scene.d2_static) add2(b, -1);
        for (const Batch2D &b : scene.d2_dynamic) add2(b, -1);
        if (fp != g_mesh2d_fingerprint) {
            int rc = rxr_set_meshes2d(ctx, m2.data(), (uint32_t)m2.size());
            if (rc != RXR_OK) {
                g_error = rxr_last_error(ctx);
                g_mesh2d_fingerprint = 0;
                return rc;
            }
            g_mesh2d_fingerprint = fp;
        }
        (void)rxr_set_projection2d(ctx, has_m2d ? projection_matrix_2d.m : nullptr);
        b2.clear();
    }

    std::vector<rxr_light> lights(scene.lights);
    lights.insert(lights.end(), scene.dynamic_lights.begin(), scene.dynamic_lights.end());

    rxr_frame f{};
    f.abi_version = RXR_ABI_VERSION;
    f.width = (uint32_t)w;
    f.height = (uint32_t)h;
    f.tile_size = (uint32_t)tile_size;
    memcpy(f.inverse_view, inverse_view_matrix.m, 64);
    memcpy(f.inverse_projection, inverse_projection_matrix.m, 64);
    f.camera_pos[0] = camera_pos.x; f.camera_pos[1] = camera_pos.y; f.camera_pos[2] = camera_pos.z;
    f.translationd2[0] = translationd2.x; f.translationd2[1] = translationd2.y;
    f.scaled2 = scaled2;
    f.hash_anim = hash_anim;
    f.animation_frame = scene.animation_frame;
    f.flags = (d2_active ? RXR_FLAG_D2_ACTIVE : 0u) | (d3_active ? RXR_FLAG_D3_ACTIVE : 0u) |
              (ignore_background_shader ? RXR_FLAG_IGNORE_BG_SHADER : 0u) |
              (preserve_transparency ? RXR_FLAG_PRESERVE_TRANSPARENCY : 0u) |
              (has_background_color ? RXR_FLAG_HAS_BACKGROUND_COLOR : 0u) | (has_ambient ? RXR_FLAG_HAS_AMBIENT : 0u) |
              (has_sun ? RXR_FLAG_HAS_SUN : 0u);
    memcpy(f.background_color, background_color, 4);
    f.ambient[0] = ambient_color.x; f.ambient[1] = ambient_color.y; f.ambient[2] = ambient_color.z; f.ambient[3] = ambient_color.w;
    f.sun_dir[0] = sun_dir.x; f.sun_dir[1] = sun_dir.y; f.sun_dir[2] = sun_dir.z;
    f.day_factor = day_factor;
    f.sample_mode = sample_mode_;
    f.time = time_;
    f.background_kind = scene.background;
    memcpy(f.background_grid, scene.background_grid, 16);
    f.has_brush_preview = has_brush_preview ? 1u : 0u;
    memcpy(f.brush_position, brush_position, 12);
    f.brush_radius = brush_radius;
    f.brush_falloff = brush_falloff;
    f.batches3d = b3.data();
    f.n_batches3d = (uint32_t)b3.size();
    f.batches2d = b2.data();
    f.n_batches2d = (uint32_t)b2.size();
    f.lights = lights.data();
    f.n_lights = (uint32_t)lights.size();
    f.occluders = mapmini.occluded_sectors.data();
    f.n_occluders = (uint32_t)mapmini.occluded_sectors.size();
    f.linedefs = mapmini.linedefs.data();
    f.n_linedefs = (uint32_t)mapmini.linedefs.size();
    f.chunks = chunks.data();
    f.n_chunks = (uint32_t)chunks.size();
    f.n_shader_programs = (uint32_t)scene.shaders.size();
    if (on_device) {
        f.use_meshes = 3;  // both halves
        memcpy(f.view, view_matrix.m, 64);
        memcpy(f.projection, projection_matrix.m, 64);
        f.mesh_transforms = mesh_transforms.empty() ? nullptr : mesh_transforms.data();
    }

    int rc = rxr_upload_frame(ctx, &f);
    if (rc != RXR_OK) g_error = rxr_last_error(ctx);
    return rc;
}

int Rasterizer::rasterize(Scene &scene, uint8_t *pixels, size_t w, size_t h, size_t tile_size, const Assets &assets) {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (tile_size == 0) {
        g_error = "tile_size 0 (step_by(0) panics in the reference)";
        return RXR_ERR_INVALID;
    }
    static const bool timing = getenv("RXR_E2E_TIMING") != nullptr;  // diagnostics (tools/e2e_probe.py)
    const auto t0 = std::chrono::steady_clock::now();
    int rc = upload(scene, w, h, tile_size, assets);
    if (rc != RXR_OK) return rc;
    if (timing) fprintf(stderr, "rxr_e2e_timing project_and_handover_ms=%.3f\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    rxr_ctx *ctx = context();
    rc = rxr_render_download(ctx, pixels);
    if (rc != RXR_OK) g_error = rxr_last_error(ctx);
    return rc;
}

// ---- the generated terrain's height field (src/chunkbuilder/terrain_generator.rs) -----------------
namespace {
// distance_point_to_segment (:1037-1055) and the same lines of apply_linedef_smoothing (:575-586)
float gen_segment_distance(Vec2 point, Vec2 seg_start, Vec2 seg_end, float &t_param) {
    const Vec2 seg = seg_end - seg_start;
    const float len_sq = rvek::dot(seg, seg);
    if (len_sq < 1e-8f) {
        t_param = 0.0f;
        return rvek::magnitude(point - seg_start);
    }
    const float t = rvek::rclamp(rvek::dot(point - seg_start, seg) / len_sq, 0.0f, 1.0f);
    const Vec2 projection = seg_start + seg * t;
    t_param = t;
    return rvek::magnitude(point - projection);
}
}  // namespace

float TerrainGenerator::sample_height_at(float x, float y) const {
    const Vec2 point{x, y};
    // calculate_map_edge_falloff (:718-743)
    auto edge_falloff = [&]() {
        const float min_edge_dist = std::fmin(std::fmin(std::fmin(point.x - map_box[0], map_box[2] - point.x), point.y - map_box[1]), map_box[3] - point.y);
        if (min_edge_dist <= 0.0f) return 0.0f;
        if (min_edge_dist >= 10.0f) return 1.0f;
        const float t = min_edge_dist / 10.0f;
        return t * t * (3.0f - 2.0f * t);
    };
    // interpolate_height_at (:650-714)
    const size_t C = control_points.size() / 4;
    float base_height = 0.0f;
    if (C) {
        bool exact = false;
        for (size_t i = 0; i < C && !exact; ++i) {
            const float *cp = &control_points[4 * i];
            if (rvek::magnitude(point - Vec2{cp[0], cp[1]}) < 1e-6f) {
                base_height = cp[2] * edge_falloff();
                exact = true;
            }
        }
        if (!exact) {
            float max_height = 0.0f;
            for (size_t i = 0; i < C; ++i) {
                const float *cp = &control_points[4 * i];
                const float distance = rvek::magnitude(point - Vec2{cp[0], cp[1]});
                const float smoothness = cp[3] * 2.0f;
                const float effective_radius = smoothness, smoothing = effective_radius;
                const float sdf_dist = distance - effective_radius;
                float falloff;
                if (sdf_dist < -smoothing) falloff = 1.0f;
                else if (sdf_dist > smoothing) falloff = 0.0f;
                else {
                    const float t = (smoothing - sdf_dist) / (2.0f * smoothing);
                    falloff = t * t * (3.0f - 2.0f * t);
                }
                const float height_contribution = cp[2] * falloff;
                if (height_contribution > max_height) max_height = height_contribution;
            }
            base_height = max_height * edge_falloff();
        }
    }
    // calculate_ridge_height_at (:513-550)
    float ridge_height = 0.0f;
    for (size_t r = 0; r < ridges.size() / 4; ++r) {
        const float *rr = &ridges[4 * r];
        float min_dist = INFINITY;
        for (uint32_t e = ridge_edge_offsets[r]; e < ridge_edge_offsets[r + 1]; ++e) {
            const float *s = &ridge_edges[4 * (size_t)e];
            float t_unused;
            min_dist = std::fmin(min_dist, gen_segment_distance(point, Vec2{s[0], s[1]}, Vec2{s[2], s[3]}, t_unused));
        }
        float contribution;
        if (min_dist <= rr[1]) contribution = rr[0];
        else {
            const float falloff_dist = min_dist - rr[1];
            if (falloff_dist >= rr[2]) contribution = 0.0f;
            else {
                const float t = 1.0f - (falloff_dist / rr[2]);
                contribution = rr[0] * std::pow(t, rr[3]);
            }
        }
        ridge_height += contribution;
    }
    // apply_linedef_smoothing (:555-623)
    const float current_height = base_height + ridge_height;
    float final_height = current_height, total_influence = 0.0f;
    for (size_t l = 0; l < linedefs.size() / 9; ++l) {
        const float *s = &linedefs[9 * l];
        float t_param;
        const float dist_to_line = gen_segment_distance(point, Vec2{s[0], s[1]}, Vec2{s[2], s[3]}, t_param);
        const float target_height = s[4] + (s[5] - s[4]) * t_param;
        float influence;
        if (dist_to_line <= s[6]) influence = 1.0f;
        else {
            const float falloff_dist = dist_to_line - s[6];
            if (falloff_dist >= s[7]) influence = 0.0f;
            else {
                const float t = 1.0f - (falloff_dist / s[7]);
                influence = std::pow(t, s[8]);
            }
        }
        if (influence > 0.0f) {
            total_influence += influence;
            final_height = final_height * (1.0f - influence) + target_height * influence;
        }
    }
    if (total_influence > 1.0f) {
        const float excess = total_influence - 1.0f;
        final_height = final_height * (1.0f - excess * 0.5f) + current_height * (excess * 0.5f);
    }
    return final_height;
}

void TerrainGenerator::sample_normal_at(float x, float y, float normal[3]) const {
    const float delta = 0.1f;
    const float h_center = sample_height_at(x, y);
    const float h_right = sample_height_at(x + delta, y + 0.0f);
    const float h_up = sample_height_at(x + 0.0f, y + delta);
    const Vec3 tangent_x{delta, h_right - h_center, 0.0f}, tangent_z{0.0f, h_up - h_center, delta};
    const Vec3 n = rvek::normalized(rvek::cross(tangent_x, tangent_z));
    normal[0] = n.x, normal[1] = n.y, normal[2] = n.z;
}

void TerrainGenerator::tile_normal(int32_t tx, int32_t tz, float normal[3]) const { sample_normal_at((float)tx + 0.5f, (float)tz + 0.5f, normal); }

std::vector<float> TerrainGenerator::tile_outline_world(int32_t tx, int32_t tz) const {
    const uint32_t sub = std::max(subdivisions, 1u);
    const float step = 1.0f / (float)sub;
    std::vector<float> outline;
    auto push = [&](float x, float z) {
        const float v[3] = {x, sample_height_at(x, z), z};
        outline.insert(outline.end(), v, v + 3);
    };
    for (uint32_t i = 0; i < sub; ++i) push((float)tx + (float)i * step, (float)tz);                 // bottom edge, left to right
    for (uint32_t i = 0; i < sub; ++i) push((float)tx + 1.0f, (float)tz + (float)i * step);          // right edge, bottom to top
    for (uint32_t i = 0; i < sub; ++i) push((float)tx + 1.0f - (float)i * step, (float)tz + 1.0f);   // top edge, right to left
    for (uint32_t i = 0; i < sub; ++i) push((float)tx, (float)tz + 1.0f - (float)i * step);          // left edge, top to bottom
    return outline;
}

void TerrainGenerator::grid_steps(const float box[4], int32_t &steps_x, int32_t &steps_y) const {
    const float cell_size = 1.0f / (float)subdivisions;
    const float min_x = std::floor(box[0]), min_y = std::floor(box[1]), max_x = std::ceil(box[2]), max_y = std::ceil(box[3]);
    // (`as i32 + 1` wraps in a release build where the cast saturated)
    steps_x = (int32_t)((uint32_t)as_i32(std::ceil((max_x - min_x) / cell_size)) + 1u);
    steps_y = (int32_t)((uint32_t)as_i32(std::ceil((max_y - min_y) / cell_size)) + 1u);
}

std::vector<float> TerrainGenerator::generate_grid(const float box[4], int32_t &steps_x, int32_t &steps_y) const {
    const float cell_size = 1.0f / (float)subdivisions;
    const float min_x = std::floor(box[0]), min_y = std::floor(box[1]);
    grid_steps(box, steps_x, steps_y);
    std::vector<float> grid;
    for (int32_t iy = 0; iy < steps_y; ++iy)
        for (int32_t ix = 0; ix < steps_x; ++ix) {
            grid.push_back(min_x + (float)ix * cell_size);
            grid.push_back(min_y + (float)iy * cell_size);
        }
    return grid;
}

void TerrainGenerator::interpolate_heights(const float *points, size_t n, float *heights, float *normals) const {
    std::lock_guard<std::recursive_mutex> lk(g_mu);   // (the worker pool runs one job at a time)
    const size_t per = 64, items = (n + per - 1) / per;
    const size_t records = control_points.size() / 4 + ridge_edges.size() / 4 + linedefs.size() / 9 + 1;
    rxr_parallel::run(items, n * records * (normals ? 3 : 1), [&](size_t item) {
        for (size_t i = item * per; i < std::min(n, (item + 1) * per); ++i) {
            heights[i] = sample_height_at(points[2 * i], points[2 * i + 1]);
            if (normals) sample_normal_at(points[2 * i], points[2 * i + 1], normals + 3 * i);
        }
    });
}

std::vector<uint32_t> TerrainGenerator::triangulate(int32_t steps_x, int32_t steps_y) {
    std::vector<uint32_t> indices;
    if (steps_x < 2 || steps_y < 2) return indices;
    const uint32_t cols = (uint32_t)steps_x;
    indices.reserve((size_t)(steps_x - 1) * (steps_y - 1) * 6);
    for (uint32_t iy = 0; iy + 1 < (uint32_t)steps_y; ++iy)
        for (uint32_t ix = 0; ix + 1 < cols; ++ix) {
            const uint32_t i0 = iy * cols + ix, i1 = i0 + 1, i2 = i0 + cols, i3 = i2 + 1;
            const uint32_t t[6] = {i0, i2, i1, i1, i2, i3};
            indices.insert(indices.end(), t, t + 6);
        }
    return indices;
}

void TerrainGenerator::grid_heights_cpu(const float *boxes, uint32_t n, uint32_t stride, uint32_t *counts, float *heights) const {
    for (uint32_t b = 0; b < n; ++b) {
        int32_t sx, sy;
        grid_steps(boxes + 4 * (size_t)b, sx, sy);
        counts[2 * (size_t)b] = (uint32_t)std::max(sx, 0);
        counts[2 * (size_t)b + 1] = (uint32_t)std::max(sy, 0);
        if ((uint64_t)std::max(sx, 0) * (uint64_t)std::max(sy, 0) > stride) continue;   // (the points are made only where they fit)
        const std::vector<float> grid = generate_grid(boxes + 4 * (size_t)b, sx, sy);
        interpolate_heights(grid.data(), grid.size() / 2, heights + (size_t)b * stride);
    }
}

int TerrainGenerator::register_records(rxr_ctx *ctx) const {
    if (g_generator_gen == generation) return RXR_OK;
    const int rc = rxr_set_terrain_generator(ctx, control_points.data(), (uint32_t)(control_points.size() / 4), ridges.data(), (uint32_t)(ridges.size() / 4),
                                             ridge_edge_offsets.data(), ridge_edges.data(), (uint32_t)(ridge_edges.size() / 4), linedefs.data(),
                                             (uint32_t)(linedefs.size() / 9), map_box);
    if (rc != RXR_OK) {
        g_error = rxr_last_error(ctx);
        return rc;
    }
    g_generator_gen = generation;
    return RXR_OK;
}

int TerrainGenerator::sample_heights(const float *points, uint32_t n, float *heights, float *normals) const {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    std::string err;
    rxr_ctx *ctx = context(&err);
    if (!ctx) return RXR_ERR_NO_DEVICE;
    int rc = register_records(ctx);
    if (rc != RXR_OK) return rc;
    rc = rxr_generated_heights(ctx, points, n, heights, normals);
    if (rc != RXR_OK) g_error = rxr_last_error(ctx);
    return rc;
}

int TerrainGenerator::grid_heights(const float *boxes, uint32_t n, uint32_t stride, uint32_t *counts, float *heights) const {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    std::string err;
    rxr_ctx *ctx = context(&err);
    if (!ctx) return RXR_ERR_NO_DEVICE;
    int rc = register_records(ctx);
    if (rc != RXR_OK) return rc;
    rc = rxr_generated_grids(ctx, boxes, n, subdivisions, stride, counts, heights);
    if (rc != RXR_OK) g_error = rxr_last_error(ctx);
    return rc;
}

// ---- the generated terrain's excluded sectors (:438-457, :747-825, :891-950) ------------------------
bool TerrainGenerator::sector_active(uint32_t s, const float box[4]) const {
    // sector_bbox.intersects(bbox), src/map/bbox.rs:43-48
    const float *sb = &excluded_boxes[4 * (size_t)s];
    return sb[0] <= box[2] && sb[2] >= box[0] && sb[1] <= box[3] && sb[3] >= box[1];
}

bool TerrainGenerator::point_in_sector(float x, float y, uint32_t s) const {
    const Vec2 point{x, y};
    const float *verts = excluded_vertices.data() + 2 * (size_t)excluded_vertex_offsets[s];
    const size_t len = excluded_vertex_offsets[s + 1] - excluded_vertex_offsets[s];
    if (len < 3) return false;
    const float epsilon = 0.01f;
    size_t j = len - 1;
    for (size_t i = 0; i < len; ++i) {
        const Vec2 vi{verts[2 * i], verts[2 * i + 1]}, vj{verts[2 * j], verts[2 * j + 1]};
        const Vec2 edge = vj - vi;
        const float edge_length_sq = rvek::dot(edge, edge);
        if (edge_length_sq > 0.0f) {
            const float t = rvek::rclamp(rvek::dot(point - vi, edge) / edge_length_sq, 0.0f, 1.0f);
            const Vec2 projection = vi + edge * t;
            const float dist = rvek::magnitude(point - projection);
            if (dist < epsilon) return true;
        }
        j = i;
    }
    bool inside = false;
    j = len - 1;
    for (size_t i = 0; i < len; ++i) {
        const Vec2 vi{verts[2 * i], verts[2 * i + 1]}, vj{verts[2 * j], verts[2 * j + 1]};
        if (((vi.y > point.y) != (vj.y > point.y)) && (point.x < (vj.x - vi.x) * (point.y - vi.y) / (vj.y - vi.y) + vi.x)) inside = !inside;
        j = i;
    }
    return inside;
}

std::vector<float> TerrainGenerator::apply_exclusions(const float *grid, const float *heights, int32_t steps_x, int32_t steps_y, const std::vector<uint32_t> &active) const {
    std::vector<float> out;
    const size_t P = (steps_x > 0 && steps_y > 0) ? (size_t)steps_x * (size_t)steps_y : 0;
    auto push = [&](size_t i) {
        const float v[3] = {grid[2 * i], heights[i], grid[2 * i + 1]};
        out.insert(out.end(), v, v + 3);
    };
    if (active.empty()) {
        for (size_t i = 0; i < P; ++i) push(i);
        return out;
    }
    const std::vector<uint32_t> indices = triangulate(steps_x, steps_y);
    const size_t T = indices.size() / 3;
    std::vector<uint8_t> exclude(T, 0);
    {
        std::lock_guard<std::recursive_mutex> lk(g_mu);   // (the worker pool runs one job at a time)
        const size_t per = 64, items = (T + per - 1) / per;
        rxr_parallel::run(items, T * 3 * (excluded_vertices.size() / 2 + 1), [&](size_t item) {
            for (size_t t = item * per; t < std::min(T, (item + 1) * per); ++t) {
                const uint32_t *ix = &indices[3 * t];
                for (const uint32_t s : active)
                    if (point_in_sector(grid[2 * ix[0]], grid[2 * ix[0] + 1], s) && point_in_sector(grid[2 * ix[1]], grid[2 * ix[1] + 1], s) &&
                        point_in_sector(grid[2 * ix[2]], grid[2 * ix[2] + 1], s)) {
                        exclude[t] = 1;
                        break;
                    }
            }
        });
    }
    for (size_t t = 0; t < T; ++t)
        if (!exclude[t])
            for (int k = 0; k < 3; ++k) push(indices[3 * t + k]);
    return out;
}

void TerrainGenerator::generate_meshes_cpu(const float *boxes, uint32_t n, uint32_t stride, uint32_t *counts, float *vertices) const {
    const uint32_t S = (uint32_t)(excluded_boxes.size() / 4);
    for (uint32_t b = 0; b < n; ++b) {
        const float *box = boxes + 4 * (size_t)b;
        int32_t sx, sy;
        grid_steps(box, sx, sy);
        std::vector<uint32_t> active;
        for (uint32_t s = 0; s < S; ++s)
            if (sector_active(s, box)) active.push_back(s);
        uint32_t *c = counts + 4 * (size_t)b;
        c[0] = (uint32_t)std::max(sx, 0), c[1] = (uint32_t)std::max(sy, 0), c[2] = (uint32_t)active.size(), c[3] = 0;
        const uint64_t points = (uint64_t)c[0] * c[1], cells = (c[0] > 1 && c[1] > 1) ? (uint64_t)(c[0] - 1) * (c[1] - 1) : 0;
        if ((active.empty() ? points : 6 * cells) > stride) continue;   // (the points are made only where the layout fits)
        if (!active.empty() && !cells) continue;
        const std::vector<float> grid = generate_grid(box, sx, sy);
        std::vector<float> heights(grid.size() / 2);
        interpolate_heights(grid.data(), heights.size(), heights.data());
        const std::vector<float> v = apply_exclusions(grid.data(), heights.data(), sx, sy, active);
        c[3] = (uint32_t)(v.size() / 3);
        float *o = vertices + (size_t)b * stride * 4;
        for (size_t i = 0; i < v.size() / 3; ++i) o[4 * i] = v[3 * i], o[4 * i + 1] = v[3 * i + 1], o[4 * i + 2] = v[3 * i + 2], o[4 * i + 3] = 1.0f;
    }
}

int TerrainGenerator::register_exclusions(rxr_ctx *ctx) const {
    if (g_exclusion_gen == generation) return RXR_OK;
    const int rc = rxr_set_terrain_exclusions(ctx, excluded_boxes.data(), excluded_vertex_offsets.data(), excluded_vertices.data(), (uint32_t)(excluded_boxes.size() / 4),
                                              (uint32_t)(excluded_vertices.size() / 2));
    if (rc != RXR_OK) {
        g_error = rxr_last_error(ctx);
        return rc;
    }
    g_exclusion_gen = generation;
    return RXR_OK;
}

int TerrainGenerator::generate_meshes(const float *boxes, uint32_t n, uint32_t stride, uint32_t *counts, float *vertices) const {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    std::string err;
    rxr_ctx *ctx = context(&err);
    if (!ctx) return RXR_ERR_NO_DEVICE;
    int rc = register_records(ctx);
    if (rc != RXR_OK || (rc = register_exclusions(ctx)) != RXR_OK) return rc;
    rc = rxr_generated_meshes(ctx, boxes, n, subdivisions, stride, counts, vertices);
    if (rc != RXR_OK) g_error = rxr_last_error(ctx);
    return rc;
}

// ---- the generated terrain's tiles (:954-1034) ------------------------------------------------------
int TerrainGenerator::set_tiles(const int32_t *cells, const uint32_t *slots, uint32_t n, uint32_t n_tiles_) {
    char message[256] = "";
    const int rc = rxr_check_terrain_tiles(cells, slots, n, n_tiles_, message, sizeof message);
    if (rc != RXR_OK) {
        g_error = std::string("TerrainGenerator::set_tiles: ") + message;
        return rc;
    }
    tile_cells.assign(cells, cells + 2 * (size_t)n);
    tile_slots.assign(slots, slots + n);
    n_tiles = n_tiles_;
    tile_overrides.clear();   // the reference is handed its FxHashMap ready: built here, once
    for (size_t i = 0; i < tile_slots.size(); ++i) tile_overrides[{tile_cells[2 * i], tile_cells[2 * i + 1]}] = tile_slots[i];
    touch();
    return RXR_OK;
}

namespace {
// Rust's `x as i32`: saturating, a NaN is 0
int32_t f32_as_i32(float x) {
    if (x != x) return 0;
    if (x >= 2147483648.0f) return INT32_MAX;
    if (x <= -2147483648.0f) return INT32_MIN;
    return (int32_t)x;
}
}  // namespace

std::vector<TerrainGenerator::TileGroup> TerrainGenerator::partition_by_tiles(const float *vertices, const uint32_t *indices, size_t n_indices, const float *uvs) const {
    std::map<uint32_t, std::vector<uint32_t>> per_tile;   // (ordered: the groups come in ascending slot)
    for (size_t t = 0; t + 3 <= n_indices; t += 3) {
        const uint32_t i0 = indices[t], i1 = indices[t + 1], i2 = indices[t + 2];
        const float *uv0 = uvs + 2 * (size_t)i0, *uv1 = uvs + 2 * (size_t)i1, *uv2 = uvs + 2 * (size_t)i2;
        const float center_u = (uv0[0] + uv1[0] + uv2[0]) / 3.0f;
        const float center_v = (uv0[1] + uv1[1] + uv2[1]) / 3.0f;
        const std::pair<int32_t, int32_t> tile_cell{f32_as_i32(std::floor(center_u)), f32_as_i32(std::floor(center_v))};
        const auto found = tile_overrides.find(tile_cell);
        const uint32_t tile_id = found != tile_overrides.end() ? found->second : 0u;
        std::vector<uint32_t> &batch = per_tile[tile_id];
        batch.insert(batch.end(), indices + t, indices + t + 3);
    }
    std::vector<TileGroup> result;
    for (const auto &entry : per_tile) {
        TileGroup g;
        g.slot = entry.first;
        std::map<uint32_t, uint32_t> vertex_remap;
        for (const uint32_t old_idx : entry.second) {
            uint32_t new_idx;
            const auto existing = vertex_remap.find(old_idx);
            if (existing != vertex_remap.end()) {
                new_idx = existing->second;
            } else {
                new_idx = (uint32_t)(g.vertices.size() / 3);
                vertex_remap[old_idx] = new_idx;
                g.vertices.insert(g.vertices.end(), vertices + 3 * (size_t)old_idx, vertices + 3 * (size_t)old_idx + 3);
                g.uvs.insert(g.uvs.end(), uvs + 2 * (size_t)old_idx, uvs + 2 * (size_t)old_idx + 2);
            }
            g.indices.push_back(new_idx);
        }
        result.push_back(std::move(g));
    }
    return result;
}

void TerrainGenerator::generate_tile_meshes_cpu(const float *boxes, uint32_t n, uint32_t max_groups, uint32_t vertex_stride, uint32_t triangle_stride, uint32_t *box_counts,
                                                uint32_t *counts, uint32_t *group_tiles, float *vertices, float *uvs_out, uint32_t *indices_out) const {
    const uint32_t S = (uint32_t)(excluded_boxes.size() / 4);
    // (vertices, indices, uvs) of every box as apply_exclusions returns them (:823-824): heights and keep flags over the worker pool
    struct Mesh {
        std::vector<float> v, uvs;
        std::vector<uint32_t> idx;
    };
    std::vector<Mesh> meshes(n);
    size_t work = 0;
    for (uint32_t b = 0; b < n; ++b) {
        const float *box = boxes + 4 * (size_t)b;
        int32_t sx, sy;
        grid_steps(box, sx, sy);
        std::vector<uint32_t> active;
        for (uint32_t s = 0; s < S; ++s)
            if (sector_active(s, box)) active.push_back(s);
        uint32_t *c = box_counts + 4 * (size_t)b;
        c[0] = (uint32_t)std::max(sx, 0), c[1] = (uint32_t)std::max(sy, 0), c[2] = (uint32_t)active.size(), c[3] = 0;
        for (uint32_t g = 0; g < max_groups; ++g) {
            const size_t m = (size_t)b * max_groups + g;
            counts[2 * m] = counts[2 * m + 1] = 0u, group_tiles[m] = 0xFFFFFFFFu;
        }
        const uint64_t points = (uint64_t)c[0] * c[1], cells = (c[0] > 1 && c[1] > 1) ? (uint64_t)(c[0] - 1) * (c[1] - 1) : 0;
        if (!cells || (active.empty() ? points : 6 * cells) > vertex_stride || 2 * cells > triangle_stride) continue;
        const std::vector<float> grid = generate_grid(box, sx, sy);
        std::vector<float> heights(grid.size() / 2);
        interpolate_heights(grid.data(), heights.size(), heights.data());
        Mesh &mesh = meshes[b];
        mesh.v = apply_exclusions(grid.data(), heights.data(), sx, sy, active);
        if (active.empty()) {
            mesh.idx = triangulate(sx, sy);
        } else {
            mesh.idx.resize(mesh.v.size() / 3);
            for (size_t i = 0; i < mesh.idx.size(); ++i) mesh.idx[i] = (uint32_t)i;
        }
        mesh.uvs.resize(mesh.v.size() / 3 * 2);
        for (size_t i = 0; i < mesh.v.size() / 3; ++i) mesh.uvs[2 * i] = mesh.v[3 * i], mesh.uvs[2 * i + 1] = mesh.v[3 * i + 2];   // generate_uvs (:882-888)
        work += mesh.idx.size() * 64;
    }
    // partition_by_tiles, one box a task over the pool (the boxes are independent; inside a box the reference's walk, in its order)
    std::lock_guard<std::recursive_mutex> lk(g_mu);   // (the worker pool runs one job at a time)
    rxr_parallel::run(n, work, [&](size_t b) {
        const Mesh &mesh = meshes[b];
        if (mesh.idx.empty()) return;
        const std::vector<TileGroup> groups = partition_by_tiles(mesh.v.data(), mesh.idx.data(), mesh.idx.size(), mesh.uvs.data());
        if (groups.size() > max_groups) return;
        box_counts[4 * b + 3] = (uint32_t)groups.size();
        for (size_t g = 0; g < groups.size(); ++g) {
            const TileGroup &t = groups[g];
            const size_t m = b * max_groups + g, nv = t.vertices.size() / 3;
            counts[2 * m] = (uint32_t)nv, counts[2 * m + 1] = (uint32_t)(t.indices.size() / 3), group_tiles[m] = t.slot;
            float *o = vertices + m * vertex_stride * 4, *u = uvs_out + m * vertex_stride * 2;
            for (size_t i = 0; i < nv; ++i) {
                o[4 * i] = t.vertices[3 * i], o[4 * i + 1] = t.vertices[3 * i + 1], o[4 * i + 2] = t.vertices[3 * i + 2], o[4 * i + 3] = 1.0f;
                u[2 * i] = t.uvs[2 * i], u[2 * i + 1] = t.uvs[2 * i + 1];
            }
            std::copy(t.indices.begin(), t.indices.end(), indices_out + m * triangle_stride * 3);
        }
    });
}

int TerrainGenerator::register_tiles(rxr_ctx *ctx) const {
    if (g_tiles_gen == generation) return RXR_OK;
    const int rc = rxr_set_terrain_tiles(ctx, tile_cells.data(), tile_slots.data(), (uint32_t)tile_slots.size(), n_tiles);
    if (rc != RXR_OK) {
        g_error = rxr_last_error(ctx);
        return rc;
    }
    g_tiles_gen = generation;
    return RXR_OK;
}

int TerrainGenerator::generate_tile_meshes(const float *boxes, uint32_t n, uint32_t max_groups, uint32_t vertex_stride, uint32_t triangle_stride, uint32_t *box_counts,
                                           uint32_t *counts, uint32_t *group_tiles, float *vertices, float *uvs, uint32_t *indices) const {
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    std::string err;
    rxr_ctx *ctx = context(&err);
    if (!ctx) return RXR_ERR_NO_DEVICE;
    int rc = register_records(ctx);
    if (rc != RXR_OK || (rc = register_exclusions(ctx)) != RXR_OK || (rc = register_tiles(ctx)) != RXR_OK) return rc;
    rc = rxr_generated_tile_meshes(ctx, boxes, n, subdivisions, max_groups, vertex_stride, triangle_stride, box_counts, counts, group_tiles, vertices, uvs, indices);
    if (rc != RXR_OK) g_error = rxr_last_error(ctx);
    return rc;
}

// ---- cameras ------------------------------------------------------------------------------------
void orbit_camera(Vec3 center, float distance, float azimuth, float elevation, float fov, float near, float far, float w,
                  float h, Mat4 &view, Mat4 &proj) {
    const float x = distance * std::cos(azimuth) * std::cos(elevation);
    const float y = distance * std::sin(elevation);
    const float z = distance * std::sin(azimuth) * std::cos(elevation);
    const Vec3 eye = Vec3{x, y, z} + center;
    view = rvek::look_at_rh(eye, center, Vec3{0, 1, 0});
    proj = rvek::perspective_fov_rh_zo(fov * (3.14159265358979323846f / 180.0f), w, h, near, far);
}

void firstp_camera(Vec3 position, Vec3 center, float fov, float near, float far, float w, float h, Mat4 &view, Mat4 &proj) {
    view = rvek::look_at_rh(position, center, Vec3{0, 1, 0});
    proj = rvek::perspective_fov_rh_zo(fov * (3.14159265358979323846f / 180.0f), w, h, near, far);
}

}  // namespace rusterix
