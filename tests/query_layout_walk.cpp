// The io-buffer layout of the blocking device queries (rusterix_amd/csrc/rxr_query_layout.h) over every subset of their optional
// arrays, for tests/test_query_io_cpu.py.  Per (query, n, subset) one line: the query, n, the subset's bits (bit i: the i-th
// optional array of the list is present), the total, then "offset:bytes" per array of the list in order.
#include <cstdio>

#include "rxr_query_layout.h"

struct Array {
    size_t unit;     // bytes per ray (intersect, terrain_hits) or per texel (the bakes)
    bool optional;   // an output the caller may leave NULL
};
struct Query {
    const char *name;
    unsigned n_arrays;
    Array arrays[QueryLayout::MAX];
};

// the arrays in the order each entry point declares them: rxr_intersect (origins, dirs, t, mesh, triangle | hitpoint, uv, normal),
// rxr_terrain_hits (origins, dirs, hit | t, world_pos, grid_pos), rxr_bake_shaders (| pixels, rgba), rxr_bake_terrain (rgba)
static const Query QUERIES[] = {
    {"intersect", 8, {{12, false}, {12, false}, {4, false}, {4, false}, {4, false}, {12, true}, {8, true}, {12, true}}},
    {"terrain_hits", 6, {{12, false}, {12, false}, {4, false}, {4, true}, {12, true}, {8, true}}},
    {"bake_shaders", 2, {{16, true}, {4, true}}},
    {"bake_terrain", 1, {{4, false}}},
};

int main() {
    const size_t counts[] = {1, 63, 64, 65, 1000};
    for (const Query &q : QUERIES) {
        unsigned n_opt = 0;
        for (unsigned i = 0; i < q.n_arrays; ++i) n_opt += q.arrays[i].optional;
        for (size_t n : counts)
            for (unsigned subset = 0; subset < (1u << n_opt); ++subset) {
                QueryLayout L;
                unsigned opt = 0;
                for (unsigned i = 0; i < q.n_arrays; ++i) {
                    const bool present = !q.arrays[i].optional || ((subset >> opt++) & 1u);
                    L.add(present ? n * q.arrays[i].unit : 0);
                }
                printf("%s %zu %u %zu", q.name, n, subset, L.total);
                for (unsigned i = 0; i < L.n; ++i) printf(" %zu:%zu", L.off[i], L.bytes[i]);
                printf("\n");
            }
    }
    return 0;
}
