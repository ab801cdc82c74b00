// mesh_resize_bases_main.cpp -- the layout arithmetic of rxr_resize_meshes (rusterix_amd/csrc/rxr_mesh_resize.h: rxr_resize_bases) as a
// program of its own.  Built with a host compiler, and once more with -fsanitize=address,undefined; tests/test_mesh_resize_abi.py runs
// both and holds the printed words to its numpy restatement.
//
//   mesh_resize_bases_main FILE     FILE: n pairs of u32 (vertices, triangles).  Prints "reached R totals VIN TIN VOUT TOUT" and then
//                                   one line "VIN TIN VOUT TOUT" per mesh whose bases were written (min(R + 1, n) lines).
// Every array is a heap block of exactly its size, so that a write past the bases of the meshes walked is a sanitizer report.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../rusterix_amd/csrc/rxr_mesh_resize.h"

int main(int argc, char **argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: mesh_resize_bases_main FILE\n");
        return 2;
    }
    FILE *f = fopen(argv[1], "rb");
    if (!f) {
        perror(argv[1]);
        return 2;
    }
    std::vector<uint32_t> counts;
    uint32_t pair[2];
    while (fread(pair, sizeof(uint32_t), 2, f) == 2) counts.insert(counts.end(), pair, pair + 2);
    fclose(f);
    const size_t n = counts.size() / 2;
    uint32_t *bases = (uint32_t *)malloc(n ? 4 * n * sizeof(uint32_t) : 1);
    uint64_t totals[4];
    const size_t reached = rxr_resize_bases(counts.data(), n, bases, totals);
    printf("reached %zu totals %llu %llu %llu %llu\n", reached, (unsigned long long)totals[0], (unsigned long long)totals[1], (unsigned long long)totals[2],
           (unsigned long long)totals[3]);
    const size_t written = reached < n ? reached + 1 : n;
    for (size_t i = 0; i < written; ++i) printf("%u %u %u %u\n", bases[4 * i], bases[4 * i + 1], bases[4 * i + 2], bases[4 * i + 3]);
    free(bases);
    return 0;
}
