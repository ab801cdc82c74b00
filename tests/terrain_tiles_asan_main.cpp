// A stand-alone program over the host mirror's CPU partition_by_tiles (rusterix_host.cpp), built with -fsanitize=address,undefined and
// run as a child process by tests/test_terrain_tiles_cpu.py: tile overrides in stripes over boxes of both layouts (one with an
// excluded square that swallows a whole tile), negative cells, an empty grid, a grid without a cell, boxes whose layout exceeds a
// stride or max_groups (box_counts only), the sums printed so that nothing is optimised away.  It touches no device: the mirror's
// device forms are not called.
#include <cstdio>
#include <vector>

#include "../rusterix_amd/csrc/host/rusterix_host.hpp"

using rusterix::TerrainGenerator;

int main() {
    TerrainGenerator g;
    g.subdivisions = 2;
    g.control_points = {20, 20, 4, 2, 40, 30, -1, 3};
    const float map_box[4] = {0, 0, 64, 64};
    for (int i = 0; i < 4; ++i) g.map_box[i] = map_box[i];
    const float square[8] = {19.5f, 19.5f, 22.5f, 19.5f, 22.5f, 21.5f, 19.5f, 21.5f}, square_box[4] = {19.5f, 19.5f, 22.5f, 21.5f};
    g.excluded_boxes.assign(square_box, square_box + 4);
    g.excluded_vertices.assign(square, square + 8);
    g.excluded_vertex_offsets = {0u, 4u};
    std::vector<int32_t> cells;
    std::vector<uint32_t> slots;
    for (int32_t x = -4; x < 40; ++x)
        for (int32_t z = -4; z < 40; ++z)
            if ((x + 4) % 3) cells.push_back(x), cells.push_back(z), slots.push_back((uint32_t)((x + 4) % 3));
    cells.push_back(20), cells.push_back(20), slots.push_back(3u);   // cell (20, 20) alone has slot 3 ((20 + 4) % 3 == 0: not listed above)
    if (g.set_tiles(cells.data(), slots.data(), (uint32_t)slots.size(), 4) != RXR_OK) return 1;
    if (g.set_tiles(cells.data(), slots.data(), (uint32_t)slots.size(), 3) == RXR_OK) return 1;   // slot 3 is out of range: refused, nothing changes
    // the unshared layout (cell (20, 20) lies inside the square: no group of slot 3), the shared one with negative cells, an empty
    // grid, one column, a box above the vertex stride
    const float boxes[5][4] = {{16.0f, 16.0f, 24.0f, 24.0f}, {-3.5f, -2.25f, 4.0f, 3.0f}, {5.0f, 5.0f, 4.0f, 4.0f}, {30.0f, 30.0f, 30.0f, 33.0f}, {0.0f, 0.0f, 32.0f, 32.0f}};
    const uint32_t n = 5, mg = 3, vs = 6 * 16 * 16, ts = 2 * 16 * 16;
    std::vector<uint32_t> box_counts(4 * n), counts(2 * n * mg), group_tiles(n * mg), indices((size_t)n * mg * ts * 3, 0xFFFFFFFFu);
    std::vector<float> vertices((size_t)n * mg * vs * 4, -1.0f), uvs((size_t)n * mg * vs * 2, -1.0f);
    g.generate_tile_meshes_cpu(&boxes[0][0], n, mg, vs, ts, box_counts.data(), counts.data(), group_tiles.data(), vertices.data(), uvs.data(), indices.data());
    double sum = 0.0;
    for (uint32_t b = 0; b < n; ++b) {
        std::printf("box %u: %u x %u points, %u active sectors, %u groups\n", b, box_counts[4 * b], box_counts[4 * b + 1], box_counts[4 * b + 2], box_counts[4 * b + 3]);
        if (box_counts[4 * b + 3] > mg) return 2;
        for (uint32_t k = 0; k < box_counts[4 * b + 3]; ++k) {
            const size_t m = (size_t)b * mg + k;
            if (counts[2 * m] > vs || counts[2 * m + 1] > ts || group_tiles[m] > 2) return 3;
            for (uint32_t i = 0; i < 3 * counts[2 * m + 1]; ++i) {
                if (indices[m * ts * 3 + i] >= counts[2 * m]) return 4;
                sum += vertices[(m * vs + indices[m * ts * 3 + i]) * 4 + 1];
            }
        }
    }
    if (box_counts[3] != 3 || box_counts[7] != 3 || box_counts[11] != 0 || box_counts[15] != 0 || box_counts[19] != 0) return 5;
    const float lone[4] = {20.0f, 20.0f, 21.0f, 21.0f};   // every triangle of the box excluded: no group at all
    g.generate_tile_meshes_cpu(lone, 1, mg, vs, ts, box_counts.data(), counts.data(), group_tiles.data(), vertices.data(), uvs.data(), indices.data());
    if (box_counts[2] != 1 || box_counts[3] != 0) return 6;
    TerrainGenerator plain;   // no overrides, no sectors: one group of slot 0
    plain.generate_tile_meshes_cpu(&boxes[1][0], 1, 1, vs, ts, box_counts.data(), counts.data(), group_tiles.data(), vertices.data(), uvs.data(), indices.data());
    if (box_counts[3] != 1 || group_tiles[0] != 0 || counts[0] != 9 * 7 || counts[1] != 2 * 8 * 6) return 7;
    for (float v : uvs) sum += v;
    std::printf("terrain tiles under sanitizers: clean (checksum %.6f)\n", sum);
    return 0;
}
