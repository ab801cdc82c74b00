// A stand-alone program over the host mirror's CPU TerrainGenerator (rusterix_host.cpp), built with -fsanitize=address,undefined
// and run as a child process by tests/test_terrain_gen_cpu.py: one scene through every CPU function, the sums printed so that
// nothing is optimised away.  It touches no device: the mirror's device forms are not called.
#include <cstdio>
#include <vector>

#include "../rusterix_amd/csrc/host/rusterix_host.hpp"

using rusterix::TerrainGenerator;

int main() {
    TerrainGenerator g;
    g.subdivisions = 3;
    g.control_points = {20, 20, 4, 2, 40, 30, -1, 3, 20, 20, 7, 1};
    g.ridges = {2, 1, 6, 2, 1, 0, 3, 0.5f, 1.5f, 0, 2, 1};
    g.ridge_edge_offsets = {0, 4, 4, 5};   // a square, a ridge without edges, one degenerate edge
    g.ridge_edges = {28, 28, 36, 28, 36, 28, 36, 36, 36, 36, 28, 36, 28, 36, 28, 28, 10, 50, 10, 50};
    g.linedefs = {4, 32, 60, 34, 0.5f, 1.5f, 1, 8, 2, 30, 4, 34, 60, 1, 0, 1.5f, 6, 0.7f, 5, 5, 5, 5, 2, 2, 1, 3, 1};
    const float map_box[4] = {0, 0, 64, 64};
    for (int i = 0; i < 4; ++i) g.map_box[i] = map_box[i];
    g.touch();
    double sum = 0.0;
    const float boxes[3][4] = {{-0.5f, -1.25f, 9.5f, 7.0f}, {30.0f, 30.0f, 34.0f, 33.0f}, {5.0f, 5.0f, 4.0f, 4.0f}};
    for (const auto &box : boxes) {
        int32_t sx = 0, sy = 0;
        const std::vector<float> grid = g.generate_grid(box, sx, sy);
        std::vector<float> heights(grid.size() / 2), normals(grid.size() / 2 * 3);
        g.interpolate_heights(grid.data(), heights.size(), heights.data(), normals.data());
        const std::vector<uint32_t> tris = TerrainGenerator::triangulate(sx, sy);
        for (uint32_t t : tris)
            if (t >= heights.size()) return 2;
        for (float h : heights) sum += h;
        for (float n : normals) sum += n;
        std::printf("box %d x %d: %zu points, %zu indices\n", sx, sy, heights.size(), tris.size());
    }
    const uint32_t stride = 40 * 40;
    std::vector<uint32_t> counts(2 * 3);
    std::vector<float> all(3 * (size_t)stride, -1.0f);
    g.grid_heights_cpu(&boxes[0][0], 3, stride, counts.data(), all.data());
    for (float h : all) sum += h;
    float n[3];
    g.tile_normal(20, 20, n);
    sum += n[0] + n[1] + n[2];
    for (float v : g.tile_outline_world(31, 33)) sum += v;
    TerrainGenerator empty;
    sum += empty.sample_height_at(1.0f, 2.0f);
    std::printf("terrain generator under sanitizers: clean (checksum %.6f)\n", sum);
    return 0;
}
