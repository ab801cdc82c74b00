// A stand-alone program over the host mirror's CPU apply_exclusions (rusterix_host.cpp), built with -fsanitize=address,undefined and
// run as a child process by tests/test_terrain_exclusion_cpu.py: sectors of every kind (a square on grid lines, a concave one, one
// with two vertices, one without any, one with a repeated vertex, one whose box is a NaN) through every CPU function, the sums
// printed so that nothing is optimised away.  It touches no device: the mirror's device forms are not called.
#include <cmath>
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
    const std::vector<std::vector<float>> polygons = {
        {20, 20, 26, 20, 26, 26, 20, 26},                            // a square on grid lines
        {28, 18, 36, 18, 36, 22, 31, 22, 31, 30, 28, 30},            // an L
        {21, 21, 22, 22},                                            // two vertices: active, holds nothing
        {},                                                          // no vertices
        {22.5f, 27.5f, 22.5f, 27.5f, 25.5f, 27.5f, 24.0f, 31.25f},   // a repeated vertex: a zero-length edge
        {30, 30, 34, 30, 32, 34},                                    // its box is a NaN: never active
    };
    const float nan = std::nanf("");
    const float boxes_of[6][4] = {{20, 20, 26, 26}, {28, 18, 36, 30}, {21, 21, 22, 22}, {19, 19, 21, 21}, {22.5f, 27.5f, 25.5f, 31.25f}, {30, nan, 34, 34}};
    for (size_t s = 0; s < polygons.size(); ++s) {
        g.excluded_boxes.insert(g.excluded_boxes.end(), boxes_of[s], boxes_of[s] + 4);
        g.excluded_vertices.insert(g.excluded_vertices.end(), polygons[s].begin(), polygons[s].end());
        g.excluded_vertex_offsets.push_back((uint32_t)(g.excluded_vertices.size() / 2));
    }
    g.touch();
    double sum = 0.0;
    size_t inside = 0;
    for (uint32_t s = 0; s < polygons.size(); ++s)
        for (int y = 16; y <= 34; ++y)
            for (int x = 16; x <= 38; ++x) inside += g.point_in_sector((float)x, (float)y * 0.5f + 8.0f, s) ? 1 : 0;
    // a box with sectors, one without (the shared layout), an empty grid, one whose layout exceeds the stride (counts only)
    const float boxes[4][4] = {{16.0f, 16.0f, 32.0f, 32.0f}, {0.0f, 0.0f, 4.5f, 3.0f}, {5.0f, 5.0f, 4.0f, 4.0f}, {16.0f, 16.0f, 48.0f, 48.0f}};
    const uint32_t stride = 6 * 32 * 32;
    std::vector<uint32_t> counts(4 * 4);
    std::vector<float> vertices(4 * (size_t)stride * 4, -1.0f);
    g.generate_meshes_cpu(&boxes[0][0], 4, stride, counts.data(), vertices.data());
    for (int b = 0; b < 4; ++b) {
        std::printf("box %d: %u x %u points, %u active sectors, %u vertices\n", b, counts[4 * b], counts[4 * b + 1], counts[4 * b + 2], counts[4 * b + 3]);
        if (counts[4 * b + 3] > stride) return 2;
    }
    if (counts[2] == 0 || counts[3] == 0 || counts[3] >= 6 * 32 * 32 || counts[6] != 0 || counts[4 * 3 + 3] != 0) return 3;
    for (float v : vertices) sum += v;
    TerrainGenerator empty;
    empty.generate_meshes_cpu(&boxes[1][0], 1, stride, counts.data(), vertices.data());
    sum += counts[3];
    std::printf("terrain exclusions under sanitizers: clean (%zu points inside, checksum %.6f)\n", inside, sum);
    return 0;
}
