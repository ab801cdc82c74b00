// Walks the whole fact space of rxr_route::raster_route (rusterix_amd/csrc/rxr_route.h) and prints one line per combination:
// the eleven facts, then the kernel's name, whether it looks the row spans up and whether its grid is the pair grid.
// Built and read by tests/test_raster_route_cpu.py.
#include <cstdio>

#include "rxr_route.h"

static const char *name(rxr_route::Route r) {
    switch (r) {  // (-Werror=switch: a route without a name here does not compile)
        case rxr_route::RASTER: return "k_raster";
        case rxr_route::FUSED: return "k_raster_fused";
        case rxr_route::RASTER_RL: return "k_raster_rl";
        case rxr_route::ROWS: return "k_raster_rows";
        case rxr_route::ROWS_RL: return "k_raster_rows_rl";
        case rxr_route::ROWS_SP: return "k_raster_rows_sp";
        case rxr_route::ROWS_RL_SP: return "k_raster_rows_rl_sp";
        case rxr_route::ROWS_CUT: return "k_raster_rows_cut";
        case rxr_route::ROWS_CUT_RL: return "k_raster_rows_cut_rl";
        case rxr_route::PAIR: return "k_raster_pair";
        case rxr_route::PAIR_RL: return "k_raster_pair_rl";
        case rxr_route::CHUNK: return "k_raster_chunk";
        case rxr_route::CHUNK_RL: return "k_raster_chunk_rl";
        case rxr_route::CHUNK_CUT: return "k_raster_chunk_cut";
        case rxr_route::CHUNK_CUT_RL: return "k_raster_chunk_cut_rl";
        case rxr_route::VM: return "k_raster_vm";
        case rxr_route::VM_S: return "k_raster_vm_s";
        case rxr_route::VM_SV: return "k_raster_vm_sv";
        case rxr_route::VM_P: return "k_raster_vm_p";
        case rxr_route::VM_V: return "k_raster_vm_v";
        case rxr_route::N_ROUTES: break;
    }
    return "?";
}

int main() {
    for (unsigned level = 0; level <= 5; ++level)
        for (unsigned plain = 0; plain < 2; ++plain)
            for (unsigned fused = 0; fused <= 2; ++fused)
                for (unsigned bits = 0; bits < 256; ++bits) {
                    rxr_route::Facts f;
                    f.kernel_level = level;
                    f.plain_programs = plain != 0;
                    f.fused_small = fused;
                    f.d3_active = bits & 1;
                    f.split_rounds = bits & 2;
                    f.spans = bits & 4;
                    f.rl = bits & 8;
                    f.has_opacity = bits & 16;
                    f.tile_stride = (bits & 32) ? 2u : 1u;
                    f.no_rows = bits & 64;
                    f.pairs_on = bits & 128;
                    const rxr_route::Choice c = rxr_route::raster_route(f);
                    std::printf("%u %u %u %d %d %d %d %d %u %d %d %s %d %d\n", level, plain, fused, f.d3_active, f.split_rounds, f.spans, f.rl, f.has_opacity,
                                f.tile_stride, f.no_rows, f.pairs_on, name(c.route), c.takes_spans, c.pair_grid);
                }
    return 0;
}
