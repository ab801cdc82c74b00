// rxr_route.h -- which raster kernel a launch gets.  Plain C++ (no HIP): the one decision behind rxr_launch_raster_grid and
// rxr_raster_takes_spans (rxr_kernels.hip), compiled on its own by tests/test_raster_route_cpu.py.
#pragma once
#include "rxr_device.h"  // KernelLevel (the part of it that is plain C++)

namespace rxr_route {

// one value per raster kernel of rxr_kernels.hip (k_raster, k_raster_fused, ... in the order of their definitions); the launcher's
// table gives each its kernel and its name
enum Route {
    RASTER, FUSED, RASTER_RL,
    ROWS, ROWS_RL, ROWS_SP, ROWS_RL_SP, ROWS_CUT, ROWS_CUT_RL,
    PAIR, PAIR_RL,
    CHUNK, CHUNK_RL, CHUNK_CUT, CHUNK_CUT_RL,
    VM, VM_S, VM_SV, VM_P, VM_V,
    N_ROUTES
};

// what a launch's RasterParams say (rxr_upload.hip, phase RasterParams; render_impl for fused_small) and the two environment
// switches, which the caller reads per launch (the tests switch them)
struct Facts {
    unsigned kernel_level;  // KernelLevel
    bool plain_programs;
    unsigned fused_small;   // 0 binned, 1 fused (RXR_SMALL_MODE=1, at most RXR_STAGE_TRIS triangles), 2 implicit list
    bool d3_active;         // RXR_FLAG_D3_ACTIVE
    bool split_rounds;      // cut-out texels, profiled batches under an opacity pass
    bool spans;             // RasterParams.row_spans is attached -- or, for the host's question, would be
    bool rl;                // relaxed_lights (demoted to exact on large or non-finite light parameters) && n_lights
    bool has_opacity;
    unsigned tile_stride;
    bool no_rows;           // RXR_NO_ROWS: binned scenes walk every candidate per pixel (k_raster)
    bool pairs_on;          // RXR_PAIR_TILES=1
};

struct Choice {
    Route route;
    bool takes_spans;  // the kernel looks RasterParams.row_spans up (raster_tile SPANS)
    bool pair_grid;    // its grid is (tiles_x, (tiles_y + 1) / 2): two tiles per workgroup
};

// rounds in row mode AROUND cut-out / profiled candidates (scan_lists_rows SPLITR): binned 3D frames only, the others never reach
// that code.  Also what picks k_raster_jit_cut (rxr_jit.hip).
inline bool rounds_cut(bool split_rounds, unsigned fused_small, bool d3_active) { return split_rounds && fused_small == 0u && d3_active; }

//   fact                                                                                  kernel
//   KL_VM_V / KL_VM_SV + plain_programs / KL_VM_SV / KL_VM_S / KL_VM                      k_raster_vm_v / _p / _sv / _s / k_raster_vm
//   KL_CHUNK (chunk textures, RXR_MIN_KERNEL_LEVEL=1)                                     k_raster_chunk   [_cut: rounds_cut] [_rl]
//   fused_small 1                                                                         k_raster_fused
//   binned 3D frame (fused_small 0), RXR_PAIR_TILES=1, no opacity pass, tile_stride 1     k_raster_pair    [_rl]
//   binned, split_rounds                                                                  k_raster_rows_cut [_rl]
//   binned, row_spans (sparse frame)                                                      k_raster_rows_sp / k_raster_rows_rl_sp
//   binned                                                                                k_raster_rows    [_rl]
//   small frame (fused_small 2), no 3D pass, RXR_NO_ROWS                                  k_raster         [_rl]
//   _rl: Facts.rl with the 3D pass active (frames without a 3D light loop: one kernel for both modes)
// Every level above KL_COMMON looks the spans up, and so do k_raster_rows_cut* and the two _sp kernels; the small-scene kernels, the pair
// kernels and plain k_raster_rows* never do (raster_tile SPANS).
inline Choice raster_route(const Facts &f) {
    const bool rl = f.rl && f.d3_active;
    if (f.kernel_level >= KL_VM_V) return {VM_V, true, false};
    if (f.kernel_level == KL_VM_SV) return {f.plain_programs ? VM_P : VM_SV, true, false};
    if (f.kernel_level == KL_VM_S) return {VM_S, true, false};
    if (f.kernel_level == KL_VM) return {VM, true, false};
    if (f.kernel_level == KL_CHUNK) {
        if (rounds_cut(f.split_rounds, f.fused_small, f.d3_active)) return {rl ? CHUNK_CUT_RL : CHUNK_CUT, true, false};
        return {rl ? CHUNK_RL : CHUNK, true, false};
    }
    if (f.fused_small == 1u) return {FUSED, false, false};
    if (f.fused_small == 0u && f.d3_active && !f.no_rows) {
        // two tiles per workgroup (raster_tile_pair): opt-in.  Built in round 3 as the 16 x 32-tile experiment the round-2 verdict asked to
        // repeat on a build that passes parity: it does pass (tests/test_gpu_rows.py runs it), and it LOSES -- 1 M-triangle grid 555 ->
        // 654 us at 8 waves per SIMD (817 / 697 / 668 at 7 / 6 / 5), teapot 29 -> 46 us (profiles/r03/pair_tiles_experiment.txt): what the
        // pair saves in per-tile instructions it pays in spills (the two shading passes share one register budget) and in a per-workgroup
        // latency chain that is twice as long.
        if (f.pairs_on && !f.has_opacity && f.tile_stride == 1u) return {rl ? PAIR_RL : PAIR, false, true};
        if (f.split_rounds) return {rl ? ROWS_CUT_RL : ROWS_CUT, true, false};
        if (f.spans) return {rl ? ROWS_RL_SP : ROWS_SP, true, false};
        return {rl ? ROWS_RL : ROWS, false, false};
    }
    return {rl ? RASTER_RL : RASTER, false, false};
}

}  // namespace rxr_route
