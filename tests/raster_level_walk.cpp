// Prints the feature-level table of the raster code (rusterix_amd/csrc/rxr_device.h) and the mappings onto it:
//   level <index> <chunk> <programs> <ssp> <inline_site> <out_of_line> <vis_programs> <pixel_items>
//   static <kernel_level> <plain_programs> <level>
//   jit <slot> <RXR_JIT_LEVEL number> <level> <slot found again from the number>
// Built and read by tests/test_raster_level_cpu.py.
#include <cstdio>

#include "rxr_device.h"

static_assert(level_features(Level::VmP).pixel_items, "the table serves constant expressions (template arguments, if constexpr)");

int main() {
    for (int i = 0; i <= (int)Level::VmP; ++i) {
        const LevelFeatures f = level_features((Level)i);
        std::printf("level %d %d %d %d %d %d %d %d\n", i, f.chunk, f.programs, f.ssp, f.inline_site, (int)f.out_of_line, f.vis_programs, f.pixel_items);
    }
    for (unsigned kl = KL_COMMON; kl <= KL_VM_V; ++kl)
        for (int plain = 0; plain < 2; ++plain) std::printf("static %u %d %d\n", kl, plain, (int)static_level(kl, plain != 0));
    for (int slot = 0; slot < N_JIT_SLOTS; ++slot)
        std::printf("jit %d %d %d %d\n", slot, jit_level_number[slot], (int)jit_slot_level[slot], jit_slot_of_number(jit_level_number[slot]));
    std::printf("jit_other %d %d\n", jit_slot_of_number(0), jit_slot_of_number(9));
    return 0;
}
