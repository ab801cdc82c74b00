"""What each feature level of the raster code carries (rusterix_amd/csrc/rxr_device.h: Level, level_features), on the CPU.

The rows below ARE the specification, written out as literals; none of them is computed from the header.
tests/raster_level_walk.cpp prints the table and the three mappings onto it: RasterParams.kernel_level (+ plain_programs) -> the
static kernel's level, the run-time compiler's slots -> the RXR_JIT_LEVEL numbers and their levels, and every level's out-of-line
twin.  tests/test_gpu_routes.py, test_gpu_shaders.py and test_gpu_shader_jit.py run the kernels of every level on the device."""
import collections
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Row = collections.namedtuple("Row", "chunk programs ssp inline_site out_of_line vis_programs pixel_items")

# in the order of the enum.  Common and Chunk run no programs: nothing of them is inlined, they are their own twins, and no program
# decides visibility.
LEVELS = ["Common", "Chunk", "Vm", "VmOol", "VmS", "VmSOol", "VmSV", "VmV", "JitPlain", "VmP"]
TABLE = {
    #                 chunk programs ssp inline out_of_line vis_programs pixel_items
    "Common":   Row(0, 0, 0, 0, "Common", 0, 1),   # k_raster*, _fused, _rows*, _pair*
    "Chunk":    Row(1, 0, 0, 0, "Chunk",  0, 1),   # k_raster_chunk*
    "Vm":       Row(1, 1, 0, 1, "VmOol",  1, 0),   # k_raster_vm, compiled slot 0
    "VmOol":    Row(1, 1, 0, 0, "VmOol",  1, 0),   # (inner: Vm's alpha test)
    "VmS":      Row(1, 1, 1, 1, "VmSOol", 1, 0),   # k_raster_vm_s
    "VmSOol":   Row(1, 1, 1, 0, "VmSOol", 1, 0),   # (inner: VmS's alpha test)
    "VmSV":     Row(1, 1, 1, 1, "VmSOol", 0, 1),   # k_raster_vm_sv
    "VmV":      Row(1, 1, 0, 1, "VmOol",  0, 1),   # k_raster_vm_v, compiled slot 1
    "JitPlain": Row(0, 1, 0, 1, "VmOol",  0, 1),   # compiled slot 2
    "VmP":      Row(0, 1, 1, 1, "VmSOol", 0, 1),   # k_raster_vm_p
}
# (kernel_level, plain_programs) -> the level of the static kernel (tests/test_raster_route_cpu.py has the kernels' names)
STATIC = {(0, 0): "Common", (0, 1): "Common", (1, 0): "Chunk", (1, 1): "Chunk", (2, 0): "Vm", (2, 1): "Vm", (3, 0): "VmS", (3, 1): "VmS",
          (4, 0): "VmSV", (4, 1): "VmP", (5, 0): "VmV", (5, 1): "VmV"}
# slot of the run-time compiler -> (-DRXR_JIT_LEVEL, level)
JIT = {0: (2, "Vm"), 1: (7, "VmV"), 2: (8, "JitPlain")}


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    exe = tmp_path_factory.mktemp("level") / "walk"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "rusterix_amd", "csrc"),
                    os.path.join(ROOT, "tests", "raster_level_walk.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    lines = collections.defaultdict(list)
    for line in out.splitlines():
        kind, *fields = line.split()
        lines[kind].append([int(f) for f in fields])
    return lines


def test_every_level_carries_what_the_table_says(walk):
    assert len(TABLE) == len(LEVELS) == 10 and len(walk["level"]) == 10
    for index, *features in walk["level"]:
        name = LEVELS[index]
        features[4] = LEVELS[features[4]]
        assert Row(*features) == TABLE[name], name


def test_the_out_of_line_twin_has_no_inlined_site_and_the_same_stack_pointer():
    for name, row in TABLE.items():
        twin = TABLE[row.out_of_line]
        assert twin.inline_site == 0 and twin.ssp == row.ssp and twin.out_of_line == row.out_of_line, name


def test_kernel_level_and_plain_programs_give_the_static_kernels_level(walk):
    assert {(kl, plain): LEVELS[level] for kl, plain, level in walk["static"]} == STATIC


def test_the_compiled_slots_are_levels_2_7_and_8(walk):
    assert {slot: (number, LEVELS[level]) for slot, number, level, _ in walk["jit"]} == JIT
    assert all(found == slot for slot, _, _, found in walk["jit"])
    assert walk["jit_other"] == [[-1, -1]]      # any other number is refused (rxr_kernels.hip: static_assert)
