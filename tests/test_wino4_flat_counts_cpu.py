"""The two workgroup counts of an F(4x4) launch (csrc/winograd.hip), without a device.

savfi_conv3x3_f4_workgroups counts 2^(5-s) x 2^s tile BLOCKS: the host routes by it (WINO4_MIN_WORKGROUPS, wino_form2), so it keeps the
values of the build before the flat tile lists -- hard-coded below from that build.  savfi_conv3x3_f4_launched_workgroups is the grid a
launch really has: ceil(tiles / 32) workgroups per sample, reduction split and 32-channel block."""
import ctypes

from meta_interpolation_amd import _hip, hip_ops
from tests import conv_ref as R

# (N, Ci, Co, H, W, pad, mode): block count of the parent build
TABLE = [
    ((32, 51, 51, 256, 448, 0, 1), 16320),       # the SepConv tail's 51 -> 51 data gradient: 65 x 113 tiles
    ((32, 64, 64, 137, 236, 1, 0), 4480),        # Subnet layers: 35 x 59 tiles
    ((32, 64, 51, 137, 236, 1, 0), 4480),
    ((32, 64, 256, 137, 236, 1, 1), 4480),
    ((32, 256, 64, 137, 236, 1, 0), 4480),
    ((8, 32, 32, 384, 512, 1, 0), 3072),         # encoder / decoder maps: powers of two, nothing to gain
    ((8, 6, 32, 384, 512, 1, 0), 3072),
    ((8, 64, 64, 192, 256, 1, 0), 1536),
    ((8, 128, 128, 96, 128, 1, 1), 768),
    ((8, 256, 256, 48, 64, 1, 0), 384),
    ((8, 512, 512, 24, 32, 1, 0), 512),          # split reductions
    ((8, 512, 512, 12, 16, 1, 1), 512),
    ((4, 8, 8, 4, 4, 1, 0), 4),
    ((4, 8, 8, 4, 4, 0, 0), 4),
    ((4, 16, 40, 22, 38, 1, 0), 24),
    ((4, 16, 40, 22, 37, 0, 1), 12),
    ((4, 51, 51, 22, 40, 0, 0), 24),
    ((4, 51, 51, 9, 130, 1, 1), 40),
    ((4, 8, 8, 7, 5, 1, 0), 4),
    ((4, 8, 8, 7, 5, 0, 0), 4),
    ((4, 256, 256, 8, 8, 1, 0), 128),
    ((4, 24, 40, 20, 48, 1, 0), 24),
    ((4, 24, 40, 20, 48, 0, 1), 12),
    ((2, 16, 24, 64, 7, 1, 1), 2),
    ((2, 24, 16, 3, 125, 1, 1), 2),
    ((1, 3, 3, 1000, 1000, 1, 0), 2000),
    ((2, 576, 528, 12, 20, 1, 0), 0),            # beyond 512 channels: F(2x2), both counts 0
    ((3, 33, 65, 129, 257, 0, 1), 486),
]


def _flat(shape):
    N = shape[0]
    p = R.f4_plan(*shape)
    if p is None:
        return 0
    tiles = R.cdiv(p["Ho"], 4) * R.cdiv(p["Wo"], 4)
    return R.cdiv(tiles, R.TT) * (p["IP"] // R.COB) * p["nsplit"] * N


def test_routing_count_keeps_the_parent_values():
    lib = _hip.lib()
    for shape, blocks in TABLE:
        assert int(lib.savfi_conv3x3_f4_workgroups(*shape)) == blocks, shape
        p = R.f4_plan(*shape)
        assert (p["workgroups"] if p else 0) == blocks, shape
    with hip_ops.wino4_block_decode():          # the routing count does not follow the test hook
        for shape, blocks in TABLE:
            assert int(lib.savfi_conv3x3_f4_workgroups(*shape)) == blocks, shape


def test_launched_grid_is_ceil_tiles_over_32():
    lib = _hip.lib()
    for shape, blocks in TABLE:
        got = int(lib.savfi_conv3x3_f4_launched_workgroups(*shape))
        assert got == _flat(shape) == hip_ops.wino4_launched_workgroups(*shape), shape
        assert got <= blocks and (got > 0) == (blocks > 0), shape
    # the layers the flat lists are for: 255 -> 230 and 70 -> 65 groups per sample and channel block
    assert _flat(TABLE[0][0]) == 230 * 2 * 32 and TABLE[0][1] == 255 * 2 * 32
    assert _flat(TABLE[1][0]) == 65 * 2 * 32 and TABLE[1][1] == 70 * 2 * 32


def test_block_decode_hook_restores_the_block_grid():
    lib = _hip.lib()
    with hip_ops.wino4_block_decode():
        for shape, blocks in TABLE:
            assert int(lib.savfi_conv3x3_f4_launched_workgroups(*shape)) == blocks, shape
        with hip_ops.wino4_block_decode(False):
            assert hip_ops.wino4_launched_workgroups(*TABLE[0][0]) == _flat(TABLE[0][0])
        assert hip_ops.wino4_launched_workgroups(*TABLE[0][0]) == TABLE[0][1]
    prev = ctypes.c_int(-1)
    assert lib.savfi_conv3x3_debug_f4_block_decode(0, ctypes.byref(prev)) == 0 and prev.value == 0      # flat is the default
    for shape, _ in TABLE:
        assert int(lib.savfi_conv3x3_f4_launched_workgroups(*shape)) == _flat(shape), shape


def test_count_queries_reject_bad_arguments():
    lib = _hip.lib()
    assert int(lib.savfi_conv3x3_f4_launched_workgroups(0, 8, 8, 8, 8, 1, 0)) == -2
    assert int(lib.savfi_conv3x3_f4_launched_workgroups(1, 8, 8, 8, 8, 2, 0)) == -3
    assert int(lib.savfi_conv3x3_f4_launched_workgroups(1, 8, 8, 1, 8, 0, 0)) == -2          # empty output
