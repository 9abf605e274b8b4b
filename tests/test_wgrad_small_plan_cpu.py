"""CPU: the plan of the small-map 3 x 3 weight gradient (csrc/convk_wgrad.hip, convk_wgrad3_small) through its host entry point
savfi_convk_wgrad3_small_plan, over maps 1 x 1 .. 24 x 32, pad 0 / 1 and 64 .. 512 channels: the LDS of a workgroup fits a CU, the bands
cover every row exactly once, the (sample, band) list is cut into at least one part and never into more than a round of workgroups, and
the kernel writes the gradient itself exactly when there is a channel block per CU."""
import ctypes

import pytest

from meta_interpolation_amd import _hip

LDS_CU = 160 * 1024
MAPS = [(1, 1), (1, 16), (2, 3), (5, 7), (6, 16), (7, 16), (8, 16), (9, 16), (12, 16), (13, 17), (3, 32), (4, 32), (5, 32), (12, 31),
        (23, 32), (24, 32), (24, 17), (17, 1)]
CHANNELS = [(64, 64), (64, 128), (80, 72), (256, 256), (256, 512), (512, 256), (512, 512)]
BATCHES = [(1, 1), (2, 1), (2, 2), (4, 1), (4, 4), (8, 4), (16, 4)]
CUS = [1, 8, 64, 255, 256, 257, 304]


def _plan(N, T, Ci, Co, H, W, pad, cus):
    out = (ctypes.c_int * 8)()
    rc = _hip.lib().savfi_convk_wgrad3_small_plan(N, T, Ci, Co, H, W, pad, cus, out)
    assert rc == 0, (N, T, Ci, Co, H, W, pad, cus, rc)
    return dict(zip(("bh", "bands", "lds", "splits", "direct", "blocks", "items", "ksteps"), out))


@pytest.mark.parametrize("pad", [0, 1])
def test_plan_properties(pad):
    for Ho, Wo in MAPS:
        H, W = Ho + 2 - 2 * pad, Wo + 2 - 2 * pad
        for Ci, Co in CHANNELS:
            for N, T in BATCHES:
                for cus in CUS:
                    p = _plan(N, T, Ci, Co, H, W, pad, cus)
                    what = (N, T, Ci, Co, H, W, pad, cus, p)
                    assert 0 < p["lds"] <= LDS_CU, what
                    # band b = rows b bh .. min(Ho, (b + 1) bh) - 1: every row once, no empty band
                    assert p["bh"] >= 1 and (p["bands"] - 1) * p["bh"] < Ho <= p["bands"] * p["bh"], what
                    covered = [0] * Ho
                    for b in range(p["bands"]):
                        for y in range(b * p["bh"], min(Ho, (b + 1) * p["bh"])):
                            covered[y] += 1
                    assert covered == [1] * Ho, what
                    # a band's pixels in whole 32-pixel K-steps (two rows each on a map of at most 16 columns), and its images inside the LDS
                    gw = 16 if Wo <= 16 else 32
                    rows = p["ksteps"] * 32 // gw
                    assert rows >= p["bh"] and rows - p["bh"] < 32 // gw, what
                    assert 24 * 16 * (rows * gw + (rows + 2) * (gw + 2)) <= p["lds"], what
                    assert p["blocks"] == T * -(-Co // 64) * -(-Ci // 64), what
                    assert p["items"] == (N // T) * p["bands"], what
                    assert 1 <= p["splits"] <= p["items"], what
                    assert p["direct"] == (1 if p["blocks"] >= cus else 0), what
                    if p["direct"]:
                        assert p["splits"] == 1, what
                    else:
                        assert p["blocks"] * p["splits"] <= max(cus, p["blocks"]), what      # one round of workgroups


def test_plan_of_the_deep_layers():
    """12 x 16: two bands of 6 rows (3 K-steps of two rows); 24 x 32: six bands of 4 rows; 512 -> 512 with T = 4 is one block per CU."""
    p = _plan(8, 4, 512, 512, 12, 16, 1, 256)
    assert (p["bh"], p["bands"], p["ksteps"], p["blocks"], p["direct"], p["splits"]) == (6, 2, 3, 256, 1, 1), p
    p = _plan(8, 4, 512, 512, 24, 32, 1, 256)
    assert (p["bh"], p["bands"], p["ksteps"], p["blocks"], p["direct"], p["splits"]) == (4, 6, 4, 256, 1, 1), p
    p = _plan(8, 4, 256, 256, 24, 32, 1, 256)
    assert (p["blocks"], p["direct"], p["splits"], p["items"]) == (64, 0, 4, 12), p
    p = _plan(8, 4, 512, 256, 24, 32, 1, 256)
    assert (p["blocks"], p["direct"], p["splits"]) == (128, 0, 2), p


def test_plan_rejects_what_the_kernel_does_not_take():
    out = (ctypes.c_int * 8)()
    lib = _hip.lib()
    assert lib.savfi_convk_wgrad3_small_plan(2, 1, 64, 64, 12, 33, 1, 256, out) == -3        # 33 output columns
    assert lib.savfi_convk_wgrad3_small_plan(2, 1, 64, 64, 12, 16, 2, 256, out) == -3        # pad 2
    assert lib.savfi_convk_wgrad3_small_plan(3, 2, 64, 64, 12, 16, 1, 256, out) == -2        # N % T
    assert lib.savfi_convk_wgrad3_small_plan(2, 1, 64, 64, 2, 16, 0, 256, out) == -2         # no output row
    assert lib.savfi_convk_wgrad3_small_plan(2, 1, 64, 64, 12, 16, 1, 256, None) == -1
