"""CPU: the F(4x4) launch plan of csrc/winograd.hip (make_plan) against its transcription in tests/conv_ref.py.

tests/test_conv_variants_gpu.py claims to launch every F(4x4) variant the plan can produce (tile-block shape, reduction split, store
width, masked / unit-major epilogues), and it computes those claims with the transcription.  Here the library's own plan answers for the
same shapes -- workgroup count (savfi_conv3x3_f4_workgroups), partial-output workspace (= the number of reduction splits),
unit-major support -- so a change of the C plan that the transcription does not follow fails here, on a machine without a GPU."""
import random

import pytest

from meta_interpolation_amd import _hip
from tests.conv_ref import f4_plan

CHANNELS = [1, 2, 3, 6, 7, 8, 9, 16, 31, 32, 33, 51, 63, 64, 65, 100, 128, 192, 248, 249, 256, 257, 264, 384, 500, 511, 512, 513, 640]
MAPS = [1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 13, 15, 16, 17, 24, 31, 32, 33, 48, 63, 64, 65, 96, 127, 128, 129, 130, 137, 160, 236, 258, 450, 512]
NS = [1, 2, 3, 4, 5, 8, 16, 31, 32]


def _grid(count, seed):
    rnd = random.Random(seed)
    cases = [(1, 512, 512, 12, 16, 1, 0), (1, 264, 64, 12, 16, 1, 0), (32, 51, 51, 258, 450, 0, 0), (8, 32, 32, 384, 512, 1, 1),
             (1, 8, 8, 128, 4, 1, 0), (1, 8, 8, 64, 8, 1, 1), (2, 1, 1, 1, 1, 1, 0)]
    for _ in range(count):
        cases.append((rnd.choice(NS), rnd.choice(CHANNELS), rnd.choice(CHANNELS), rnd.choice(MAPS), rnd.choice(MAPS), rnd.randint(0, 1),
                      rnd.randint(0, 1)))
    return cases


@pytest.mark.parametrize("seed", [0, 1])
def test_f4_plan_transcription_matches_the_library(seed):
    lib = _hip.lib()
    seen = {"split": 0, "ragged": 0, "ts": set(), "vecw": set(), "f2": 0}
    for N, Ci, Co, H, W, pad, mode in _grid(6000, seed):
        plan = f4_plan(N, Ci, Co, H, W, pad, mode)
        wgs = int(lib.savfi_conv3x3_f4_workgroups(N, Ci, Co, H, W, pad, mode))
        case = (N, Ci, Co, H, W, pad, mode)
        if wgs < 0:                                   # an empty output: the library refuses the shape
            assert plan is None, case
            continue
        if plan is None:
            assert wgs == 0, case                     # F(2x2) by channel counts
            seen["f2"] += 1
            continue
        assert wgs == plan["workgroups"], (case, wgs, plan)
        if H * W >= 4:
            # the partial outputs of a split launch: nsplit x N x I x Ho x Wo floats (none unsplit)
            part = int(lib.savfi_conv3x3_tasks_pre_workspace_floats(N, 1, Ci, Co, H, W, pad, mode))
            I = Co if mode == 0 else Ci
            assert part == (plan["nsplit"] * N * I * plan["Ho"] * plan["Wo"] if plan["nsplit"] > 1 else 0), (case, part, plan)
            if mode == 0:
                want = plan["nsplit"] == 1 and plan["Wo"] % 16 == 0
                assert int(lib.savfi_conv3x3_unit16_supported(N, 1, Ci, Co, H, W, pad)) == int(want), (case, plan)
            else:
                want = plan["nsplit"] == 1 and W % 16 == 0 and plan["Wo"] % 2 == 0
                assert int(lib.savfi_conv3x3_in_unit16_supported(N, 1, Ci, Co, H, W, pad)) == int(want), (case, plan)
        seen["split"] += plan["nsplit"] > 1
        seen["ragged"] += plan["ragged"]
        seen["ts"].add(plan["tile_shift"])
        seen["vecw"].add(plan["vecw"])
    # the grid reaches every branch of the plan
    assert seen["split"] and seen["ragged"] and seen["f2"], seen
    assert seen["ts"] == set(range(6)) and seen["vecw"] == {1, 2, 4}, seen


def test_f4_plan_examples():
    """Hand-checked plans: the ragged split of the issue's example and the benchmark's widest layers."""
    p = f4_plan(1, 264, 64, 12, 16, 1, 0)             # 33 chunks, 8 per split: 5 splits, the last with one chunk
    assert (p["nsplit"], p["chunks_per_split"], p["ragged"], p["tile_shift"]) == (5, 8, True, 3)
    p = f4_plan(32, 51, 51, 258, 450, 0, 0)           # 64 x 112 tiles: 2 x 16-tile blocks (224, as many as 4 x 8), no split, x4 stores
    assert (p["nsplit"], p["tile_shift"], p["vecw"]) == (1, 4, 4)
    p = f4_plan(8, 512, 512, 24, 32, 1, 0)            # 6 x 8 tiles of 4 x 4 in two 4 x 8 blocks; 512 workgroups: the reduction in two
    assert (p["tile_shift"], p["th"], p["tw"], p["nsplit"], p["chunks_per_split"]) == (3, 2, 1, 2, 32)
    assert f4_plan(1, 576, 528, 12, 20, 1, 0) is None  # beyond 512 channels: F(2x2)
