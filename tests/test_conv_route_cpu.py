"""CPU: hip_ops.conv_route and every public routing predicate against the transcription of the predicates they replaced
(tests/conv_route_ref.py), over a seeded grid of layers in both forms and with each knob moved off its default in turn.

The predicates take stand-ins for tensors (shape, dtype, dim(), is_cuda): the routing is host logic over integers."""
import random

import pytest
import torch

from meta_interpolation_amd import _hip, hip_ops
from tests import conv_route_ref as ref

CHANNELS = [1, 3, 6, 8, 9, 16, 32, 47, 48, 51, 63, 64, 65, 128, 192, 256, 512, 513]
MAPS = [1, 2, 3, 4, 8, 12, 13, 16, 24, 32, 33, 48, 64, 66, 96, 98, 128, 130, 160, 256, 384, 512]
NS = [1, 2, 3, 4, 8, 16]
FAR = 10 ** 9

# each knob off its default in turn; the *_FWD thresholds far above the *_BWD ones: the forward stays on ATen, the data gradient does not
SETTINGS = [{}] + [{name: value} for name, value in [
    ("CONVK", False), ("WINOGRAD_CONV", False), ("WINO_MIN_TILES_FWD", 3000), ("WINO_MIN_TILES_BWD", 3000), ("WINO_MIN_TILES_FWD_BATCHED", 1000),
    ("WINO_MIN_TILES_BWD_BATCHED", 1000), ("WGRAD_MIN_PIXELS", 500), ("WGRAD_MIN_CI", 64), ("WGRAD_WINO", False), ("WGRAD_WINO_MIN_GFLOP", 0.5),
    ("WGRAD_WINO_MIN_PIXELS", 1000), ("CONVK_3X3_MIN_PIXELS", 100), ("CONVK_WGRAD3_RING_MIN_PIXELS", 500),
    ("CONVK_WGRAD3_RING_SMALL_MIN_PIXELS", 300), ("CONVK_WGRAD3", False), ("CONVK_WGRAD3_RING", False), ("WINO4_MIN_WORKGROUPS", 16),
    ("WINO4_MIN_PIXELS", 5000), ("TASKS_MIN_TILES_FWD", 500), ("TASKS_MIN_TILES_BWD", 500), ("TASKS_WGRAD_MIN_PIXELS", 200)]] + [
    {"WINO_MIN_TILES_FWD": FAR, "WINO_MIN_TILES_FWD_BATCHED": FAR}, {"TASKS_MIN_TILES_FWD": FAR}]

# (T, N, Ci, Co, H, W, K, stride, padding, dilation, groups, direct): one layer per route, whatever the random draw (F(4x4) workgroups by
# tests.conv_ref.f4_plan: test_fixed_layers_have_the_workgroups_their_routes_rest_on)
FIXED = [(T, N, Ci, Co, H, W, 3, 1, pad, 1, 1, False) for T in (None, 4) for N, Ci, Co, H, W, pad in [
    (8, 32, 32, 96, 128, 1), (4, 64, 64, 96, 128, 1), (4, 51, 51, 98, 130, 0),       # 192 workgroups: F(4x4)
    (8, 51, 51, 66, 130, 0),                                                          # 256, 128 wide: the unit-major layer
    (2, 64, 64, 96, 128, 1),                                                          # 96: the direct kernel by size
    (2, 16, 16, 16, 16, 1), (4, 16, 16, 16, 16, 1),                                   # 2 / 4: F(2x2), ATen weight gradient
    (8, 256, 256, 24, 32, 1), (1, 8, 8, 16, 16, 1), (1, 64, 64, 32, 32, 1)]] + [
    (None, 2, 16, 16, 32, 32, 3, 2, 1, 1, 1, False), (2, 2, 8, 8, 64, 64, 3, 2, 1, 1, 1, False), (None, 1, 6, 16, 24, 24, 5, 1, 2, 1, 1, False),
    (3, 3, 6, 16, 20, 24, 5, 1, 2, 1, 1, False), (None, 1, 8, 8, 8, 8, 3, 1, 1, 1, 1, True), (None, 4, 16, 16, 32, 32, 3, 1, 1, 1, 2, False),
    (None, 2, 3, 8, 64, 64, 1, 1, 0, 1, 1, False), (2, 2, 64, 3, 64, 64, 7, 1, 3, 1, 1, False)]


class Stand:
    """What a routing predicate reads of a tensor."""
    dtype, is_cuda = torch.float32, True

    def __init__(self, *shape):
        self.shape = torch.Size(shape)

    def dim(self):
        return len(self.shape)


def _layers(count, seed):
    rnd = random.Random(seed)
    layers = list(FIXED)
    for _ in range(count):
        K = rnd.choice([1, 3, 3, 3, 5, 7])
        layers.append((rnd.choice([None, None, 2, 4]), rnd.choice(NS), rnd.choice(CHANNELS), rnd.choice(CHANNELS), rnd.choice(MAPS),
                       rnd.choice(MAPS), K, rnd.choice([1, 1, 1, 2, (1, 1), (1, 2)]),
                       rnd.choice([0, 1, 1, K // 2, K - 1, K, (1, 1), (0, 1), (K // 2, K // 2)]), rnd.choice([1, 1, 1, 2, (1, 1)]),
                       rnd.choice([1, 1, 1, 2]), rnd.random() < 0.2))
    return layers


def test_the_knobs_are_the_transcription_s():
    for name, value in ref.DEFAULTS.items():
        assert getattr(hip_ops, name) == value and type(getattr(hip_ops, name)) is type(value), name
    assert all(name in ref.DEFAULTS for s in SETTINGS for name in s) and {n for s in SETTINGS for n in s} == set(ref.DEFAULTS)


def test_fixed_layers_have_the_workgroups_their_routes_rest_on():
    wgs = lambda N, Ci, Co, H, W, pad: ref.wino4_workgroups(N, Ci, Co, H, W, pad)
    assert wgs(8, 32, 32, 96, 128, 1) == wgs(4, 64, 64, 96, 128, 1) == wgs(4, 51, 51, 98, 130, 0) == 192 >= hip_ops.WINO4_MIN_WORKGROUPS
    assert wgs(8, 51, 51, 66, 130, 0) == 256 and wgs(2, 64, 64, 96, 128, 1) == 96 and wgs(2, 16, 16, 16, 16, 1) == 2


@pytest.mark.parametrize("setting", SETTINGS, ids=["+".join(s) or "defaults" for s in SETTINGS])
def test_routes_and_predicates_match_the_transcription(setting, monkeypatch):
    for name, value in setting.items():
        monkeypatch.setattr(hip_ops, name, value)
    k = dict(ref.DEFAULTS, **setting)
    lib = _hip.lib()
    seen = {form: {"fwd": set(), "dgrad": set(), "wgrad": set()} for form in ("shared", "tasks")}
    for layer in _layers(1500, sorted(setting)[0] if setting else "defaults"):
        T, N, Ci, Co, H, W, K, stride, padding, dilation, groups, direct = layer
        tasks = T is not None
        groups = 1 if tasks else groups                 # the per-task form has none
        xs, ws = (N, Ci, H, W), ((T, Co, Ci, K, K) if tasks else (Co, Ci, K, K))
        x, w = Stand(*xs), Stand(*ws)
        conf = (stride, padding, dilation)
        want = ref.route(k, xs, ws, *conf, groups, direct)
        got = hip_ops.conv_route(xs, ws, *conf, groups, direct)
        assert (got.fwd, got.dgrad, got.wgrad) == want, (layer, got, want)
        plain = ref._one(stride, 1) and ref._one(dilation, 1) and groups == 1 and ref._pad(padding) >= 0
        assert (got.K, got.pad) == ((K, ref._pad(padding)) if plain else (None, None)), (layer, got)
        for key, value in zip(("fwd", "dgrad", "wgrad"), want):
            seen["tasks" if tasks else "shared"][key].add(value)

        # the public predicates: thin wrappers with their old results
        assert hip_ops.convk_eligible(x, w, *conf, groups, direct) == ref.convk_eligible(k, xs, ws, *conf, groups, direct), layer
        if tasks:
            for backward in (False, True):
                assert hip_ops.conv3x3_tasks_eligible(x, w, *conf, backward) == ref.conv3x3_tasks_eligible(k, xs, ws, *conf, backward), layer
            assert hip_ops.conv3x3_wgrad_tasks_eligible(x, w, *conf) == ref.conv3x3_wgrad_tasks_eligible(k, xs, ws, *conf), layer
        else:
            for backward in (False, True):
                assert hip_ops.conv3x3_eligible(x, w, *conf, groups, backward) == ref.conv3x3_eligible(k, xs, ws, *conf, groups, backward), layer
            assert hip_ops.conv3x3_wgrad_eligible(x, w, *conf, groups) == ref.conv3x3_wgrad_eligible(k, xs, ws, *conf, groups), layer
        Ho, Wo = H + 2 * (K // 2) - K + 1, W + 2 * (K // 2) - K + 1
        for n in (None, N):
            assert hip_ops.convk_wgrad_preferred(K, Ci, Co, Ho, Wo, direct, n) == ref.convk_wgrad_preferred(k, K, Ci, Co, Ho, Wo, direct, n), layer
        assert hip_ops._wgrad_wino(N, Ci, Co, Ho, Wo) == ref.wgrad_wino(k, N, Ci, Co, Ho, Wo), layer
        if isinstance(padding, int):
            eligible = ref.convk_reflect_eligible(k, xs, ws, padding)
            assert hip_ops.convk_reflect_eligible(x, w, padding) == eligible, layer
            if eligible:                # a mirrored border: the weight gradient stays with the direct kernels whatever their rule says
                mirrored = hip_ops.conv_route(xs, ws, 1, padding, 1, 1, False, True)
                assert (mirrored.fwd, mirrored.dgrad, mirrored.wgrad) == ref.route(k, xs, ws, 1, padding, 1, 1, False, True) \
                    == ("convk", "convk", "convk"), layer
        if K == 3 and padding in (0, 1):
            assert hip_ops.wino4_workgroups(N, Ci, Co, H, W, padding) == ref.wino4_workgroups(N, Ci, Co, H, W, padding), layer
            assert hip_ops.wino_form2(x, w, padding) == ref.wino_form2(k, xs, ws, padding), layer
            plan_ok = tasks and H * W >= 4 and int(lib.savfi_conv3x3_unit16_supported(N, T, Ci, Co, H, W, padding)) == 1
            assert hip_ops.conv3x3_unit16_supported(x, w, padding) == bool(ref.unit16_route(k, xs, ws, padding) and plan_ok), layer
            if tasks and H + 2 * padding - 2 > 0 and W + 2 * padding - 2 > 0:
                gy_shape = (N, Co, H + 2 * padding - 2, W + 2 * padding - 2)
                assert hip_ops.conv3x3_in_unit16_supported(gy_shape, w, padding) == \
                    (int(lib.savfi_conv3x3_in_unit16_supported(N, T, Ci, Co, *gy_shape[2:], padding)) == 1), layer

    # every route is reached in each form that can produce it -- the untransformed Winograd data gradient ('conv3x3') where the forward
    # thresholds lie above the backward ones
    if not setting:
        for form in seen.values():
            assert form == {"fwd": {"convk", "wino", "wino2", "aten"}, "dgrad": {"convk", "wino", "wino2", "aten"},
                            "wgrad": {"convk", "conv3x3", "aten"}}, seen
    if "WINO_MIN_TILES_FWD_BATCHED" in setting and len(setting) == 2:
        assert "conv3x3" in seen["shared"]["dgrad"], seen
    if setting == {"TASKS_MIN_TILES_FWD": FAR}:
        assert "conv3x3" in seen["tasks"]["dgrad"], seen


def test_a_map_that_is_not_on_the_device_routes_nowhere():
    """The device / dtype / rank precondition is the tensor's, not the route's: every predicate says no, whatever the layer."""
    w, wt = Stand(64, 64, 3, 3), Stand(4, 64, 64, 3, 3)
    assert hip_ops.conv3x3_eligible(Stand(8, 64, 96, 128), w, 1, 1, 1, 1)
    host, double, flat = Stand(8, 64, 96, 128), Stand(8, 64, 96, 128), Stand(64, 96, 128)
    host.is_cuda, double.dtype = False, torch.float64
    for x in (host, double, flat):
        assert not hip_ops.convk_eligible(x, w, 1, 1, 1) and not hip_ops.conv3x3_eligible(x, w, 1, 1, 1, 1)
        assert not hip_ops.conv3x3_wgrad_eligible(x, w, 1, 1, 1, 1) and not hip_ops.conv3x3_tasks_eligible(x, wt, 1, 1, 1)
        assert not hip_ops.conv3x3_wgrad_tasks_eligible(x, wt, 1, 1, 1) and not hip_ops.conv3x3_unit16_supported(x, wt, 1)
