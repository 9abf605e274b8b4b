"""-m gpu: where a fused convolution gets its packed / transformed filters from, seen as launch names -- the filters made with the
fast weights of an update, the ones a module keeps for its own weight, the ones of a registered constant weight.

EXPECTED holds each scenario's launch-name sequences (bench.py's timer names, captured as in test_conv_dispatch_gpu.py) as the code
before the filter store was gathered into one lookup issues them: each layer's kernels are those test_conv_dispatch_gpu.py recorded on
that code for the same shapes, the filter launches among them follow from its lookup functions (transcribed in tests/filter_store_ref.py).
The file is written to pass unchanged on both trees.

The layers are the smallest that reach each kind of filter ('convk': packed for the direct kernel, 'wino2': the F(2x2) transform), shared
weights and a per-task (T = 2) copy.  Every pass compares y and gx with float64 conv2d through the local gate of tests/conv_ref.py with
the family constants of test_conv_dispatch_gpu.py -- in particular a pass after the weight changed must follow the new weight."""
import contextlib

import pytest
import torch

from meta_interpolation_amd import _hip, hip_ops, model_utils
from tests import conv_ref as R
from tests import test_conv_dispatch_gpu as D
from tests.helpers import record_launches

pytestmark = pytest.mark.gpu

DEV = "cuda"
SLOPE = 0.0

# name: (T, N, Ci, Co, H, W, K, pad); T = None: shared weights
LAYERS = {
    "convk3": (None, 1, 64, 64, 32, 32, 3, 1),
    "f2": (None, 2, 16, 16, 16, 16, 3, 1),
    "convk5": (None, 1, 6, 16, 24, 24, 5, 2),
    "tasks-convk3": (2, 2, 64, 64, 32, 32, 3, 1),
    "tasks-f2": (2, 4, 16, 16, 16, 16, 3, 1),
}

_FWD3 = ["conv3x3_fwd", "bias_act_bwd", "conv3x3_bwd_data"]
_FWDK = ["convk_fwd", "bias_act_bwd", "convk_bwd_data", "convk_wgrad"]
_PASS = {"convk3": _FWDK, "f2": _FWD3, "convk5": _FWDK, "tasks-convk3": _FWDK, "tasks-f2": _FWD3}
_SINGLE = {"convk3": "convk_filters", "f2": "conv3x3_filters", "convk5": "convk_filters", "tasks-convk3": "convk_filters",
           "tasks-f2": "conv3x3_filters"}


def _passes(names, single=()):
    """The launches of one pass over `names`; the layers in `single` make their own filters first."""
    return [n for name in names for n in ([_SINGLE[name]] if name in single else []) + _PASS[name]]


# scenario -> the launches of each of its stages
EXPECTED = {
    "update": [
        ["mt_update"] + _passes(LAYERS, single=LAYERS),
        ["mt_update", "convk_filters_multi", "conv3x3_filters_multi"] + _passes(LAYERS),
        ["mt_update", "convk_filters_multi", "conv3x3_filters_multi"] + _passes(LAYERS),
    ],
    "module": [
        _passes(["convk3", "f2", "convk5"], single=["convk3", "f2", "convk5"]),
        _passes(["convk3", "f2", "convk5"]),
        ["convk_filters_multi", "conv3x3_filters_multi"],
        _passes(["convk3", "f2", "convk5"]),
        _passes(["convk3", "f2", "convk5"], single=["convk3", "f2", "convk5"]),
    ],
    "const": [
        ["convk_filters", "convk_fwd", "conv3x3_filters", "conv3x3_fwd"],
        ["convk_filters", "convk_fwd", "bias_act_bwd", "convk_bwd_data", "conv3x3_filters", "conv3x3_fwd", "bias_act_bwd", "conv3x3_bwd_data"],
        ["convk_fwd", "bias_act_bwd", "convk_bwd_data", "conv3x3_fwd", "bias_act_bwd", "conv3x3_bwd_data"],
        ["convk_filters", "convk_fwd", "bias_act_bwd", "convk_bwd_data", "conv3x3_filters", "conv3x3_fwd", "bias_act_bwd", "conv3x3_bwd_data"],
    ],
}


@contextlib.contextmanager
def _Record():
    """The names of every launch through _hip.launch while the block runs."""
    with record_launches() as rec:
        yield rec.names


def _reset():
    hip_ops.filters_after_update([])        # no prepared filters, no newest update
    hip_ops._pack_plans.clear()


def _tensors(seed):
    """Per layer: x, w, b and a cotangent, seeded."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    out = {}
    for name, (T, N, Ci, Co, H, W, K, pad) in LAYERS.items():
        lead = () if T is None else (T,)
        out[name] = dict(x=torch.randn(N, Ci, H, W, device=DEV, generator=g),
                         w=torch.randn(lead + (Co, Ci, K, K), device=DEV, generator=g) / (K * Ci ** 0.5),
                         b=0.1 * torch.randn(lead + (Co,), device=DEV, generator=g),
                         gy=torch.randn(N, Co, H + 2 * pad - K + 1, W + 2 * pad - K + 1, device=DEV, generator=g))
    return out


def _pass(name, x, w, b, gy, cache=None, backward=True):
    """One forward (and backward) of the layer on the GPU, y and gx held to float64; returns the gradients of (w, b) where they ask."""
    T, N, Ci, Co, H, W, K, pad = LAYERS[name]
    with _Record() as names:
        xr = x.clone().requires_grad_(backward)
        if T is None:
            y = hip_ops.conv_bias_act(xr, w, b, 1, pad, 1, 1, SLOPE, False, cache)
        else:
            y = hip_ops.conv_bias_act_tasks(xr, w, b, 1, pad, 1, SLOPE)
        n_fwd = len(names)
        grads = None
        if backward:
            inputs = [xr] + [t for t in (w, b) if t.requires_grad]
            grads = torch.autograd.grad(y, inputs, gy)
        torch.cuda.synchronize()
    w5 = (w if T else w[None]).detach().cpu()
    b2 = (b if T else b[None]).detach().cpu()
    ref, mag = R.conv_tasks64(x.cpu(), w5, pad, T or 1, bias=b2)
    y = y.detach().cpu()
    D._check(name + " y", y, R.act(ref, SLOPE), mag, D._family(names[:n_fwd], ("_fwd",)))
    if backward:
        gz = gy.double().cpu() * R.mask_factor(y.double(), SLOPE)
        gref, gmag = R.dgrad_tasks64(gz, w5, pad, T or 1)
        D._check(name + " gx", grads[0], gref, gmag, D._family(names[n_fwd:], ("_bwd_data",)))
    return None if grads is None else list(grads[1:])


def _filter_launches(names):
    return [n for n in names if "_filters" in n]


def _expect(scenario, stages):
    for i, names in enumerate(stages):
        print("%s[%d]: %r" % (scenario, i, names))
    assert stages == EXPECTED[scenario]


def test_fast_weights_of_an_update_get_their_filters_in_one_launch_per_kind_from_the_second_step():
    """Three inner steps of mt_update, every layer forward and backward on each step's fast weights."""
    _reset()
    ts = _tensors(31)
    order = list(LAYERS)
    fast = [t for name in order for t in (ts[name]["w"].clone().requires_grad_(), ts[name]["b"].clone().requires_grad_())]
    grads = [0.1 * torch.randn_like(t) for t in fast]
    lrs = [torch.tensor(1e-2, device=DEV) for _ in fast]
    stages = []
    try:
        for step in range(3):
            with _Record() as names:
                fast = hip_ops.mt_update(_hip.RULE_SGD, _hip.LR_SCALAR, fast, grads, lrs)
                grads = []
                for i, name in enumerate(order):
                    t = ts[name]
                    grads += [g.detach() for g in _pass(name, t["x"], fast[2 * i], fast[2 * i + 1], t["gy"])]
            stages.append(names)
    finally:
        _reset()
    _expect("update", stages)
    assert sorted(_filter_launches(stages[0])) == sorted(_SINGLE.values())
    for later in stages[1:]:
        assert _filter_launches(later) == ["convk_filters_multi", "conv3x3_filters_multi"]


def test_a_module_s_own_weight_keeps_its_filters_per_version_and_refresh_remakes_them_in_one_launch_per_kind():
    _reset()
    ts = _tensors(32)
    order = ["convk3", "f2", "convk5"]
    mods = {}
    for name in order:
        T, N, Ci, Co, H, W, K, pad = LAYERS[name]
        m = mods[name] = model_utils.MetaConv2dLayer(Ci, Co, K, 1, pad).to(DEV)
        with torch.no_grad():
            m.weight.copy_(ts[name]["w"])
            m.bias.copy_(ts[name]["b"])

    def run():
        with _Record() as names:
            for name in order:
                m, t = mods[name], ts[name]
                _pass(name, t["x"], m.weight, m.bias, t["gy"], cache=m._filters)
        return names

    def change():
        with torch.no_grad():
            for m in mods.values():
                m.weight.mul_(1.5)
                m.bias.add_(0.1)
    try:
        stages = [run(), run()]
        change()
        with _Record() as names:
            hip_ops.refresh_module_filters(list(mods.values()))
        stages += [names, run()]            # this pass reads the refreshed filters: its values follow the new weight
        change()
        stages.append(run())                # no refresh: every layer finds its weight changed and makes its own
    finally:
        _reset()
    _expect("module", stages)
    assert not _filter_launches(stages[1]) and not _filter_launches(stages[3])


def test_a_registered_constant_weight_gets_each_filter_once_per_stream_until_it_is_unregistered():
    _reset()
    ts = _tensors(33)
    order = ["tasks-convk3", "tasks-f2"]

    def run(backward):
        with _Record() as names:
            for name in order:
                t = ts[name]
                _pass(name, t["x"], t["w"], t["b"], t["gy"], backward=backward)
        return names
    try:
        for name in order:
            hip_ops.register_const_weight(ts[name]["w"])
        stages = [run(False), run(True), run(True)]     # forward filters, then the data gradient's only, then nothing
        for name in order:
            hip_ops.unregister_const_weight(ts[name]["w"])
        stages.append(run(True))
    finally:
        for name in order:
            hip_ops.unregister_const_weight(ts[name]["w"])
        _reset()
    _expect("const", stages)
    assert not _filter_launches(stages[2])
