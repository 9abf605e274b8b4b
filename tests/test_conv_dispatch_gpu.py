"""-m gpu: which kernels hip_ops.conv_bias_act / conv_bias_act_tasks launch, and in which order, over the routing table of the fused
convolutions -- one small case per route of the forward, the data gradient, the weight gradient and the bias gradient, in both forms.

EXPECTED holds each case's forward and backward launch-name sequences as the commit before the routing was folded into one function
(hip_ops.conv_route) produced them: the file passes unchanged on both trees.  A launch name is what bench.py's timers key on; the ATen
(MIOpen) convolutions launch nothing through _hip.launch, so a direction that stays there shows as the absence of a name.

Every case also compares y, gx, gw and gb with float64 conv2d autograd on the whole map.  A quantity that a savfi kernel made is held to
the local gate of tests/conv_ref.py with the family constants of test_conv_layers_gpu.py / test_conv_variants_gpu.py (the family is read
from the launch name); one that ATen made to the 1e-6 of test_hip_ops_gpu.test_conv_bias_act_matches_unfused_torch.  The
bias gradient is summed by a savfi kernel on every route: the bias family's constant."""
import pytest
import torch
import torch.nn.functional as F

from meta_interpolation_amd import hip_ops
from tests import conv_ref as R
from tests.helpers import record_launches
from tests import test_conv_layers_gpu as L
from tests import test_conv_variants_gpu as V

pytestmark = pytest.mark.gpu

DEV = "cuda"
C_FAMILY = dict(L.C_FAMILY, f4=V.C_F4, f2=V.C_F2)
ATEN_TOL = 1e-6


def _case(T, N, Ci, Co, H, W, K=3, pad=1, stride=1, slope=0.0, **kw):
    return dict(dict(T=T, N=N, Ci=Ci, Co=Co, H=H, W=W, K=K, pad=pad, stride=stride, slope=slope, direct=False, reflect=False, in_slope=None,
                     defer=False, bias=True, need_x=True, overlap=False, out_unit16=0), **kw)


# T = None: shared weights (conv_bias_act); else conv_bias_act_tasks
CASES = {
    "shared-aten": _case(None, 1, 8, 8, 16, 16),
    "shared-stride2": _case(None, 2, 16, 16, 32, 32, stride=2),
    "shared-f2": _case(None, 2, 16, 16, 16, 16),
    "shared-f4": _case(None, 8, 32, 32, 96, 128),
    "shared-f4-overlap": _case(None, 8, 32, 32, 96, 128, overlap=True),
    "shared-wgrad-wino": _case(None, 8, 256, 256, 24, 32),
    "shared-convk-relu": _case(None, 1, 64, 64, 32, 32, slope=0.0),
    "shared-convk-linear": _case(None, 1, 64, 64, 32, 32, slope=1.0),
    "shared-5x5-masked": _case(None, 1, 6, 16, 24, 24, K=5, pad=2, in_slope=0.0),
    "shared-direct": _case(None, 1, 8, 8, 8, 8, direct=True),
    "shared-reflect": _case(None, 1, 8, 8, 32, 32, reflect=True),
    "shared-f4-masked": _case(None, 4, 64, 64, 96, 128, in_slope=0.0),
    "shared-convk-masked": _case(None, 1, 64, 64, 32, 32, in_slope=0.0),
    "shared-f2-defer": _case(None, 2, 16, 16, 16, 16, defer=True),
    "shared-f2-nobias": _case(None, 2, 16, 16, 16, 16, bias=False),
    "shared-f2-no-gx": _case(None, 2, 16, 16, 16, 16, need_x=False),
    "shared-aten-overlap": _case(None, 1, 8, 8, 16, 16, overlap=True),
    "tasks-stride2-grouped": _case(2, 2, 8, 8, 8, 8, stride=2),
    "tasks-stride2-per-task": _case(2, 2, 8, 8, 64, 64, stride=2),
    "tasks-f2": _case(2, 4, 16, 16, 16, 16),
    "tasks-f4": _case(4, 8, 32, 32, 96, 128),
    "tasks-f4-overlap": _case(4, 8, 32, 32, 96, 128, overlap=True),
    "tasks-wgrad-wino-linear": _case(4, 8, 256, 256, 24, 32, slope=1.0),
    "tasks-wgrad-wino-relu": _case(4, 8, 256, 256, 24, 32, slope=0.0),
    "tasks-convk-linear": _case(2, 2, 64, 64, 32, 32, slope=1.0),
    "tasks-5x5": _case(3, 3, 6, 16, 20, 24, K=5, pad=2),
    "tasks-unit16": _case(4, 8, 51, 51, 66, 130, pad=0, slope=1.0, out_unit16=1),
}

# case -> (forward launches, backward launches), recorded on the commit before conv_route
EXPECTED = {
    "shared-aten": (["bias_act_fwd"], ["bias_act_bwd"]),
    "shared-stride2": (["bias_act_fwd"], ["bias_act_bwd"]),
    "shared-f2": (["conv3x3_filters", "conv3x3_fwd"], ["bias_act_bwd", "conv3x3_bwd_data"]),
    "shared-f4": (["conv3x3_filters", "conv3x3f4_fwd"], ["bias_act_bwd", "conv3x3f4_bwd_data", "conv3x3_wgrad"]),
    "shared-f4-overlap": (["conv3x3_filters", "conv3x3f4_fwd"], ["bias_act_bwd", "conv3x3f4_bwd_data", "conv3x3_wgrad"]),
    "shared-wgrad-wino": (["conv3x3_filters", "conv3x3f4_fwd"], ["bias_act_bwd", "conv3x3f4_bwd_data", "conv3x3_wgrad"]),
    "shared-convk-relu": (["convk_filters", "convk_fwd"], ["bias_act_bwd", "convk_bwd_data", "convk_wgrad"]),
    "shared-convk-linear": (["convk_filters", "convk_fwd"], ["convk_bwd_data", "convk_wgrad"]),
    "shared-5x5-masked": (["convk_filters", "convk_fwd"], ["bias_act_bwd", "convk_bwd_data", "bias_act_bwd", "convk_wgrad"]),
    "shared-direct": (["convk_filters", "convk_fwd"], ["bias_act_bwd", "convk_bwd_data", "convk_wgrad"]),
    "shared-reflect": (["convk_filters", "convk_fwd"], ["bias_act_bwd", "convk_bwd_data", "reflect_pad_bwd", "convk_wgrad"]),
    "shared-f4-masked": (["conv3x3_filters", "conv3x3f4_fwd"], ["bias_act_bwd", "conv3x3f4_bwd_data", "convk_wgrad"]),
    "shared-convk-masked": (["convk_filters", "convk_fwd"], ["bias_act_bwd", "convk_bwd_data", "convk_wgrad"]),
    "shared-f2-defer": (["conv3x3_filters", "conv3x3_fwd"], ["bias_act_bwd", "conv3x3_bwd_data"]),
    "shared-f2-nobias": (["conv3x3_filters", "conv3x3_fwd"], ["bias_act_bwd", "conv3x3_bwd_data"]),
    "shared-f2-no-gx": (["conv3x3_filters", "conv3x3_fwd"], ["bias_act_bwd"]),
    "shared-aten-overlap": (["bias_act_fwd"], ["bias_act_bwd"]),
    "tasks-stride2-grouped": (["bias_act_fwd"], ["bias_act_bwd"]),
    "tasks-stride2-per-task": (["bias_act_fwd"], ["bias_act_bwd"]),
    "tasks-f2": (["conv3x3_filters", "conv3x3_fwd"], ["bias_act_bwd", "conv3x3_bwd_data"]),
    "tasks-f4": (["conv3x3_filters", "conv3x3f4_fwd"], ["bias_act_bwd", "conv3x3f4_bwd_data", "conv3x3_wgrad"]),
    "tasks-f4-overlap": (["conv3x3_filters", "conv3x3f4_fwd"], ["bias_act_bwd", "conv3x3f4_bwd_data", "conv3x3_wgrad"]),
    "tasks-wgrad-wino-linear": (["conv3x3_filters", "conv3x3f4_fwd"], ["conv3x3f4_bwd_data", "conv3x3_wgrad"]),
    "tasks-wgrad-wino-relu": (["conv3x3_filters", "conv3x3f4_fwd"], ["bias_act_bwd", "conv3x3f4_bwd_data", "conv3x3_wgrad"]),
    "tasks-convk-linear": (["convk_filters", "convk_fwd"], ["convk_bwd_data", "convk_wgrad"]),
    "tasks-5x5": (["convk_filters", "convk_fwd"], ["bias_act_bwd", "convk_bwd_data", "convk_wgrad"]),
    "tasks-unit16": (["conv3x3_filters", "conv3x3f4_fwd"], ["conv3x3f4_bwd_data", "convk_wgrad"]),
}

_RUNS = {}


def _run(name):
    """One forward + backward of the case on the GPU, launches captured; kept for the cases that compare two runs."""
    if name in _RUNS:
        return _RUNS[name]
    c = CASES[name]
    T, N, Ci, Co, K = c["T"], c["N"], c["Ci"], c["Co"], c["K"]
    g = torch.Generator(device=DEV).manual_seed(sorted(CASES).index(name.replace("-overlap", "")))
    x = torch.randn(N, Ci, c["H"], c["W"], device=DEV, generator=g)
    if c["in_slope"] is not None:
        x = torch.relu(x)               # the activated output of a producer that left its derivative to this layer
    w = torch.randn((T or 1, Co, Ci, K, K), device=DEV, generator=g) / (K * Ci ** 0.5)
    b = 0.1 * torch.randn(T or 1, Co, device=DEV, generator=g) if c["bias"] else None
    xr = x.clone().requires_grad_(c["need_x"])
    wr = (w if T else w[0]).clone().requires_grad_()
    br = None if b is None else (b if T else b[0]).clone().requires_grad_()
    hip_ops.set_weight_gradient_overlap(c["overlap"])
    try:
        with record_launches() as rec:
            names = rec.names
            if T:
                y = hip_ops.conv_bias_act_tasks(xr, wr, br, c["stride"], c["pad"], 1, c["slope"], direct=c["direct"], in_slope=c["in_slope"],
                                                defer=c["defer"], out_unit16=c["out_unit16"])
            else:
                y = hip_ops.conv_bias_act(xr, wr, br, c["stride"], c["pad"], 1, 1, c["slope"], direct=c["direct"], reflect=c["reflect"],
                                          in_slope=c["in_slope"], defer=c["defer"])
            n_fwd = len(names)
            gy = torch.randn(y.shape, device=DEV, generator=g)
            inputs = ([xr] if c["need_x"] else []) + [wr] + ([br] if br is not None else [])
            grads = list(torch.autograd.grad(y, inputs, gy))
            hip_ops.join_weight_gradients()
            torch.cuda.synchronize()
    finally:
        hip_ops.set_weight_gradient_overlap(False)
    y = y.detach()
    if c["out_unit16"]:         # the memory is [N][Ho][Wo/16][Co][16] under the shape [N,Co,Ho,Wo]
        Ho, Wo = y.shape[2:]
        y = y.reshape(N, Ho, Wo // 16, Co, 16).permute(0, 3, 1, 2, 4).reshape(N, Co, Ho, Wo).contiguous()
    gx = grads.pop(0) if c["need_x"] else None
    gw = grads.pop(0).reshape(w.shape)
    gb = grads.pop(0).reshape(T or 1, Co) if br is not None else None
    _RUNS[name] = dict(x=x, w=w, b=b, gy=gy, y=y, gx=gx, gw=gw, gb=gb, fwd=names[:n_fwd], bwd=names[n_fwd:])
    return _RUNS[name]


def _family(names, suffixes):
    """Kernel family of the launch that made a quantity (None: ATen), from its timer name."""
    families = {"conv3x3f4": "f4", "conv3x3": "f2", "convk": "convk"}
    made = [families[n.split("_")[0]] for n in names if n.endswith(suffixes) and n.split("_")[0] in families]
    assert len(made) <= 1, names
    return made[0] if made else None


def _check(what, got, ref, mag, family, tol=ATEN_TOL):
    got = got.cpu()
    if family is None:
        err = (got.double() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-12)
        print("%-14s ATen    rel %.3g (gate %g)" % (what, err, tol))
        assert err < tol, (what, err)
        return
    if family in ("f4", "f2"):
        mag = R.pool7(mag)
    print("%-14s %-13s local %.3g (gate %g)" % (what, family, R.local_ratio(got, ref, mag), C_FAMILY[family]))
    R.assert_local(got, ref, mag, C_FAMILY[family], family, what)


@pytest.mark.parametrize("name", list(CASES))
def test_launch_sequence_and_values(name):
    c, r = CASES[name], _run(name)
    T, slope, pad = c["T"] or 1, c["slope"], c["pad"]
    print("%s: forward %r backward %r" % (name, r["fwd"], r["bwd"]))
    assert (r["fwd"], r["bwd"]) == EXPECTED[name]
    if c["overlap"]:            # the side stream changes where the weight gradient runs, not one bit of any result
        base = _run(name.replace("-overlap", ""))
        for k in ("y", "gx", "gw", "gb"):
            assert torch.equal(r[k], base[k]), k
        return

    # float64 on the CPU, per task: z = conv(x, w) + b and its magnitude, then the three gradients for the cotangent of z
    x, w, y, gy = r["x"].double().cpu(), r["w"].double().cpu(), r["y"].cpu(), r["gy"].double().cpu()
    b = None if r["b"] is None else r["b"].double().cpu()
    gz = gy if (slope == 1.0 or c["defer"]) else gy * R.mask_factor(y.double(), slope)
    ref = {k: [None] * T for k in ("y", "ymag", "gx", "gxmag", "gw", "gwmag")}
    for t in range(T):
        for tag, absolute in (("", False), ("mag", True)):
            f = torch.abs if absolute else (lambda v: v)
            xt, wt = f(x[t::T]).requires_grad_(), f(w[t]).requires_grad_()
            xp = F.pad(xt, (pad,) * 4, mode="reflect") if c["reflect"] else xt
            z = F.conv2d(xp, wt, None if b is None else f(b[t]), c["stride"], 0 if c["reflect"] else pad)
            ref["y" + tag][t] = z.detach() if absolute else R.act(z.detach(), slope)
            ref["gx" + tag][t], ref["gw" + tag][t] = torch.autograd.grad(z, (xt, wt), f(gz[t::T]))
    interleave = lambda parts: torch.stack(parts, 1).reshape((-1,) + tuple(parts[0].shape[1:]))
    _check("y", r["y"], interleave(ref["y"]), interleave(ref["ymag"]), _family(r["fwd"], ("_fwd",)))
    if c["need_x"]:
        gx_ref, gx_mag = interleave(ref["gx"]), interleave(ref["gxmag"])
        if c["in_slope"] is not None:
            gx_ref = gx_ref * R.mask_factor(x, c["in_slope"])
        _check("gx", r["gx"], gx_ref, gx_mag, _family(r["bwd"], ("_bwd_data",)))
    wfam = "convk_wgrad" if "convk_wgrad" in r["bwd"] else ("conv3x3_wgrad" if "conv3x3_wgrad" in r["bwd"] else None)
    _check("gw", r["gw"], torch.stack(ref["gw"]), torch.stack(ref["gwmag"]), wfam)
    if b is not None:
        gzt = torch.stack([gz[t::T] for t in range(T)])
        _check("gb", r["gb"], gzt.sum((1, 3, 4)), gzt.abs().sum((1, 3, 4)), "bias")
