"""Writes tests/golden/dain_net.npz: what pins the restatements of tests/dain_net_ref.py to the reference's own DAIN modules.

Needs the reference checkout (argument: its root); runs on the host.  It loads the reference's pure-torch files by path --
dain/MegaDepth/pytorch_DIW_scratch.py, dain/S2D_models/S2DF.py and dain/Resblock/BasicBlock.py with the reference's model_utils,
dain/loss_function.py, dain/networks/DAIN.py with stand-ins in sys.modules for its compiled extensions, its flow estimator and its option
parser --, fills them with the numpy-rule weights of tests/dain_net_ref.py and runs them on the CPU in float32 and float64.

The file holds key names, shapes and small arrays only (no weights): the 779 hourglass names and shapes, the names and shapes of the other
nets, outputs at 2x3x16x16 and 2x3x64x64 in train() and eval() mode, the running buffers after one and after two training forwards,
and the loss and the ten rectify gradients on a 1x437x16x16 input.

    python tools/gen_dain_golden.py /path/to/reference
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from tests import dain_net_ref as R  # noqa: E402

SEED = 4100
SIZES = (16, 64)


def load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def reference_modules(root):
    d = os.path.join(root, 'dain')
    load('model_utils', os.path.join(root, 'model_utils.py'))
    hg = load('ref_hourglass', os.path.join(d, 'MegaDepth', 'pytorch_DIW_scratch.py'))
    s2d = load('ref_s2df', os.path.join(d, 'S2D_models', 'S2DF.py'))
    res = load('ref_resblock', os.path.join(d, 'Resblock', 'BasicBlock.py'))
    loss = load('dain.loss_function', os.path.join(d, 'loss_function.py'))
    stack = load('dain.Stack', os.path.join(d, 'Stack.py'))
    pkg = types.ModuleType('dain')
    pkg.__path__ = []
    sys.modules['dain'] = pkg
    for name, attrs in (('dain.my_package', ()), ('dain.my_package.FilterInterpolation', ('FilterInterpolationModule',)),
                        ('dain.my_package.FlowProjection', ('FlowProjectionModule',)),
                        ('dain.my_package.DepthFlowProjection', ('DepthFlowProjectionModule',))):
        m = types.ModuleType(name)
        m.__path__ = []
        for a in attrs:
            setattr(m, a, None)            # the compiled extensions: never called here
        sys.modules[name] = m
    pwc = types.ModuleType('dain.PWCNet')
    pwc.pwc_dc_net = lambda path=None: nn.Module()
    mega = types.ModuleType('dain.MegaDepth')
    mega.HourGlass = lambda pretrained=None: hg.pytorch_DIW_scratch
    for name, m in (('dain.PWCNet', pwc), ('dain.MegaDepth', mega), ('dain.S2D_models', s2d), ('dain.Resblock', res)):
        sys.modules[name] = m
        setattr(pkg, name.split('.')[1], m)
    pkg.loss_function, pkg.Stack = loss, stack
    dain = load('ref_dain', os.path.join(d, 'networks', 'DAIN.py'))
    return hg, s2d, res, loss, dain


def fill(module, state):
    own = module.state_dict()
    assert set(own) == set(state), sorted(set(own) ^ set(state))[:10]
    module.load_state_dict({k: v.clone() for k, v in state.items()}, strict=True)


def main(root):
    torch.set_num_threads(1)          # one summation order on the host, whatever the machine's cores (the test does the same)
    hg_mod, s2d_mod, res_mod, loss_mod, dain_mod = reference_modules(root)
    out = {}
    torch.manual_seed(0)
    net = dain_mod.MetaDAIN(training=False, resume=False)
    ref_sd = {k: v for k, v in net.state_dict().items() if not k.startswith('flownets.')}
    out['metadain_keys'] = np.array(list(ref_sd))
    out['metadain_shapes'] = np.array([','.join(str(s) for s in v.shape) for v in ref_sd.values()])
    hg = hg_mod.pytorch_DIW_scratch
    out['hourglass_keys'] = np.array(list(hg.state_dict()))
    out['hourglass_shapes'] = np.array([','.join(str(s) for s in v.shape) for v in hg.state_dict().values()])
    assert [k for k, p in net.named_parameters() if 'rectifyNet' in k] == ['rectifyNet.' + k for k in R.RECTIFY_NAMES]

    hg_state = R.numpy_rule_state(R.hourglass_shapes(), SEED)
    ctx_state = R.numpy_rule_state(R.s2df_shapes(), SEED + 1)
    filt_state = R.numpy_rule_state(R.filternet_shapes(), SEED + 2)
    rect_state = R.numpy_rule_state(R.rectify_shapes(), SEED + 3)

    for dtype, tag in ((torch.float32, 'f32'), (torch.float64, 'f64')):
        for size in SIZES:
            x = R.numpy_rule_frames((2, 3, size, size), SEED + 10 + size).to(dtype)
            # hourglass: train (one, then a second forward: the running buffers after each), eval
            hg.to(dtype)
            fill(hg, {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in hg_state.items()})
            hg.train()
            with torch.no_grad():
                y1 = hg(x)
                after1 = {k: v.clone() for k, v in hg.state_dict().items()}
                y2 = hg(x.flip(0) * 0.5)
                after2 = {k: v.clone() for k, v in hg.state_dict().items()}
            out['hg_train_%s_%d' % (tag, size)] = R.golden_view('hg', size, y1.numpy())
            out['hg_train2_%s_%d' % (tag, size)] = R.golden_view('hg', size, y2.numpy())
            for name, state in (('after1', after1), ('after2', after2)):
                for key in R.GOLDEN_BUFFERS:
                    out['hg_%s_%s_%d_%s' % (name, tag, size, key)] = state[key].numpy()
                out['hg_%s_%s_%d_sum_mean' % (name, tag, size)] = np.array(
                    sum(float(v.double().sum()) for k, v in state.items() if k.endswith('running_mean')))
                out['hg_%s_%s_%d_sum_var' % (name, tag, size)] = np.array(
                    sum(float(v.double().sum()) for k, v in state.items() if k.endswith('running_var')))
            fill(hg, {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in hg_state.items()})
            hg.eval()
            with torch.no_grad():
                out['hg_eval_%s_%d' % (tag, size)] = R.golden_view('hg', size, hg(x).numpy())
            # context net
            ctx = net.ctxNet.to(dtype)
            fill(ctx, {k: v.to(dtype) for k, v in ctx_state.items()})
            with torch.no_grad():
                y = ctx(x).numpy()
            assert np.array_equal(y[:, :3], x.numpy())                             # (the first three channels are the frame)
            out['ctx_%s_%d' % (tag, size)] = R.golden_view('ctx', size, y)
            out['ctx_sum_%s_%d' % (tag, size)] = np.array(y.astype(np.float64).sum())
        # filter net: 64 is the smallest side its five pools admit with the padding rule; 32 is the smallest they admit at all
        for size in (32, 64):
            x6 = R.numpy_rule_frames((2, 6, size, size), SEED + 20 + size).to(dtype)
            net.to(dtype)
            own = net.state_dict()
            own.update({k: v.to(dtype) for k, v in filt_state.items()})
            net.load_state_dict(own)
            with torch.no_grad():
                trunk = net.forward_singlePath(net.initScaleNets_filter, x6, 'filter')
                h1 = net.forward_singlePath(net.initScaleNets_filter1, trunk, name=None)
                h2 = net.forward_singlePath(net.initScaleNets_filter2, trunk, name=None)
            heads = torch.stack((h1, h2)).numpy()
            out['filter_heads_%s_%d' % (tag, size)] = R.golden_view('heads', size, heads)
            out['filter_heads_sum_%s_%d' % (tag, size)] = np.array(heads.astype(np.float64).sum())
        # rectify net + Charbonnier loss on a 1x437x16x16 input
        rect = net.rectifyNet.to(dtype)
        fill(rect, {k: v.to(dtype) for k, v in rect_state.items()})
        ri = (R.numpy_rule_frames((1, 437, 16, 16), SEED + 30) - 0.5).to(dtype)
        cur = R.numpy_rule_frames((1, 3, 16, 16), SEED + 31).to(dtype)
        tgt = R.numpy_rule_frames((1, 3, 16, 16), SEED + 32).to(dtype)
        tgt[0, 0, 0, :4] = (rect(ri) + cur).detach()[0, 0, 0, :4]                 # a few differences that are exactly 0
        frame = rect(ri) + cur
        loss = loss_mod.charbonier_loss(frame - tgt, 1e-8)
        grads = torch.autograd.grad(loss, [dict(rect.named_parameters())[k] for k in R.RECTIFY_NAMES])
        out['rect_frame_%s' % tag], out['rect_loss_%s' % tag] = frame.detach().numpy(), loss.detach().numpy()
        out['rect_target_%s' % tag] = tgt.numpy()
        for k, g in zip(R.RECTIFY_NAMES, grads):
            # a gradient is as large as its weight: its sum, its absolute sum and its first values are what is kept
            flat = g.double().flatten()
            out['rect_grad_%s_%s' % (tag, k)] = np.concatenate(([float(flat.sum()), float(flat.abs().sum())], flat[:32].numpy()))
    path = os.path.join(REPO, 'tests', 'golden', 'dain_net.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes,', len(out), 'arrays')


if __name__ == '__main__':
    main(sys.argv[1])
