"""Shared by the second-order system comparisons of the warps (tests/test_warp2_system_gpu.py) and the CPU test of their conditioning
(tests/test_warp2_ref_cpu.py): the case, the weights, and the oracle's run.

The case is the one of test_second_order_voxelflow_matches_oracle: 1 task, 64 x 64, SGD, 1*MSE, 2 inner steps, second order, and its
gate (5e-5 relative on the loss, fingerprints to 2e-3 of their abs-sum).  Comparing float32 on the device with float32 on the CPU is
only a test where the problem is well conditioned: second derivatives of a chaotic flow field amplify the rounding of either side.  With
the seeded default weights the oracle's own float32 and float64 runs are 3.4e-4 apart on RRIN's outer gradients (a sixth of the gate) and
1.6e-2 on Super SloMo's (eight gates).  So the last convolutions of the flow heads are scaled -- RRIN's by 0.5, Super SloMo's by 0.25 --
in the state dict BOTH sides get; float32 and float64 are then 5e-6 and 4e-7 apart, and the CPU suite asserts a quarter of the gate.

The device runs happen in ONE child process with a convolution-library database of its own (`python -m tests.warp2_system`): a
second-order pass sends every convolution through the library's solver search, and what that search leaves behind -- in the process
and in the database the suite shares -- moved the bits of a later first-order SepConv pass by one unit in the last place
(tests/test_wino4_lane_exchange_gpu.py, which passes alone and in the suite without these runs)."""
import functools
import json
import os
import subprocess
import sys
import tempfile

import torch

from meta_interpolation_amd import synthetic
from oracle import meta as ometa, rules as orules
from tests.helpers import fp, oracle_base

OVER = dict(optimizer='SGD', inner_lr=1e-2, loss='1*MSE', number_of_training_steps_per_iter=2,
            number_of_evaluation_steps_per_iter=2, second_order=True, first_order_to_second_order_epoch=-1)
LOSS_GATE, FP_GATE = 5e-5, 2e-3
RECIPE = {'voxelflow': 'smooth', 'rrin': None, 'superslomo': None}
# the last convolution of every sub-network that puts out a flow, and what it is scaled by
FLOW_HEADS = {'voxelflow': (), 'rrin': ('Flow_L.last', 'refine_flow.last'), 'superslomo': ('flowComp.conv3', 'arbTimeFlowIntrp.conv3')}
HEAD_SCALE = {'voxelflow': 1.0, 'rrin': 0.5, 'superslomo': 0.25}


def scale_flow_heads(model, named):
    """in place, on {name: tensor}: the oracle's base or dict(net.named_parameters()) of the product's plugin"""
    with torch.no_grad():
        for head in FLOW_HEADS[model]:
            for suffix in ('.weight', '.bias'):
                named[head + suffix].mul_(HEAD_SCALE[model])


def frames(model):
    return synthetic.septuplet_batch(1, 64, 64, model=model)


def _oracle(model, dtype, forward_kwargs):
    base = oracle_base(model, recipe=RECIPE[model])
    scale_flow_heads(model, base)
    base = {n: (t.detach().to(dtype).requires_grad_(t.requires_grad) if t.is_floating_point() else t) for n, t in base.items()}
    names_w = {n: base[n] for n in ometa.inner_param_names([(n, p) for n, p in base.items() if p.is_floating_point()])}
    lrs = {k: v.to(dtype) for k, v in orules.init_lrs('lslr', names_w, 1e-2, num_steps=2).items()}
    torch.set_num_threads(min(16, torch.get_num_threads()))
    res = ometa.run_iteration(model, base, [f.to(dtype) for f in frames(model)], rule='lslr', optimizer='SGD', lrs=lrs, num_steps=2,
                              loss='MSE', training=True, second_order=True, forward_kwargs=forward_kwargs)
    res['loss'].backward()
    return res['loss'].item(), {n: fp(p.grad) for n, p in base.items() if p.requires_grad and p.grad is not None}


@functools.lru_cache(maxsize=None)
def oracle_run(model, dtype=torch.float32):
    """(loss, {parameter name: fingerprint of its outer gradient}) of the oracle's second-order meta-iteration; the warps are the
    written-out statements that differentiate twice (Super SloMo's and RRIN's default O.flow_warp is one)"""
    from oracle import torch_ops as O
    return _oracle(model, dtype, dict(warp=O.voxel_warp_blend_written_out) if model == 'voxelflow' else None)


# ------------------------------------------------------------------------------------------------------------------------------------
# the product's runs, in a child process
# ------------------------------------------------------------------------------------------------------------------------------------
ONCE = "once_differentiable"          # what autograd says when the second backward meets the fused warp without the flag
MARK = "WARP2_SYSTEM "


def device_run(model, flag):
    """(loss, outer-gradient fingerprints) of the product's meta-iteration with --warp_second_order `flag`, in this process"""
    from tests.helpers import build_system, observe
    system = build_system(model, dict(OVER, warp_second_order=flag, weight_recipe=RECIPE[model]))
    scale_flow_heads(model, dict(system.net.named_parameters()))
    rec = observe(system)
    losses, _, _ = system.run_train_iter(data_batch=frames(model), epoch=0, do_evaluation=False)
    torch.cuda.synchronize()
    return losses['loss'].item(), rec['outer_grad_fp']


@functools.lru_cache(maxsize=None)
def device_runs():
    """{(model, flag): (loss, fingerprints) or the message of the RuntimeError the run raised}, from one child process"""
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MIOPEN_USER_DB_PATH=tempfile.mkdtemp(prefix='savfi_warp2_miopen_'))
    cmd = [sys.executable] + (['-s'] if sys.flags.no_user_site else []) + ['-m', 'tests.warp2_system']
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=repo, env=env)
    lines = [line for line in out.stdout.splitlines() if line.startswith(MARK)]
    assert out.returncode == 0 and len(lines) == 1, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])
    res = {}
    for key, val in json.loads(lines[0][len(MARK):]).items():
        model, flag = key.split('/')
        res[(model, int(flag))] = val['error'] if 'error' in val else (val['loss'], val['fp'])
    return res


def _main():
    torch.backends.cudnn.deterministic = True                  # as tests/conftest.py pins the library for the parity suites
    res = {}
    for model in ('voxelflow', 'rrin', 'superslomo'):
        for flag in (1, 0):
            try:
                loss, fps = device_run(model, flag)
                res['%s/%d' % (model, flag)] = dict(loss=loss, fp={k: [float(x) for x in v] for k, v in fps.items()})
            except RuntimeError as exc:
                res['%s/%d' % (model, flag)] = dict(error=str(exc)[:500])
                if ONCE not in str(exc):                       # anything but the expected refusal: start nothing more on the device
                    print(MARK + json.dumps(res))
                    raise
    print(MARK + json.dumps(res))


if __name__ == '__main__':
    _main()
