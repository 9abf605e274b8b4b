"""Shared test helpers (CPU side): build oracle inputs from the seeded recipe, read golden fixtures."""
import ast
import contextlib
import os

import numpy as np
import torch

from meta_interpolation_amd import synthetic
from meta_interpolation_amd.config import default_args

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def golden(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)


def build_plugin(model, device="cpu", recipe=None):
    """The product's nn.Module for `model` (constructing it launches no kernel) with seeded weights (`recipe`: synthetic.py)."""
    from meta_interpolation_amd.meta_learning_system import MODEL_REGISTRY
    args = default_args(model=model, num_gpu=0)
    net = MODEL_REGISTRY[model](args, False)
    synthetic.load_seeded_weights(net, model, recipe=recipe)
    return net.to(device)


def oracle_base(model, recipe=None):
    """{name: tensor} for the oracle: parameters are leaves with requires_grad, buffers are plain."""
    net = build_plugin(model, recipe=recipe)
    base = {}
    pnames = {n for n, _ in net.named_parameters()}
    for name, t in net.state_dict().items():
        t = t.clone()
        if name in pnames:
            t.requires_grad_(True)
        base[name] = t
    return base


def parse_case_args(npz):
    return dict(ast.literal_eval(str(npz['args'])))


def fp(t):
    t = t.detach().double().reshape(-1).cpu()
    v = [t.sum().item(), t.abs().sum().item()] + t[:4].tolist()
    return np.array(v + [0.0] * (6 - len(v)))


FP_ATOL = 1e-8     # absolute floor of a fingerprint sum: fp32 rounding of O(1) activations summed over a layer


def assert_fp_close(got, want, rtol=1e-5, what="", extra_abs=0.0):
    """Fingerprints: [sum, abs-sum, first 4].  Compared relative to the abs-sum scale, with an absolute floor: the gradient
    of a 12-element channel-attention bias has an abs-sum of 5e-6, and 1e-3 of that is below the rounding noise of the
    convolutions it is summed from (seen as a run-order dependent 1.06e-3 on exactly that tensor).  `extra_abs`: an absolute
    allowance the caller derives from another contract bound (an updated weight w - lr g carries the gradient's bound on lr g)."""
    scale = max(abs(want[1]), 1e-12)
    assert abs(got[0] - want[0]) <= rtol * scale + FP_ATOL + extra_abs, (what, got[0], want[0])
    assert abs(got[1] - want[1]) <= rtol * scale + FP_ATOL + extra_abs, (what, got[1], want[1])


CANARY = 7777.0
PAD = 64                  # floats of canary on either side of a buffer the kernels write (256 bytes: the payload stays aligned)


class Guarded:
    """Device outputs inside canary-padded buffers: new(name, *shape) hands out a view, check() asserts nothing around any of them
    changed."""

    def __init__(self, device="cuda"):
        self.bufs, self.device = {}, device

    def new(self, name, *shape, fill=None):
        n = int(np.prod(shape))
        buf = torch.full((n + 2 * PAD,), CANARY, device=self.device)
        view = buf[PAD:PAD + n]
        if fill is not None:
            view.fill_(fill)
        self.bufs[name] = (buf, n)
        return view.view(*shape)

    def check(self, where):
        for name, (buf, n) in self.bufs.items():
            assert bool((buf[:PAD] == CANARY).all()) and bool((buf[PAD + n:] == CANARY).all()), "%s: wrote outside %s" % (where, name)

    def untouched(self, name):
        buf, n = self.bufs[name]
        return bool((buf == CANARY).all())


class LaunchRecord:
    """What record_launches() saw, in launch order: `launches` holds one [name, nbytes, flops, whats] per _hip.launch call (whats: the
    `what` strings _hip.check was handed while that launch ran), `names` just the names."""

    def __init__(self):
        self.launches, self.names = [], []


@contextlib.contextmanager
def record_launches():
    """Record every launch through _hip.launch while the block runs; the launches themselves run as usual (timers included).  The
    previous _hip.launch / _hip.check come back on exit."""
    from meta_interpolation_amd import _hip
    rec, launch, check, running = LaunchRecord(), _hip.launch, _hip.check, []

    def spy_launch(name, fn, nbytes=0, flops=0):
        entry = [name, nbytes, flops, []]
        rec.launches.append(entry)
        rec.names.append(name)
        running.append(entry)
        try:
            return launch(name, fn, nbytes=nbytes, flops=flops)
        finally:
            running.pop()

    def spy_check(code, what):
        if running:
            running[-1][3].append(what)
        return check(code, what)

    _hip.launch, _hip.check = spy_launch, spy_check
    try:
        yield rec
    finally:
        _hip.launch, _hip.check = launch, check


def build_system(model, overrides, fuse=1, device="cuda"):
    """Product system with seeded weights.  Execution-mode switches are pinned to the plain eager loop unless a test asks for a
    mode (`graph_inner_loop`, `task_batch`, `task_streams` in `overrides`): the fixture tests hook update_params per step."""
    from meta_interpolation_amd.meta_learning_system import SceneAdaptiveInterpolation
    overrides = dict(overrides)
    recipe = overrides.pop('weight_recipe', None)          # fixture key: which seeded-weights recipe the reference run used
    overrides.setdefault('graph_inner_loop', 0)
    overrides.setdefault('task_streams', 1)
    args = default_args(model=model, num_gpu=1, fuse_support_pairs=fuse, **overrides)
    net = build_plugin(model, device, recipe=recipe)
    system = SceneAdaptiveInterpolation(args, net=net)
    if args.attenuate:
        sd, gm = synthetic.seeded_attenuator_state(len(system.inner_loop_optimizer.names_learning_rates_dict))
        system.attenuator.load_state_dict(sd)
        with torch.no_grad():
            system.gamma_mult.copy_(gm)
    return system


def observe(system, check_rule=False):
    """Wrap update_params / optimizer.step of a product system to record fingerprints.  With
    check_rule=True every fused update is also replayed on the CPU by the oracle's rule from the SAME
    weights / grads / learning rates and the element-wise deviation is recorded (rec['rule_err'])."""
    rec = dict(n_live=[], grad_fp=[], weight_fp=[], moved=[], outer_grad_fp={}, rule_err=[])
    rule = system.inner_loop_optimizer
    theta = {k.replace('module.', ''): v.detach() for k, v in system.net.named_parameters()}
    orig = rule.update_params
    kind = 'metasgd' if type(rule).__name__.startswith('MetaSGD') else 'lslr'
    ostate = {}
    if check_rule:
        from oracle import rules as orules
        orig_init = rule.initialize_state

        def initialize_state():
            ostate['st'] = orules.RuleState()
            return orig_init()
        rule.initialize_state = initialize_state

    def update_params(names_weights_dict, names_grads_wrt_params_dict, num_step, **kw):
        if check_rule:
            w_cpu = {k: v.detach().cpu() for k, v in names_weights_dict.items()}
            g_cpu = {k: (None if v is None else v.detach().cpu()) for k, v in names_grads_wrt_params_dict.items()}
        out = orig(names_weights_dict=names_weights_dict, names_grads_wrt_params_dict=names_grads_wrt_params_dict,
                   num_step=num_step, **kw)
        if check_rule:
            lrs = {k: v.detach().cpu() for k, v in rule.names_learning_rates_dict.items()}
            with torch.no_grad():
                want = orules.update_params(kind, rule.optimizer, w_cpu, g_cpu, lrs, num_step, ostate['st'])
            assert sorted(want) == sorted(out)
            worst = 0.0
            for k, v in want.items():
                d = (out[k].detach().cpu() - v).abs().max().item()
                worst = max(worst, d / max(v.abs().max().item(), 1e-12))
            rec['rule_err'].append(worst)
        rec['n_live'].append(len(out))
        rec['grad_fp'].append({k: fp(v) for k, v in names_grads_wrt_params_dict.items() if v is not None})
        rec['weight_fp'].append({k: fp(v) for k, v in out.items()})
        # how far each fast weight has moved away from theta (abs-sum): the part of its value that is accumulated lr * g
        rec['moved'].append({k: ((v.detach() - theta[k]).abs().sum().item() if k in theta and v.shape == theta[k].shape else 0.0)
                             for k, v in out.items()})
        return out
    rule.update_params = update_params

    def step(*a, **k):
        rec['outer_grad_fp'] = {n: fp(p.grad) for n, p in system.named_parameters()
                                if p.requires_grad and p.grad is not None}
    system.optimizer.step = step
    return rec




# ---------------------------------------------------------------------------------------------
# CPU test doubles: let the host logic (task loop, sharding, all-reduce) run without a GPU.  They live
# in tests/ only; the product classes raise on CPU tensors.
# ---------------------------------------------------------------------------------------------
class OracleRule(torch.nn.Module):
    """Inner rule with the product surface, arithmetic by oracle/rules.py (pure PyTorch, any device)."""

    def __init__(self, kind, optimizer, init_lr, num_steps):
        super().__init__()
        self.kind, self.optimizer, self.init_lr, self.num_steps = kind, optimizer, init_lr, num_steps
        self.names_learning_rates_dict = torch.nn.ParameterDict()

    def initialize(self, names_weights_dict):
        from oracle import rules
        lrs = rules.init_lrs(self.kind, names_weights_dict, self.init_lr, num_steps=self.num_steps, learnable=True)
        self.names_learning_rates_dict = torch.nn.ParameterDict(
            {k: torch.nn.Parameter(v.detach().clone()) for k, v in lrs.items()})

    def initialize_state(self):
        from oracle import rules
        self.st = rules.RuleState()

    def update_params(self, names_weights_dict, names_grads_wrt_params_dict, num_step, tau=0.1):
        from oracle import rules
        return rules.update_params(self.kind, self.optimizer, names_weights_dict, names_grads_wrt_params_dict,
                                   dict(self.names_learning_rates_dict.items()), num_step, self.st)


class ToyNet(torch.nn.Module):
    """Two-conv interpolation plugin built from the product's Meta layers (CPU-capable: conv2d only)."""
    lockstep_tasks = True      # samples never interact, fast weights only through the meta layers

    def __init__(self):
        super().__init__()
        from meta_interpolation_amd.model_utils import MetaConv2dLayer, MetaSequential
        self.body = MetaSequential(MetaConv2dLayer(6, 8, 3, 1, 1), torch.nn.ReLU(), MetaConv2dLayer(8, 3, 3, 1, 1))

    def forward(self, f0, f1, params=None, **kw):
        from meta_interpolation_amd.model_utils import as_view
        pv = as_view(params)
        return self.body(torch.cat([f0, f1], 1), None if pv is None else pv.sub("body"))

    def zero_grad(self, params=None):
        from meta_interpolation_amd.model_utils import zero_grad_params
        zero_grad_params(self, params)

    def restore_backup_stats(self):
        pass


class CpuL1(torch.nn.Module):
    def forward(self, out, tgt, **kw):
        l = torch.nn.functional.l1_loss(out, tgt)
        return {'L1': l, 'total': l}

    def per_sample(self, out, tgt):
        l = (out - tgt).abs().flatten(1).mean(1)
        return {'L1': l, 'total': l}

    def loss_keys(self):
        return ['L1', 'total']


def build_toy_system(task_parallel=None, steps=2, batch=4, seed=0, msl=False, task_batch=0):
    from meta_interpolation_amd.meta_learning_system import SceneAdaptiveInterpolation
    args = default_args(model='toy', num_gpu=0, optimizer='SGD', inner_lr=0.05, outer_lr=0.01, batch_size=batch,
                        number_of_training_steps_per_iter=steps, number_of_evaluation_steps_per_iter=steps,
                        use_multi_step_loss_optimization=msl, multi_step_loss_num_epochs=5, fuse_support_pairs=0,
                        task_batch=task_batch)
    torch.manual_seed(seed)
    net = ToyNet()
    return SceneAdaptiveInterpolation(args, net=net, inner_loop_optimizer=OracleRule('lslr', 'SGD', 0.05, steps),
                                      criterion=CpuL1(), task_parallel=task_parallel)
