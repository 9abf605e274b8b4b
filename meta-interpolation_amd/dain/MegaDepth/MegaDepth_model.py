"""MegaDepth's hourglass (Li & Snavely 2018; Chen et al.'s "Depth in the Wild" network), the depth estimator of DAIN, on the gfx950 kernels.

``HourGlass(pretrained=None)`` returns the module whose ``state_dict()`` has the 779 names and shapes of the reference's
dain/MegaDepth/pytorch_DIW_scratch.py (nested Sequential indices such as ``3.0.0.1.0.0.weight``), so that
best_generalization_net_G.pth and dain_base.pth load by name.  The tree is built from a compact description: an inception block is
(width of its 1x1 branch, ((kernel, middle width, width), ...)) and a level of the hourglass is a pair of branches, one of which pools,
recurses and upsamples.

The forward runs, per layer: the convolution through hip_ops.conv_bias_act (its routing decides the kernel; the 1x1 and 11x11 layers take
its ATen route), BatchNorm + ReLU on csrc/dainnet.hip with each branch written into its slice of the block's concatenation, the two
max-pools on the same file, the two average pools on csrc/avgpool.hip, and each level's "upsample, then add the skip" as one pass.

BatchNorm: the reference runs this network in training mode whenever the system trains or validates (it calls self.train() and never
eval(), meta_learning_system.py:595-617), so every BatchNorm normalises with the statistics of the call's own batch -- the two frames of
one task.  ``forward(x, n_per_group)`` keeps that for any batch: a group of n_per_group consecutive samples gets the statistics of a call
of its own, bit for bit.  The statistics of all 155 layers land in one flat buffer [2, groups, channels of all layers] that the caller keeps
(``last_stats``): the forward does not touch the running buffers; ``update_running_stats(stats)`` applies the update of one reference
forward per group (momentum 0.1, unbiased variance, num_batches_tracked + 1) as one multi-tensor call.  In eval mode the BatchNorms read
the running buffers.  Forward only: the depth net is frozen on every path of the reference's system.
"""
import torch
import torch.nn as nn

from ... import _hip, hip_ops

__all__ = ['HourGlass']

# inception blocks: (width of the 1x1 branch, ((kernel, middle width, width), ...)); the input width is whatever comes in
A = (32, ((3, 32, 32), (5, 32, 32), (7, 32, 32)))           # -> 128
B = (64, ((3, 32, 64), (5, 32, 64), (7, 32, 64)))           # -> 256
C = (64, ((3, 64, 64), (7, 64, 64), (11, 64, 64)))          # -> 256
E = (32, ((3, 64, 32), (7, 64, 32), (11, 64, 32)))          # -> 128
F = (32, ((3, 64, 32), (5, 64, 32), (7, 64, 32)))           # -> 128
G = (16, ((3, 32, 16), (7, 32, 16), (11, 32, 16)))          # -> 64
H = (16, ((3, 64, 16), (7, 64, 16), (11, 64, 16)))          # -> 64
# a level: the two branches of its ConcatTable in the reference's order; a list inside a branch is the next level
LEVEL1 = [[B, B], ['avg', B, B, B, 'up']]
LEVEL2 = [[B, C], ['avg', B, B, LEVEL1, B, C, 'up']]
LEVEL3 = [['max', A, B, LEVEL2, B, A, 'up'], [A, E]]
LEVEL4 = [['max', A, A, LEVEL3, F, G, 'up'], [H]]


class ConcatTable(nn.Sequential):
    """Torch7's ConcatTable: every child on the same input (the reference's LambdaMap)."""


class CAddTable(nn.Module):
    """Torch7's CAddTable: the sum of the branches (the reference's parameterless LambdaReduce)."""


class Inception(nn.Sequential):
    """Branches of conv - BatchNorm - ReLU (- conv - BatchNorm - ReLU), concatenated over channels."""

    @property
    def out_channels(self):
        return sum([m for m in br if isinstance(m, nn.Conv2d)][-1].out_channels for br in self)


def _unit(cin, cout, k):
    return [nn.Conv2d(cin, cout, (k, k), (1, 1), ((k - 1) // 2, (k - 1) // 2)), nn.BatchNorm2d(cout, 1e-05, 0.1, False), nn.ReLU()]


def _inception(cin, spec):
    first, rest = spec
    return Inception(nn.Sequential(*_unit(cin, first, 1)),
                     *[nn.Sequential(*(_unit(cin, mid, 1) + _unit(mid, out, k))) for k, mid, out in rest])


def _branch(cin, items):
    mods = []
    for it in items:
        if it == 'max':
            mods.append(nn.MaxPool2d((2, 2), (2, 2)))
        elif it == 'avg':
            mods.append(nn.AvgPool2d((2, 2), (2, 2)))
        elif it == 'up':
            mods.append(nn.UpsamplingNearest2d(scale_factor=2))
        elif isinstance(it, list):
            mods.append(_level(cin, it))
        else:
            mods.append(_inception(cin, it))
            cin = mods[-1].out_channels
    return nn.Sequential(*mods)


def _level(cin, spec):
    return nn.Sequential(ConcatTable(*[_branch(cin, items) for items in spec]), CAddTable())


class HourGlassNet(nn.Sequential):
    """0: Conv2d(3, 128, 7), 1: BatchNorm2d(128) (the one affine BatchNorm), 2: ReLU, 3: the four-level hourglass, 4: Conv2d(64, 1, 3)."""

    def __init__(self):
        super().__init__(nn.Conv2d(3, 128, (7, 7), (1, 1), (3, 3)), nn.BatchNorm2d(128), nn.ReLU(), _level(128, LEVEL4),
                         nn.Conv2d(64, 1, (3, 3), (1, 1), (1, 1)))
        self._bns = [m for m in self.modules() if isinstance(m, nn.BatchNorm2d)]
        off = 0
        for m in self._bns:
            m.stat_offset = off                                 # its channels in the flat statistics buffer
            off += m.num_features
        self.stat_channels = off
        self._filters = {}
        self.last_stats = None

    # -- layers ---------------------------------------------------------------------------------------------------------------
    def _conv(self, c, x, run):
        """One call per group: which kernel a convolution runs on depends on its batch, and a group's numbers must not."""
        npg, cache = run['npg'], self._filters.setdefault(id(c), {})
        one = lambda t: hip_ops.conv_bias_act(t, c.weight, c.bias, 1, c.padding[0], 1, 1, 1.0, cache=cache)
        if x.shape[0] == npg:
            return one(x)
        return torch.cat([one(x[g:g + npg]) for g in range(0, x.shape[0], npg)], 0)

    def _bn_relu(self, bn, x, run, out=None, c_off=0):
        C = bn.num_features
        if not run['training']:                                 # eval mode: the running buffers, one set for the whole batch
            return hip_ops.bn_apply_relu(x, bn.running_mean.view(1, C), bn.running_var.view(1, C), x.shape[0], bn.weight, bn.bias,
                                         bn.eps, out, c_off)
        off = bn.stat_offset
        mean, var = run['mean'][:, off:off + C], run['var'][:, off:off + C]
        hip_ops.bn_stats(x, run['npg'], mean, var)
        run['count'][off] = run['npg'] * x.shape[2] * x.shape[3]
        return hip_ops.bn_apply_relu(x, mean, var, run['npg'], bn.weight, bn.bias, bn.eps, out, c_off)

    def _inception(self, block, x, run):
        out = x.new_empty(x.shape[0], block.out_channels, x.shape[2], x.shape[3])
        c_off = 0
        for br in block:
            t = x
            for i in range(0, len(br), 3):                      # conv, BatchNorm, ReLU; the branch's last unit writes its slice
                last = i + 3 == len(br)
                t = self._bn_relu(br[i + 1], self._conv(br[i], t, run), run, out if last else None, c_off if last else 0)
            c_off += br[-3].out_channels
        return out

    def _run(self, mods, x, run):
        """The modules of one branch; a trailing upsample is left to the caller, which adds the skip in the same pass."""
        for m in mods:
            if isinstance(m, Inception):
                x = self._inception(m, x, run)
            elif isinstance(m, nn.MaxPool2d):
                x = hip_ops.max_pool2x2(x)
            elif isinstance(m, nn.AvgPool2d):
                x = hip_ops.avg_pool2x2(x)
            elif isinstance(m, nn.UpsamplingNearest2d):
                assert m is mods[-1]
            else:                                               # a level: Sequential(ConcatTable(a, b), CAddTable)
                a, b = m[0]
                ya, yb = self._run(list(a), x, run), self._run(list(b), x, run)
                low, skip = (ya, yb) if isinstance(a[-1], nn.UpsamplingNearest2d) else (yb, ya)
                x = hip_ops.upnearest2x_add(low, skip)
        return x

    @torch.no_grad()
    def forward(self, x, n_per_group=None):
        """x [N,3,H,W] (H, W multiples of 16) -> log depth [N,1,H,W].  Training mode: groups of n_per_group consecutive samples
        (default: the whole batch, the reference's call) are normalised on their own; their statistics are left in ``last_stats``.
        A group's result is, bit for bit, that of a call on the group alone."""
        x = x.contiguous()
        _hip.require_cuda(x)
        npg = x.shape[0] if n_per_group is None else int(n_per_group)
        if npg <= 0 or x.shape[0] % npg:
            raise ValueError("a batch of %d samples is no multiple of n_per_group = %d" % (x.shape[0], npg))
        run = {'npg': npg, 'training': self.training}
        if self.training:
            flat = x.new_empty(2, x.shape[0] // npg, self.stat_channels)
            run.update({'mean': flat[0], 'var': flat[1], 'count': {}})
        y = self._bn_relu(self[1], self._conv(self[0], x, run), run)
        y = self._run([self[3]], y, run)
        y = self._conv(self[4], y, run)
        if self.training:
            self.last_stats = run
        return y

    # -- running statistics -----------------------------------------------------------------------------------------------------
    def update_running_stats(self, stats, groups=None):
        """What the reference's forwards that produced `stats` (a ``last_stats``) do to the running buffers: for every group in order,
        running <- 0.9 running + 0.1 (mean | variance * n / (n - 1)) and num_batches_tracked + 1, as one multi-tensor call per group."""
        G = stats['mean'].shape[0]
        running = [b.running_mean for b in self._bns] + [b.running_var for b in self._bns]
        unbias = [1.0] * len(self._bns) + [stats['count'][b.stat_offset] / (stats['count'][b.stat_offset] - 1.0) for b in self._bns]
        for g in (range(G) if groups is None else groups):
            src = []
            for key in ('mean', 'var'):
                row = stats[key][g]
                src += [row[b.stat_offset:b.stat_offset + b.num_features] for b in self._bns]
            hip_ops.bn_running_update(running, src, unbias, 0.1)
            torch._foreach_add_([b.num_batches_tracked for b in self._bns], 1)


def HourGlass(pretrained=None):
    """The hourglass; `pretrained`: a state dict file saved from a DataParallel wrapper (its 'module.' prefix is stripped, as
    dain/MegaDepth/models/HG_model.py:37 does)."""
    model = HourGlassNet()
    if pretrained is not None:
        pretrained_dict = torch.load(pretrained, map_location='cpu', weights_only=False)
        model_dict = model.state_dict()
        model_dict.update({k[7:]: v for k, v in pretrained_dict.items()})
        model.load_state_dict(model_dict)
    return model
