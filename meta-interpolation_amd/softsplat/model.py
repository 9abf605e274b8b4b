"""Softmax-splatting plugin (``--model softsplat``): the image-level variant of Niklaus & Liu (CVPR 2020) with fast weights, built from
parts this package has.

    reflect-pad to 64 -> flowComp(I0|I1) -> F_0_1, F_1_0                       (Super SloMo's MetaUNet(6, 4), the same names)
      Z_0 = alpha * mean_c |I0 - warp(I1, F_0_1)|,  Z_1 = alpha * mean_c |I1 - warp(I0, F_1_0)|       (alpha: a learnable scalar, < 0)
      S_0, h_0 = softsplat(I0, t F_0_1, Z_0),       S_1, h_1 = softsplat(I1, (1 - t) F_1_0, Z_1)      (hip_ops.softsplat: forward warps)
      refine(S_0|S_1|h_0|h_1|I0|I1) -> residual r (3 channels), logit m (1)    (MetaUNet(14, 4))
      frame = sigmoid(m) S_0 + (1 - sigmoid(m)) S_1 + r, cropped

``t`` is Super SloMo's ``T_GRID[ind]`` as an fp32 Python float, so the pass reads nothing on the host and can be captured.  Both U-Nets
read the fast-weight dict (``flowComp.*``, ``refine.*``); ``alpha`` is the module's own parameter: it is meta-learned by the outer loop and
not adapted by the inner one.  Samples never interact (``lockstep_tasks``).  ``flowComp`` carries Super SloMo's names, so a Super SloMo
``state_dictFC`` loads into it.  Second-order passes take hip_ops.softsplat_composed; the metric's backward warp needs
``--warp_second_order 1`` there (without it the warp raises, as it does for Super SloMo).

There is no reference implementation and no public checkpoint on hand: loading one (``pretrained_models/softsplat_base.pth``, a state
dict of this module) is not verified.  Not built: feature-pyramid splatting with a GridNet, a `linear` mode.
"""
import numpy as np
import torch
import torch.nn as nn

from .. import hip_ops, model_utils
from ..model_utils import _pad_to_multiple, as_view, zero_grad_params
from ..rrin.model import warp
from ..superslomo.model import T_GRID, MetaUNet

MODES = ('soft', 'avg')


class MetaSoftSplat(nn.Module):
    lockstep_tasks = True     # samples never interact; verified against the sequential loop (tests/test_softsplat_system_gpu.py)

    def __init__(self, alpha=-20.0, mode='soft', resume=False):
        super().__init__()
        if mode not in MODES:
            raise ValueError("softsplat: mode must be one of %s, got %r" % (MODES, mode))
        self.mode = mode
        self.flowComp = MetaUNet(6, 4)
        self.refine = MetaUNet(14, 4)
        self.alpha = nn.Parameter(torch.full((1,), float(alpha)))
        if resume:
            path = 'pretrained_models/softsplat_base.pth'
            print('Loading model: ' + path)
            self.load_state_dict(torch.load(path, map_location='cpu', weights_only=False))

    def forward(self, frame0, frame1, ind=3, params=None, **kwargs):
        t = float(np.float32(T_GRID[int(ind)]))
        u = float(np.float32(1.0 - T_GRID[int(ind)]))
        pw, ph = _pad_to_multiple(frame0.size(3), 6), _pad_to_multiple(frame0.size(2), 6)
        left, top = pw // 2, ph // 2
        pad_in = nn.ReflectionPad2d([left, pw - left, top, ph - top])
        I0, I1 = pad_in(frame0), pad_in(frame1)
        pv = as_view(params)
        sub = (lambda name: None) if pv is None else pv.sub

        flows = self.flowComp(torch.cat((I0, I1), dim=1), params=sub("flowComp"))
        F_0_1, F_1_0 = flows[:, :2], flows[:, 2:]
        alpha = self.alpha.detach() if model_utils.own_params_const() else self.alpha
        if self.mode == 'soft':
            Z_0 = alpha.view(1, 1, 1, 1) * (I0 - warp(I1, F_0_1)).abs().mean(1, keepdim=True)
            Z_1 = alpha.view(1, 1, 1, 1) * (I1 - warp(I0, F_1_0)).abs().mean(1, keepdim=True)
        else:
            Z_0 = Z_1 = None
        S_0, h_0 = hip_ops.softsplat(I0, t * F_0_1, Z_0, self.mode, return_hit=True)
        S_1, h_1 = hip_ops.softsplat(I1, u * F_1_0, Z_1, self.mode, return_hit=True)
        tail = self.refine(torch.cat((S_0, S_1, h_0, h_1, I0, I1), dim=1), params=sub("refine"))
        m = torch.sigmoid(tail[:, 3:4])
        frame = m * S_0 + (1.0 - m) * S_1 + tail[:, :3]
        return frame[:, :, top:frame.size(2) - (ph - top), left:frame.size(3) - (pw - left)]

    def zero_grad(self, params=None):
        zero_grad_params(self, params)

    def restore_backup_stats(self):
        pass  # no batch statistics in this model
