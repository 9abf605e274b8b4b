"""AdaCoF plugin (``--model adacof``): adaptive collaboration of flows (Lee et al., CVPR 2020) with fast weights.

The SepConv U-Net (kernel_unet.py: ``moduleConv{1..5}``, ``moduleDeconv{5..2}``, ``moduleUpsample{5..2}``) with another tail: per output
pixel the network predicts F x F taps, each with a weight AND a learned 2-D offset, and samples the frame bilinearly at the displaced
position (hip_ops.adacof: one fused launch forward, one backward).  Seven heads read the 64-channel half-resolution map:
``moduleWeight{1,2}`` (softmax over the F*F channels), ``moduleAlpha{1,2}`` (vertical offsets), ``moduleBeta{1,2}`` (horizontal offsets)
and ``moduleOcclusion`` (one channel, sigmoid); each is conv 64->64, ReLU, conv 64->64, ReLU, conv 64->n, ReLU, bilinear x2, conv n->n
(parameters ``.{0,2,4,7}.weight/.bias``).

    out = occ * adacof(pad(frame0), W1, A1, B1) + (1 - occ) * adacof(pad(frame1), W2, A2, B2)

Frames are unit range, reflect-padded at the bottom and right to multiples of 32 for the network and replicate-padded by
(F - 1) * dilation / 2 for the op; the result is cropped to the frame.  As in the SepConv plugin only the encoder / decoder ``Basic``
blocks read the fast-weight dict; the heads and the ``moduleUpsampleN`` use the module's own parameters.  Samples never interact
(``lockstep_tasks``), and the op reads nothing on the host, so captured inner loops work as for SepConv.

There is no reference implementation and no public checkpoint on hand: parameter names follow the published layout as far as known;
loading a public checkpoint is not verified.  Not built: a frame gradient in the fused op, one launch for the pair and the blend,
softmax / sigmoid inside the op.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import hip_ops, kernel_unet
from ..model_utils import as_view, zero_grad_params


def _reflect_to_multiple(x, multiple=32):
    """Mirror `x` at the bottom and right up to multiples of `multiple` (hip_ops.reflect_pad pads all four sides: the window is cut)."""
    H, W = x.shape[2], x.shape[3]
    pb, pr = (-H) % multiple, (-W) % multiple
    p = max(pb, pr)
    if p == 0:
        return x
    if p >= H or p >= W:
        raise ValueError("adacof: a %d x %d frame is too small to mirror up to a multiple of %d" % (H, W, multiple))
    return hip_ops.reflect_pad(x, p)[:, :, p:p + H + pb, p:p + W + pr]


class MetaAdaCoF(nn.Module):
    lockstep_tasks = True     # samples never interact; verified against the sequential loop (tests/test_adacof_system_gpu.py)

    def __init__(self, kernel_size=5, dilation=1, resume=False):
        super().__init__()
        self.kernel_size, self.dilation = int(kernel_size), int(dilation)
        if self.kernel_size % 2 == 0 or not 1 <= self.kernel_size <= 11 or not 1 <= self.dilation <= 8:
            raise ValueError("adacof: kernel_size must be odd and at most 11, dilation 1 to 8; got %d, %d" % (self.kernel_size, self.dilation))
        taps = self.kernel_size ** 2
        kernel_unet.build(self)       # moduleConv1..5 / modulePool1..5, moduleDeconv5..2 / moduleUpsample5..2
        self.moduleWeight1 = kernel_unet.head(taps)
        self.moduleAlpha1 = kernel_unet.head(taps)
        self.moduleBeta1 = kernel_unet.head(taps)
        self.moduleWeight2 = kernel_unet.head(taps)
        self.moduleAlpha2 = kernel_unet.head(taps)
        self.moduleBeta2 = kernel_unet.head(taps)
        self.moduleOcclusion = kernel_unet.head(1)
        if resume:
            path = 'pretrained_models/adacof_base.pth'
            print('Loading model: ' + path)
            self.load_state_dict(torch.load(path, map_location='cpu', weights_only=False))

    def forward(self, frame0, frame1, params=None, **kwargs):
        height, width = frame0.size(2), frame0.size(3)
        pv = as_view(params)
        fast = (lambda n: None) if pv is None else pv.sub
        x = _reflect_to_multiple(torch.cat([frame0, frame1], 1))
        combine = kernel_unet.run(self, x, fast)          # [N,64,ph/2,pw/2]

        def head(name):
            return getattr(self, name)(combine)[:, :, :height, :width]
        rim = ((self.kernel_size - 1) * self.dilation // 2,) * 4
        dots = []
        for i, frame in ((1, frame0), (2, frame1)):
            weights = torch.softmax(head("moduleWeight%d" % i), 1)
            dots.append(hip_ops.adacof(F.pad(frame, rim, mode='replicate'), weights, head("moduleAlpha%d" % i), head("moduleBeta%d" % i),
                                       self.dilation))
        occlusion = torch.sigmoid(head("moduleOcclusion"))
        return occlusion * dots[0] + (1.0 - occlusion) * dots[1]

    def zero_grad(self, params=None):
        zero_grad_params(self, params)

    def restore_backup_stats(self):
        pass  # no batch statistics in this model
