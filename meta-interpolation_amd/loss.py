"""Loss wrapper for the inner/outer objectives: ``'w*TYPE+w*TYPE'`` with TYPE in {L1, MSE, SSIM, MSSSIM, Lap, Census}.

Surface follows the reference's ``Loss`` (loss.py:278-350): ``criterion(sr, hr) -> {TYPE: w*loss, ...,
'total': sum}``.  L1 / MSE run on the fused savfi reduction kernel (one launch, no temporaries), SSIM on the fused
window kernel of csrc/ssim.hip (forward and gradient, the reference's data-dependent dynamic range decided on the device);
the reference's VGG / GAN / SuperSloMo terms are outside this path and are rejected loudly.

MSSSIM is an ADDITION: the reference's ``Loss`` has no such branch, though the reference vendors ``pytorch_msssim.msssim``.  The term is
``1 - msssim(sr, hr, normalize=True)`` with the data-dependent range of every level, on the multi-scale kernels of csrc/ssim.hip.
``normalize=True`` because the plain product is NaN whenever a level's contrast mean is negative, which an untrained prediction gives.

Lap is an ADDITION too: the Laplacian-pyramid L1 that kernel-based interpolators train with, five levels of the 5-tap binomial window
with reflected borders, the last level the low-pass residual, ``sum_s 2^s sum |b_s| / n_0`` (the scale of L1), on the fused kernels of
csrc/laploss.hip (one pyramid of ``sr - hr``; gradient for ``sr`` only).  Frames of 17 x 17 or more.

Census is an ADDITION as well: the census (soft ternary) loss that flow-based interpolators train with, a distance between 7 x 7
local-structure descriptors that a brightness or contrast change between the frames hardly moves.  On the gray image ``g`` (zero outside
the frame), ``t_o = d_o / sqrt(0.81 + d_o^2)`` of ``d_o = g(p + o) - g(p)`` for the 49 offsets, ``delta_o = (t_o(sr) - t_o(hr))^2``, the mean
over the offsets of ``delta_o / (0.1 + delta_o)``, summed over the pixels off the outermost ring and divided by ``H W``, on the fused kernels
of csrc/census.hip (gradient for ``sr`` only).  3 or 1 channels, frames of 3 x 3 or more.  The constants presume unit-range frames; the
term is applied to whatever tensors the criterion receives, as the other terms are -- Super SloMo's mean-subtracted and VoxelFlow's
normalised frames included.
"""
import torch.nn as nn

from . import hip_ops


def msssim_loss(sr, hr):
    """1 - msssim(sr, hr, normalize=True) as one value over the batch, the range of every level decided from `sr` (gradient for `sr` only)."""
    return 1 - hip_ops.msssim(sr, hr, normalize=True)


def msssim_loss_per_sample(sr, hr):
    """[N]: the same term for every sample on its own, each an N = 1 call (tasks adapted in lockstep)."""
    return 1 - hip_ops.msssim_per_sample(sr, hr, normalize=True)


# TYPE -> (one value over the batch, [N]: every sample on its own)
_KERNELS = {'L1': (hip_ops.l1_loss, hip_ops.l1_loss_per_sample), 'MSE': (hip_ops.mse_loss, hip_ops.mse_loss_per_sample),
            'SSIM': (hip_ops.ssim_loss, hip_ops.ssim_loss_per_sample), 'MSSSIM': (msssim_loss, msssim_loss_per_sample),
            'Lap': (hip_ops.lap_loss, hip_ops.lap_loss_per_sample), 'Census': (hip_ops.census_loss, hip_ops.census_loss_per_sample)}


class Loss(nn.modules.loss._Loss):
    def __init__(self, args):
        super().__init__()
        self.loss = []
        for term in args.loss.split('+'):
            weight, loss_type = term.split('*')
            if loss_type not in _KERNELS:
                raise NotImplementedError(
                    "loss '%s' is outside the inner-loop path built here (only L1, MSE; 'Super' / VGG terms need pretrained VGG16 weights)" % loss_type)
            self.loss.append({'type': loss_type, 'weight': float(weight), 'function': _KERNELS[loss_type][0]})
        self.cuda_only = True

    def loss_keys(self):
        """Keys of the dict forward() returns (rank-independent: the logging all-reduce is laid out from them)."""
        return [l['type'] for l in self.loss] + ['total']

    def _terms(self, sr, hr, per_sample):
        """{TYPE: weight * term, ..., 'total': their sum}, the terms over the batch or per sample."""
        total = 0
        losses = {}
        for l in self.loss:
            eff = l['weight'] * (_KERNELS[l['type']][1] if per_sample else l['function'])(sr, hr)
            losses[l['type']] = eff
            total = total + eff
        losses['total'] = total
        return losses

    def per_sample(self, sr, hr):
        """The same terms for every sample of a batch on its own: {TYPE: [N], 'total': [N]} (tasks adapted in lockstep:
        the reference evaluates the criterion once per task on N=1 tensors, meta_learning_system.py:389-395)."""
        return self._terms(sr, hr, True)

    def forward(self, sr, hr, **kwargs):
        return self._terms(sr, hr, False)


class CharbonnierLoss(nn.modules.loss._Loss):
    """The criterion of --model dain whatever --loss says (reference meta_learning_system.py:493-505 with dain/networks/DAIN.py:638-639):
    the Charbonnier loss of the unpadded rectified frame, ``{'DAIN': L, 'total': L}``.  The reference's sum also holds the term of the
    unrectified frame with weight 0.0; it is not computed here."""

    def __init__(self, eps=hip_ops.CHARBONNIER_EPS):
        super().__init__()
        self.eps = float(eps)
        self.cuda_only = True

    def loss_keys(self):
        return ['DAIN', 'total']

    def per_sample(self, sr, hr):
        value = hip_ops.charbonnier_loss_per_sample(sr, hr, self.eps)
        return {'DAIN': value, 'total': value}

    def forward(self, sr, hr, **kwargs):
        value = hip_ops.charbonnier_loss(sr, hr, self.eps)
        return {'DAIN': value, 'total': value}
