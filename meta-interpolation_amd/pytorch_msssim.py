"""The reference's ``pytorch_msssim`` names for multi-scale SSIM (pytorch_msssim/__init__.py:78-142) on the fused gfx950 kernels of
csrc/ssim.hip: ``msssim`` and ``MSSSIM`` with the reference's arguments.  Device tensors only; gradient for ``img1`` only.

What the kernels do not offer is refused, never approximated: a ``window_size`` other than 11 (the window of a level is
min(11, H_s, W_s) taps, as in the reference) and ``size_average=False`` (the reference mixes a per-sample SSIM with a batch-wide cs
there; hip_ops.msssim_per_sample gives every sample's own value instead).
"""
import torch

from . import hip_ops


def msssim(img1, img2, window_size=11, size_average=True, val_range=None, normalize=False):
    if window_size != 11:
        raise NotImplementedError("msssim: the kernels are built for window_size=11, got %r" % (window_size,))
    if not size_average:
        raise NotImplementedError("msssim: size_average=False (a per-sample SSIM with a batch-wide cs) is not offered; "
                                  "hip_ops.msssim_per_sample gives every sample's own value")
    return hip_ops.msssim(img1, img2, val_range=val_range, normalize=normalize)


class MSSSIM(torch.nn.Module):
    def __init__(self, window_size=11, size_average=True, channel=3):
        super().__init__()
        self.window_size = window_size
        self.size_average = size_average
        self.channel = channel

    def forward(self, img1, img2):
        return msssim(img1, img2, window_size=self.window_size, size_average=self.size_average)
