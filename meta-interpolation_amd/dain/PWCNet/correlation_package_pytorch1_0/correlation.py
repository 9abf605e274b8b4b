"""``Correlation(pad_size, kernel_size, max_displacement, stride1, stride2, corr_multiply)(input1, input2)`` -- the cost volume of
PWC-Net (dain/PWCNet/correlation_package_pytorch1_0/correlation.py of the reference) on csrc/correlation.hip.  The library builds the
one configuration PWC-Net uses; `slope` fuses the LeakyReLU that PWCDCNet.forward applies to every cost volume into the kernel."""
import torch

from .... import hip_ops

__all__ = ['Correlation', 'CorrelationFunction']

SUPPORTED = "pad_size = max_displacement = 4, kernel_size = 1, stride1 = stride2 = 1, corr_multiply = 1"


def _require_supported(pad_size, kernel_size, max_displacement, stride1, stride2, corr_multiply):
    if (pad_size, kernel_size, max_displacement, stride1, stride2, corr_multiply) != (4, 1, 4, 1, 1, 1):
        raise NotImplementedError("Correlation(pad_size=%r, kernel_size=%r, max_displacement=%r, stride1=%r, stride2=%r, "
                                  "corr_multiply=%r): only PWC-Net's configuration is built (%s)"
                                  % (pad_size, kernel_size, max_displacement, stride1, stride2, corr_multiply, SUPPORTED))


class CorrelationFunction:
    """The reference's autograd function, as far as its callers see it: ``CorrelationFunction.apply(input1, input2, pad_size, ...)``."""

    @staticmethod
    def apply(input1, input2, pad_size, kernel_size, max_displacement, stride1, stride2, corr_multiply, slope=1.0):
        _require_supported(pad_size, kernel_size, max_displacement, stride1, stride2, corr_multiply)
        return hip_ops.correlation(input1, input2, max_displacement, slope)


class Correlation(torch.nn.Module):
    def __init__(self, pad_size=0, kernel_size=0, max_displacement=0, stride1=1, stride2=2, corr_multiply=1):
        super(Correlation, self).__init__()
        _require_supported(pad_size, kernel_size, max_displacement, stride1, stride2, corr_multiply)      # at construction, not first use
        self.pad_size = pad_size
        self.kernel_size = kernel_size
        self.max_displacement = max_displacement
        self.stride1 = stride1
        self.stride2 = stride2
        self.corr_multiply = corr_multiply

    def forward(self, input1, input2, slope=1.0):
        return CorrelationFunction.apply(input1, input2, self.pad_size, self.kernel_size, self.max_displacement, self.stride1,
                                         self.stride2, self.corr_multiply, slope)
