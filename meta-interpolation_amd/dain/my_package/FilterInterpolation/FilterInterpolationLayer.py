"""DAIN's adaptive warping layer on the gfx950 kernel (csrc/dainwarp.hip through hip_ops.filter_interpolation).

Same call surface as the reference's dain/my_package/FilterInterpolation/FilterInterpolationLayer.py (a Function with
``apply(input1, input2, input3)``); the CUDA extension behind it is replaced by the C ABI of libsavfi_hip.so.  Device tensors only:
a CPU tensor raises NotImplementedError.
"""
from .... import hip_ops


class FilterInterpolationLayer:
    """``FilterInterpolationLayer.apply(input1, input2, input3)``: input1 [B,C,H,W] warped by the flow input2 [B,2,H,W] through the
    per-pixel 4 x 4 filter input3 [B,16,H,W]."""

    @staticmethod
    def apply(input1, input2, input3):
        return hip_ops.filter_interpolation(input1, input2, input3)
