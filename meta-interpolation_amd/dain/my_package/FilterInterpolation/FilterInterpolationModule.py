"""``FilterInterpolationModule()(input1, input2, input3)`` -- the module MetaDAIN.forward calls (dain/networks/DAIN.py:585-596)."""
import torch

from .FilterInterpolationLayer import FilterInterpolationLayer

__all__ = ['FilterInterpolationModule']


class FilterInterpolationModule(torch.nn.Module):
    def forward(self, input1, input2, input3):
        return FilterInterpolationLayer.apply(input1, input2, input3)
