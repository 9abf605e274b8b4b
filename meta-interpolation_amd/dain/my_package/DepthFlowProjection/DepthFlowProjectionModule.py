"""``DepthFlowProjectionModule(requires_grad)(input1, input2)`` -- the module MetaDAIN.forward calls (dain/networks/DAIN.py:585-596)."""
import torch

from .DepthFlowProjectionLayer import DepthFlowProjectionLayer

__all__ = ['DepthFlowProjectionModule']


class DepthFlowProjectionModule(torch.nn.Module):
    def __init__(self, requires_grad=True):
        super().__init__()
        self.requires_grad = requires_grad

    def forward(self, input1, input2):
        return DepthFlowProjectionLayer.apply(input1, input2, self.requires_grad)
