"""DAIN's context extractor ``S2DF_3dense`` (dain/S2D_models/S2DF.py): a 7x7 convolution and two residual blocks with dilations 4 and 8,
none with a bias, whose three 64-channel maps are concatenated behind the frame: 3 + 3 * 64 = 195 channels.

The reference's names (block1.0.weight, block{2,3}.conv{1,2}.weight) and its initialisation (normal, sqrt(2 / (k * k * out))).  Every
convolution runs through hip_ops.conv_bias_act with its ReLU in the epilogue (the dilated layers take its ATen route) and each block's
``relu(out + residual)`` is one pass (hip_ops.add_relu).  Forward only: the net is frozen on every path of the reference's system.
"""
import math

import torch
import torch.nn as nn

from ... import _hip, hip_ops

__all__ = ['S2DF', 'S2DF_3dense', 'BasicBlock']


def conv3x3(in_planes, out_planes, dilation=1, stride=1):
    "3x3 convolution with padding"
    return nn.Conv2d(in_planes, out_planes, kernel_size=3, stride=stride, padding=int(dilation * (3 - 1) / 2), dilation=dilation, bias=False)


def _conv(c, x, slope, cache):
    return hip_ops.conv_bias_act(x, c.weight, c.bias, c.stride[0], c.padding[0], c.dilation[0], 1, slope, cache=cache.setdefault(id(c), {}))


class BasicBlock(nn.Module):
    expansion = 1

    def __init__(self, inplanes, planes, dilation=1, stride=1, downsample=None):
        super(BasicBlock, self).__init__()
        assert downsample is None
        self.conv1 = conv3x3(inplanes, planes, dilation, stride)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = conv3x3(planes, planes)
        self.downsample = downsample
        self.stride = stride
        self._filters = {}

    def forward(self, x):
        out = _conv(self.conv2, _conv(self.conv1, x, 0.0, self._filters), 1.0, self._filters)
        return hip_ops.add_relu(out, x)


class S2DF(nn.Module):

    def __init__(self, block, num_blocks, dense=True, dilation=True):
        self.inplanes = 64
        super(S2DF, self).__init__()
        assert num_blocks == 3 and dense, "S2DF_3dense is the one configuration MetaDAIN builds"
        self.dense = dense
        self.num_block = num_blocks
        self.block1 = nn.Sequential(*[
            nn.Conv2d(3, 64, kernel_size=7, stride=1, padding=3, bias=False),
            nn.ReLU(inplace=True)
        ])
        self.dilation = dilation
        self.block2 = block(self.inplanes, 64, dilation=4 if dilation else 1)
        self.block3 = block(self.inplanes, 64, dilation=8 if dilation else 1)
        self.block4 = None
        self._filters = {}

        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                n = m.kernel_size[0] * m.kernel_size[1] * m.out_channels
                m.weight.data.normal_(0, math.sqrt(2. / n))

    @torch.no_grad()
    def forward(self, x):
        x = x.contiguous()
        _hip.require_cuda(x)                                    # device tensors only: a host tensor raises NotImplementedError
        y1 = _conv(self.block1[0], x, 0.0, self._filters)
        y2 = self.block2(y1)
        y3 = self.block3(y2)
        return torch.cat([x, y1, y2, y3], dim=1)


def S2DF_3dense():
    model = S2DF(BasicBlock, 3, dense=True)
    return model
