"""DAIN's rectify net ``MetaMultipleBasicBlock_4`` (dain/Resblock/BasicBlock.py): the one part of MetaDAIN the inner loop adapts.

Ten tensors under the reference's names -- block1.0.weight / bias (7x7 from the 437 channels of the front), block{2,3,4}.conv{1,2}.weight
(3x3, no bias), block5.0.weight / bias (3x3 to the frame) -- and its initialisation: MetaConv2dLayer's Xavier-uniform weights and zero
biases (the reference's normal initialisation loops test for nn.Conv2d and never match a MetaConv2dLayer).  ``params`` follows this
package's ParamView convention (model_utils.py); every convolution runs on hip_ops.conv_bias_act through MetaConv2dLayer, a block's
conv -> ReLU -> conv pair with the ReLU's derivative folded into the second convolution's data gradient (model_utils.conv_pair), and a
block's tail ``relu(out + residual)`` is hip_ops.add_relu.

Every layer asks for the direct split-bf16 convolution in its precise form (``direct=True``), as VoxelFlow's layers do: measured on the
rectified frame of a 64 x 64 input against float64, the default routes (Winograd F(4x4) for the 3x3 layers, the plain split for the
7x7) were 3.7 times the host's float32 error with a bias of 2e-7 of the frame's scale, which the mean of the Charbonnier loss does
not average away; the direct form is at 1.5 times, without a bias.
"""
import torch.nn as nn

from ...model_utils import MetaConv2dLayer, MetaSequential, as_view, conv_pair
from ... import hip_ops

__all__ = ['MetaBasicBlock', 'MetaMultipleBasicBlock', 'MetaMultipleBasicBlock_4']


class MetaBasicBlock(nn.Module):
    expansion = 1

    def __init__(self, inplanes, planes, dilation=1, stride=1, downsample=None):
        super(MetaBasicBlock, self).__init__()
        assert downsample is None and stride == 1
        self.conv1 = MetaConv2dLayer(inplanes, planes, kernel_size=3, padding=1, stride=stride, use_bias=False, direct=True)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = MetaConv2dLayer(planes, planes, kernel_size=3, padding=1, stride=stride, use_bias=False, direct=True)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x, params=None):
        pv = as_view(params)
        sub = (lambda n: None) if pv is None else pv.sub
        out = conv_pair(self.conv1, self.conv2, x, sub('conv1'), sub('conv2'), 0.0)
        if x.is_cuda:
            return hip_ops.add_relu(out, x)
        raise NotImplementedError("MetaBasicBlock has no CPU path: its tail is a savfi HIP op")


class MetaMultipleBasicBlock(nn.Module):

    def __init__(self, input_feature, block, num_blocks, intermediate_feature=64, dense=True):
        super(MetaMultipleBasicBlock, self).__init__()
        assert num_blocks == 4, "MetaMultipleBasicBlock_4 is the one configuration MetaDAIN builds"
        self.dense = dense
        self.num_block = num_blocks
        self.intermediate_feature = intermediate_feature

        self.block1 = MetaSequential(*[
            MetaConv2dLayer(input_feature, intermediate_feature, kernel_size=7, stride=1, padding=3, use_bias=True, direct=True),
            nn.ReLU(inplace=True)
        ])
        self.block2 = block(intermediate_feature, intermediate_feature, dilation=1)
        self.block3 = block(intermediate_feature, intermediate_feature, dilation=1)
        self.block4 = block(intermediate_feature, intermediate_feature, dilation=1)
        self.block5 = MetaSequential(*[MetaConv2dLayer(intermediate_feature, 3, 3, 1, 1, direct=True)])

    def forward(self, x, params=None):
        pv = as_view(params)
        sub = (lambda n: None) if pv is None else pv.sub
        x = self.block1(x, params=sub('block1'))
        x = self.block2(x, params=sub('block2'))
        x = self.block3(x, params=sub('block3'))
        x = self.block4(x, params=sub('block4'))
        return self.block5(x, params=sub('block5'))


def MetaMultipleBasicBlock_4(input_feature, intermediate_feature=64):
    model = MetaMultipleBasicBlock(input_feature, MetaBasicBlock, 4, intermediate_feature)
    return model
