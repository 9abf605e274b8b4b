"""The U-Net the kernel-predicting plugins share (``--model sepconv``, ``--model adacof``): the builders of its blocks and its pass.

Five encoder ``Basic`` blocks (three 3x3 convolutions with ReLUs) with 2x2 average pooling, four decoder blocks with a bilinear x2
``Upsample`` and a skip connection each; the result is the 64-channel half-resolution map the plugins' heads read.  Parameter names are
the reference's (sepconv/model.py:168-250): ``moduleConv{1..5}.{0,2,4}``, ``moduleDeconv{5..2}.{0,2,4}``, ``moduleUpsample{5..2}.1``.
Only the ``Basic`` blocks read the fast-weight dict; the ``moduleUpsampleN`` always use the module's own parameters (:292-307).
"""
import torch.nn as nn

from . import hip_ops
from .hip_ops import Upsample2x
from .model_utils import MetaConv2dLayer, MetaSequential

ENCODER = [("moduleConv1", 6, 32), ("moduleConv2", 32, 64), ("moduleConv3", 64, 128),
           ("moduleConv4", 128, 256), ("moduleConv5", 256, 512)]
DECODER = [("moduleDeconv5", 512, 512), ("moduleDeconv4", 512, 256), ("moduleDeconv3", 256, 128),
           ("moduleDeconv2", 128, 64)]


def conv(cin, cout):
    return MetaConv2dLayer(in_channels=cin, out_channels=cout, kernel_size=3, stride=1, padding=1)


def basic(cin, cout):
    return MetaSequential(conv(cin, cout), nn.ReLU(inplace=False),
                          conv(cout, cout), nn.ReLU(inplace=False),
                          conv(cout, cout), nn.ReLU(inplace=False))


def upsample(ch):
    return MetaSequential(Upsample2x(align_corners=True), conv(ch, ch), nn.ReLU(inplace=False))


def head(taps):
    """64 -> `taps` planes at full resolution: three half-resolution convolutions, bilinear x2, one more convolution"""
    return MetaSequential(conv(64, 64), nn.ReLU(inplace=False),
                          conv(64, 64), nn.ReLU(inplace=False),
                          conv(64, taps), nn.ReLU(inplace=False),
                          Upsample2x(align_corners=True),
                          conv(taps, taps))


def build(net):
    """Give `net` the encoder (with its poolings) and the decoder, in the reference's registration order."""
    for i, (name, cin, cout) in enumerate(ENCODER, start=1):
        setattr(net, name, basic(cin, cout))
        setattr(net, "modulePool%d" % i, hip_ops.AvgPool2x2())
    for name, cin, cout in DECODER:
        setattr(net, name, basic(cin, cout))
        setattr(net, name.replace("Deconv", "Upsample"), upsample(cout))


def run(net, x, fast, pool_epilogue=True):
    """x [N,6,ph,pw] (ph, pw multiples of 32) -> the combined map [N,64,ph/2,pw/2].  fast(name) -> the block's fast weights or None."""
    skips = []
    for i, (name, _, _) in enumerate(ENCODER, start=1):
        # the block's activated output feeds the pooling and a skip connection: one op with one element-wise pass in backward (the
        # pooling's adjoint + the sum of the two cotangents + the block's last ReLU derivative, which the block leaves to it)
        # (where the block's last layer runs on the F(4x4) kernel, its output stage has stored the pooled map already: pool_epilogue)
        if x.is_cuda:
            res = getattr(net, name)(x, fast(name), defer_last=True, pool_last=pool_epilogue)
            x, slope, pooled = res if pool_epilogue else res + (None,)
            x, skip = (pooled, x) if pooled is not None else hip_ops.avg_pool2x2_and_skip(x, slope)
        else:
            x, slope = getattr(net, name)(x, fast(name), defer_last=True)
            assert slope is None
            x, skip = getattr(net, "modulePool%d" % i)(x), x
        skips.append(skip)
    for name, _, _ in DECODER:
        # (the block's last ReLU has one consumer, the bilinear x2 of its Upsample: its derivative is left to that op's adjoint)
        x, slope = getattr(net, name)(x, fast(name), defer_last=True)
        x = getattr(net, name.replace("Deconv", "Upsample"))(x, in_slope=slope)   # own parameters, as the reference
        x = x + skips.pop()
    return x
