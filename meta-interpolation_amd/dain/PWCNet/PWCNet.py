"""PWC-DC-Net (Sun et al., 2018), the flow estimator of DAIN: dain/PWCNet/PWCNet.py of the reference on the gfx950 kernels.

``PWCDCNet(md=4)`` has the reference's 128 parameters under the reference's names (so pwc_net.pth.tar loads with strict=True) and its
Kaiming initialisation; ``forward(x, output_more=False)`` is PWCDCNet.forward:
  - every conv() block and flow predictor runs through hip_ops.conv_bias_act (bias and LeakyReLU(0.1) in the kernel's epilogue); its
    routing decides the kernel, the strided and the dilated layers take its ATen route;
  - the five cost volumes are one launch each with their LeakyReLU fused (csrc/correlation.hip), the four warps one launch each
    (mesh grid, normalisation, two grid_samples, threshold and product in the reference);
  - the transposed convolutions are F.conv_transpose2d.
The reference adapts rectifyNet only and freezes everything else (meta_learning_system.py:96-101), so the estimator runs forward only on
constant weights in every execution mode: forward() runs under torch.no_grad().  The reference's precomputed 4 x 1024 x 2048 mesh grid
and its B_MAX assert have no counterpart (the warp kernel takes x, y from its thread index): a lockstep batch may exceed 4.
PWCDCNet_old is not ported: the reference never selects it.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import _hip, hip_ops
from .correlation_package_pytorch1_0.correlation import Correlation

__all__ = ['pwc_dc_net', 'PWCDCNet']

SLOPE = 0.1


def conv(in_planes, out_planes, kernel_size=3, stride=1, padding=1, dilation=1):
    return nn.Sequential(
        nn.Conv2d(in_planes, out_planes, kernel_size=kernel_size, stride=stride, padding=padding, dilation=dilation, bias=True),
        nn.LeakyReLU(SLOPE))


def predict_flow(in_planes):
    return nn.Conv2d(in_planes, 2, kernel_size=3, stride=1, padding=1, bias=True)


def deconv(in_planes, out_planes, kernel_size=4, stride=2, padding=1):
    return nn.ConvTranspose2d(in_planes, out_planes, kernel_size, stride, padding, bias=True)


class PWCDCNet(nn.Module):
    """PWC-DC net: dilated context network and DenseNet connections."""
    DIRECT = False          # A/B and tests: True = every 3x3 / stride 1 layer on the direct split-bf16 kernel (no Winograd rounding)

    def __init__(self, md=4):
        """md: maximum displacement of the correlation (4 is the one the library builds)"""
        super(PWCDCNet, self).__init__()
        chans = [3, 16, 32, 64, 96, 128, 196]
        for lv in range(1, 7):
            # (level 6 names its strided layer conv6aa and the next one conv6a: kept)
            first, second = ('a', 'aa') if lv < 6 else ('aa', 'a')
            setattr(self, 'conv%d%s' % (lv, first), conv(chans[lv - 1], chans[lv], kernel_size=3, stride=2))
            setattr(self, 'conv%d%s' % (lv, second), conv(chans[lv], chans[lv], kernel_size=3, stride=1))
            setattr(self, 'conv%db' % lv, conv(chans[lv], chans[lv], kernel_size=3, stride=1))

        self.corr = Correlation(pad_size=md, kernel_size=1, max_displacement=md, stride1=1, stride2=1, corr_multiply=1)
        self.leakyRELU = nn.LeakyReLU(SLOPE)

        nd = (2 * md + 1) ** 2
        dd = [128, 256, 352, 416, 448]                  # np.cumsum([128, 128, 96, 64, 32])
        for lv in range(6, 1, -1):
            od = nd if lv == 6 else nd + chans[lv] + 4
            for i, (extra, out) in enumerate(zip([0] + dd[:4], [128, 128, 96, 64, 32])):
                setattr(self, 'conv%d_%d' % (lv, i), conv(od + extra, out, kernel_size=3, stride=1))
            setattr(self, 'predict_flow%d' % lv, predict_flow(od + dd[4]))
            setattr(self, 'deconv%d' % lv, deconv(2, 2, kernel_size=4, stride=2, padding=1))       # deconv2 exists, unused, as in the reference
            if lv > 2:
                setattr(self, 'upfeat%d' % lv, deconv(od + dd[4], 2, kernel_size=4, stride=2, padding=1))

        self.dc_conv1 = conv(od + dd[4], 128, kernel_size=3, stride=1, padding=1, dilation=1)
        self.dc_conv2 = conv(128, 128, kernel_size=3, stride=1, padding=2, dilation=2)
        self.dc_conv3 = conv(128, 128, kernel_size=3, stride=1, padding=4, dilation=4)
        self.dc_conv4 = conv(128, 96, kernel_size=3, stride=1, padding=8, dilation=8)
        self.dc_conv5 = conv(96, 64, kernel_size=3, stride=1, padding=16, dilation=16)
        self.dc_conv6 = conv(64, 32, kernel_size=3, stride=1, padding=1, dilation=1)
        self.dc_conv7 = predict_flow(32)

        for m in self.modules():
            if isinstance(m, nn.Conv2d) or isinstance(m, nn.ConvTranspose2d):
                nn.init.kaiming_normal_(m.weight.data, mode='fan_in')
                if m.bias is not None:
                    m.bias.data.zero_()

        self._filters = {}          # per Conv2d: packed / transformed filters of its weight (hip_ops.filter_lookup)

    def _conv(self, m, x):
        """A conv() block (Conv2d + LeakyReLU(0.1)) or a bare flow predictor, one fused call."""
        c, slope = (m[0], SLOPE) if isinstance(m, nn.Sequential) else (m, 1.0)
        return hip_ops.conv_bias_act(x, c.weight, c.bias, c.stride[0], c.padding[0], c.dilation[0], 1, slope, direct=self.DIRECT,
                                     cache=self._filters.setdefault(id(c), {}))

    def warp(self, x, flo, scale=1.0):
        """x [B,C,H,W] (im2) warped back to im1 by the flow flo * scale [B,2,H,W]"""
        return hip_ops.pwc_warp(x, flo, scale)

    @torch.no_grad()
    def forward(self, x, output_more=False):
        x = x.contiguous()
        _hip.require_cuda(x)                                    # device tensors only: a host tensor raises NotImplementedError
        cv = self._conv
        c1, c2 = [x[:, :3, :, :]], [x[:, 3:, :, :]]           # c1[l-1], c2[l-1]: the level-l features of im1, im2 (index 0: the images)
        for lv in range(1, 7):
            first, second = ('a', 'aa') if lv < 6 else ('aa', 'a')
            for pyr in (c1, c2):
                y = cv(getattr(self, 'conv%d%s' % (lv, first)), pyr[-1])
                y = cv(getattr(self, 'conv%d%s' % (lv, second)), y)
                pyr.append(cv(getattr(self, 'conv%db' % lv), y))

        flows = {}
        up_flow = up_feat = None
        for lv, scale in ((6, None), (5, 0.625), (4, 1.25), (3, 2.5), (2, 5.0)):
            f1, f2 = c1[lv], c2[lv]
            if lv == 6:
                x = self.corr(f1, f2, SLOPE)
            else:
                x = torch.cat((self.corr(f1, self.warp(f2, up_flow, scale), SLOPE), f1, up_flow, up_feat), 1)
            for i in range(5):
                x = torch.cat((cv(getattr(self, 'conv%d_%d' % (lv, i)), x), x), 1)
            flows[lv] = cv(getattr(self, 'predict_flow%d' % lv), x)
            if lv > 2:
                d, u = getattr(self, 'deconv%d' % lv), getattr(self, 'upfeat%d' % lv)
                up_flow = F.conv_transpose2d(flows[lv], d.weight, d.bias, d.stride, d.padding)
                up_feat = F.conv_transpose2d(x, u.weight, u.bias, u.stride, u.padding)

        x = cv(self.dc_conv4, cv(self.dc_conv3, cv(self.dc_conv2, cv(self.dc_conv1, x))))
        flow2 = flows[2] + cv(self.dc_conv7, cv(self.dc_conv6, cv(self.dc_conv5, x)))
        if not output_more:
            return flow2
        return [flow2, flows[3], flows[4], flows[5], flows[6]]


def pwc_dc_net(path=None):
    model = PWCDCNet()
    if path is not None:
        data = torch.load(path)
        if 'state_dict' in data.keys():
            model.load_state_dict(data['state_dict'])
        else:
            model.load_state_dict(data)
    return model
