"""MetaDAIN (Bao et al., 2019): the depth-aware interpolation network of the reference's dain/networks/DAIN.py:423-846 on the gfx950 kernels.

The reference adapts ``rectifyNet`` only and freezes everything else (meta_learning_system.py:96-101); MetaDAIN.forward hands ``params`` to
rectifyNet alone (DAIN.py:603-608).  So everything up to ``rectify_input`` and ``cur_output`` -- two hourglass passes, two PWC-Net passes,
the context net twice, the filter net, two projections and four warps -- is a function of the frames and of constants.  Here it is
``front(frame0, frame1)``, run under no_grad, and ``forward(frame0, frame1, params, front=...)`` is the rectify net on a given front:
a caller that adapts on a triplet evaluates its front once and passes it to every pass over that triplet.  ``forward`` computes the
front itself when none is given (the reference's structure; ``reuse_front = False`` tells the system to do that on every pass).
``front(..., out=alloc_front(...))`` builds the front in place at fixed addresses (the four warps write their channel slices of the rectify
input), and ``forward(..., update_stats=False)`` with ``replay_running_stats`` lets a caller run several tasks' passes on shared fronts
and still move the running statistics in the sequential loop's order: what the lockstep and hipGraph paths (--dain_task_modes 1) use.

Kept from the reference: the sub-networks' names (dain_base.pth loads by name), the order of constructing and initialising them, the stack
logic of the filter net, div_flow = 20 and the bilinear x4 of the flows, the reflection padding to multiples of 64 and its inverse.
The depth net runs with BatchNorm statistics per task in training mode (dain/MegaDepth/MegaDepth_model.py); a front keeps them and every
forward on it applies the running-statistics update the reference's forward would have made.  The streams and the device synchronisation
of the reference's forward have no counterpart, and neither has the Charbonnier term of the unrectified frame, which it weights with 0.0
(DAIN.py:639): forward returns the unpadded rectified frame and the system applies the loss.  No CPU path.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import _hip, hip_ops
from ...model_utils import MetaConv2dLayer, as_view, zero_grad_params
from ..my_package.FilterInterpolation import FilterInterpolationModule
from ..my_package.DepthFlowProjection import DepthFlowProjectionModule
from .. import S2D_models
from .. import Resblock
from .. import MegaDepth
from ..PWCNet.PWCNet import pwc_dc_net

__all__ = ['MetaDAIN', 'Front']


class Stack:
    def __init__(self):
        self.stack = []

    def pop(self):
        return self.stack.pop() if self.stack else None

    def push(self, val):
        return self.stack.append(val)


class Front:
    """What the frozen part of MetaDAIN makes of one batch of frame pairs: ``rectify_input`` [B,437,Hp,Wp], ``cur_output`` [B,3,Hp,Wp],
    ``padding`` (left, right, top, bottom) of the reflection padding, ``bn_stats`` (the depth net's batch statistics, one group per
    pair; None in eval mode) and, when asked for, ``parts``: the intermediate tensors by name."""
    __slots__ = ('rectify_input', 'cur_output', 'padding', 'bn_stats', 'parts')

    def __init__(self, rectify_input, cur_output, padding, bn_stats, parts=None):
        self.rectify_input, self.cur_output, self.padding, self.bn_stats, self.parts = rectify_input, cur_output, padding, bn_stats, parts


class MetaDAIN(torch.nn.Module):
    graph_capture = False     # by default this plugin takes the sequential eager task body (graph_inner_loop.supported); --dain_task_modes 1
                              # sets graph_capture and lockstep_tasks on the system's INSTANCE
    reuse_front = True        # A/B (bench, tests): False = the system recomputes the front on every pass, as the reference does

    def __init__(self, channel=3, filter_size=4, timestep=0.5, training=True, resume=False):
        super(MetaDAIN, self).__init__()
        self.filter_size = filter_size
        self.timestep = timestep
        assert (timestep == 0.5)
        self.numFrames = int(1.0 / timestep) - 1

        self.initScaleNets_filter, self.initScaleNets_filter1, self.initScaleNets_filter2 = \
            self.get_MonoNet5(channel, filter_size * filter_size, "filter")

        self.ctxNet = S2D_models.__dict__['S2DF_3dense']()
        self.ctx_ch = 3 * 64 + 3

        self.rectifyNet = Resblock.__dict__['MetaMultipleBasicBlock_4'](3 + 3 + 3 + 2 * 1 + 2 * 2 + 16 * 2 + 2 * self.ctx_ch, 128)

        self._initialize_weights()

        # the released weights of the two estimators are read where the reference reads its base model: with `resume`
        self.flownets = pwc_dc_net("dain/PWCNet/pwc_net.pth.tar" if resume else None)
        self.div_flow = 20.0
        self.depthNet = MegaDepth.__dict__['HourGlass'](
            "dain/MegaDepth/checkpoints/test_local/best_generalization_net_G.pth" if resume else None)

        self._filters = {}
        self.front_evaluations = 0          # frame pairs front() has been evaluated on

        if resume:
            print('loading pretrained model from pretrained_models/dain_base.pth')
            self.load_state_dict(torch.load('pretrained_models/dain_base.pth', map_location='cpu', weights_only=False))

    def _initialize_weights(self):
        for m in self.modules():
            if isinstance(m, nn.Conv2d) or isinstance(m, MetaConv2dLayer):
                nn.init.xavier_uniform_(m.weight.data)
                if m.bias is not None:
                    m.bias.data.zero_()
            elif isinstance(m, nn.BatchNorm2d):
                m.weight.data.fill_(1)
                m.bias.data.zero_()
            elif isinstance(m, nn.Linear):
                m.weight.data.normal_(0, 0.01)
                m.bias.data.zero_()

    def freeze_front(self):
        """The reference's freeze (meta_learning_system.py:96-101): only rectifyNet keeps requires_grad."""
        for k, v in self.named_parameters():
            v.requires_grad = k.find('rectifyNet') >= 0

    # ------------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def paddings(h, w):
        """(left, right, top, bottom) of the reflection padding to multiples of 64."""
        sh = 6
        pw = 0 if w == ((w >> sh) << sh) else (((w >> sh) + 1) << sh) - w
        ph = 0 if h == ((h >> sh) << sh) else (((h >> sh) + 1) << sh) - h
        return (pw // 2, pw - pw // 2, ph // 2, ph - ph // 2)

    @staticmethod
    def unpad(x, padding):
        left, right, top, bottom = padding
        return x[..., top:x.shape[-2] - bottom, left:x.shape[-1] - right]

    # channels of rectify_input: cur_output, ref0, ref2, the two offsets, the two filter sets, the two warped contexts
    RECTIFY_CHANNELS = 437
    _SLICES = {'cur_output': 0, 'ref0': 3, 'ref2': 6, 'offset0': 9, 'offset1': 11, 'filter0': 13, 'filter1': 29, 'ctx0': 45, 'ctx2': 241}

    @classmethod
    def alloc_front(cls, B, H, W, device):
        """A Front for B pairs of H x W frames whose ``rectify_input`` and ``cur_output`` are allocated (zeroed) for the padded size:
        what ``front(..., out=)`` fills in place, call after call, at fixed addresses (graph_inner_loop.py)."""
        padding = cls.paddings(H, W)
        Hp, Wp = H + padding[2] + padding[3], W + padding[0] + padding[1]
        return Front(torch.zeros(B, cls.RECTIFY_CHANNELS, Hp, Wp, device=device), torch.zeros(B, 3, Hp, Wp, device=device), padding, None)

    @torch.no_grad()
    def front(self, frame0, frame1, keep_parts=False, out=None):
        """Everything of the reference's forward that does not depend on ``params``, for B frame pairs [B,3,H,W] at once; each pair is
        one BatchNorm group of the depth net.  Returns a Front.

        ``out``: a Front of alloc_front(B, H, W, device) to fill in place: the four warps write their channel slices of its
        ``rectify_input`` themselves, the other 39 channels are copied in, ``cur_output`` is written, ``bn_stats`` (and ``parts``) are
        replaced -- the same bits as without ``out``, no 437-channel temporary, and ``out`` is what is returned."""
        _hip.require_cuda(frame0.contiguous(), frame1.contiguous())
        assert frame0.shape == frame1.shape and frame0.dim() == 4
        B = frame0.shape[0]
        padding = self.paddings(frame0.shape[2], frame0.shape[3])
        if out is not None:
            Hp, Wp = frame0.shape[2] + padding[2] + padding[3], frame0.shape[3] + padding[0] + padding[1]
            if (tuple(out.rectify_input.shape) != (B, self.RECTIFY_CHANNELS, Hp, Wp) or tuple(out.cur_output.shape) != (B, 3, Hp, Wp)
                    or tuple(out.padding) != tuple(padding)):
                raise ValueError("front(out=): %s / %s is no Front of alloc_front for %d pairs of %d x %d frames"
                                 % (tuple(out.rectify_input.shape), tuple(out.cur_output.shape), B, frame0.shape[2], frame0.shape[3]))
            _hip.require_cuda(out.rectify_input, out.cur_output)
        self.front_evaluations += B
        if any(padding):
            pad = nn.ReflectionPad2d(list(padding))
            frame0, frame1 = pad(frame0), pad(frame1)
        cur_input_0, cur_input_2 = frame0.contiguous(), frame1.contiguous()
        cur_offset_input = torch.cat((cur_input_0, cur_input_2), dim=1)
        cur_filter_input = cur_offset_input
        time_offsets = [kk * self.timestep for kk in range(1, 1 + self.numFrames, 1)]

        # the reference's batch is cat((frame0, frame2), 0) of ONE pair; for B pairs the two frames of a pair stay adjacent: a group
        temp = self.depthNet(torch.stack((cur_input_0, cur_input_2), dim=1).flatten(0, 1), 2)
        temp = temp.view(B, 2, *temp.shape[1:])
        log_depth = [temp[:, 0], temp[:, 1]]
        bn_stats = self.depthNet.last_stats if self.depthNet.training else None

        # every other frozen net runs pair by pair: which kernel a convolution takes depends on its batch, and a pair's front must be,
        # bit for bit, that of a call of its own (the system's fused support pairs and single passes then see the same numbers)
        def per_pair(fn, *tensors):
            if B == 1:
                return fn(*tensors)
            outs = [fn(*[t[i:i + 1] for t in tensors]) for i in range(B)]
            if isinstance(outs[0], (list, tuple)):
                return [torch.cat([o[k] for o in outs], 0) for k in range(len(outs[0]))]
            return torch.cat(outs, 0)
        ctx = [per_pair(self.ctxNet, cur_input_0), per_pair(self.ctxNet, cur_input_2)]
        cur_ctx_output = [torch.cat((ctx[0], log_depth[0]), dim=1), torch.cat((ctx[1], log_depth[1]), dim=1)]
        temp = per_pair(lambda t: self.forward_singlePath(self.initScaleNets_filter, t, 'filter'), cur_filter_input)
        cur_filter_output = [per_pair(lambda t: self.forward_singlePath(self.initScaleNets_filter1, t, name=None), temp),
                             per_pair(lambda t: self.forward_singlePath(self.initScaleNets_filter2, t, name=None), temp)]
        depth_inv = [1e-6 + 1 / torch.exp(d) for d in log_depth]

        flows = [per_pair(lambda t: self.forward_flownets(self.flownets, t, time_offsets=time_offsets), cur_offset_input),
                 per_pair(lambda t: self.forward_flownets(self.flownets, t, time_offsets=time_offsets[::-1]),
                          torch.cat((cur_input_2, cur_input_0), dim=1))]
        cur_offset_outputs = [self.FlowProject(flows[0], depth_inv[0]), self.FlowProject(flows[1], depth_inv[1])]

        cur_offset_output = [cur_offset_outputs[0][0], cur_offset_outputs[1][0]]
        parts = None
        if keep_parts:
            parts = {'input0': cur_input_0, 'input2': cur_input_2, 'log_depth': log_depth, 'ctx': ctx, 'filter_trunk': temp,
                     'filters': cur_filter_output, 'depth_inv': depth_inv, 'flows': [flows[0][0], flows[1][0]],
                     'offsets': cur_offset_output}
        if out is not None:
            return self._front_into(out, cur_input_0, cur_input_2, cur_ctx_output, cur_offset_output, cur_filter_output, bn_stats, parts)
        ctx0, ctx2 = self.FilterInterpolate_ctx(cur_ctx_output[0], cur_ctx_output[1], cur_offset_output, cur_filter_output)
        cur_output, ref0, ref2 = self.FilterInterpolate(cur_input_0, cur_input_2, cur_offset_output, cur_filter_output,
                                                        self.filter_size ** 2)
        rectify_input = torch.cat((cur_output, ref0, ref2, cur_offset_output[0], cur_offset_output[1],
                                   cur_filter_output[0], cur_filter_output[1], ctx0, ctx2), dim=1)
        if keep_parts:
            parts.update({'ctx_warped': [ctx0, ctx2], 'refs': [ref0, ref2]})
        return Front(rectify_input, cur_output, padding, bn_stats, parts)

    def _front_into(self, out, input0, input2, ctx, offset, filt, bn_stats, parts):
        """The tail of front() into ``out``: FilterInterpolate_ctx, FilterInterpolate and the concatenation, without the concatenation."""
        ri, at = out.rectify_input, self._SLICES
        for name, src in (('ctx0', ctx[0]), ('ctx2', ctx[1]), ('ref0', input0), ('ref2', input2)):
            k = 0 if name in ('ctx0', 'ref0') else 1
            hip_ops.filter_interpolation_into(ri, at[name], src, offset[k], filt[k])
        ref0, ref2 = ri[:, at['ref0']:at['ref0'] + 3], ri[:, at['ref2']:at['ref2'] + 3]
        torch.add(ref0 / 2.0, ref2 / 2.0, out=out.cur_output)         # FilterInterpolate's ref0_offset / 2.0 + ref2_offset / 2.0
        for name, src in (('cur_output', out.cur_output), ('offset0', offset[0]), ('offset1', offset[1]), ('filter0', filt[0]),
                          ('filter1', filt[1])):
            ri[:, at[name]:at[name] + src.shape[1]].copy_(src)
        if parts is not None:                                          # views of the slices
            n = self.ctx_ch + 1
            parts.update({'ctx_warped': [ri[:, at['ctx0']:at['ctx0'] + n], ri[:, at['ctx2']:at['ctx2'] + n]], 'refs': [ref0, ref2]})
        out.bn_stats, out.parts = bn_stats, parts
        return out

    def replay_running_stats(self, support, target, tasks, passes):
        """The depth net's running-statistics updates of the sequential task loop, for ``tasks`` tasks whose passes ran on shared fronts
        with update_stats=False: ``support`` holds the 2 x tasks support pairs in sample-major order (pair j * tasks + t is support j of
        task t), ``target`` the tasks target pairs; ``passes`` is one task's forwards in order, 's' = a support pass (its two pairs, a
        then b), 't' = a target pass.  Task by task, as the reference's loop applies them.  Eager: never inside a captured graph."""
        if not self.training or support.bn_stats is None:
            return
        for t in range(tasks):
            for p in passes:
                if p == 's':
                    self.depthNet.update_running_stats(support.bn_stats, groups=[t, tasks + t])
                else:
                    self.depthNet.update_running_stats(target.bn_stats, groups=[t])

    def forward(self, frame0, frame1, params=None, front=None, update_stats=True, **kwargs):
        """The rectified middle frame [B,3,H,W] of frame0, frame1 [B,3,H,W]; ``params``: fast weights of rectifyNet (names with or
        without the 'rectifyNet.' prefix of the inner-loop dictionary; stacked [T, ...] for T tasks in lockstep over a batch in
        sample-major order); ``front``: front(frame0, frame1) when the caller has it.
        In training mode the depth net's running statistics move as in one reference forward per pair, unless ``update_stats`` is
        False: a caller that runs several tasks' passes on one front (lockstep, captured graphs) replays the updates in the
        sequential loop's order afterwards (replay_running_stats)."""
        if front is None:
            front = self.front(frame0, frame1)
        if update_stats and self.training and front.bn_stats is not None:
            self.depthNet.update_running_stats(front.bn_stats)
        pv = as_view(params)
        if pv is not None and 'rectifyNet' in pv:
            pv = pv.sub('rectifyNet')
        cur_output_rectified = self.rectifyNet(front.rectify_input, params=pv) + front.cur_output
        return self.unpad(cur_output_rectified, front.padding)

    def forward_flownets(self, model, input, time_offsets=None):
        if time_offsets is None:
            time_offsets = [0.5]
        elif type(time_offsets) == float:
            time_offsets = [time_offsets]
        temp = model(input)  # this is a single direction motion results, but not a bidirectional one
        temps = [self.div_flow * temp * time_offset for time_offset in time_offsets]
        temps = [F.interpolate(temp, scale_factor=4, mode='bilinear', align_corners=False) for temp in temps]
        return temps

    '''keep this function'''
    def forward_singlePath(self, modulelist, input, name):
        stack = Stack()
        layers = list(modulelist)
        temp = input
        k = 0
        while k < len(layers):
            layer = layers[k]
            if isinstance(layer, nn.Conv2d):
                # conv (+ the ReLU that follows it) is one fused call
                relu = k + 1 < len(layers) and isinstance(layers[k + 1], nn.ReLU)
                temp = hip_ops.conv_bias_act(temp, layer.weight, layer.bias, 1, layer.padding[0], 1, 1, 0.0 if relu else 1.0,
                                             cache=self._filters.setdefault(id(layer), {}))
                k += 2 if relu else 1
                continue
            # use the pop-pull logic, looks like a stack.
            # met a pooling layer, take its input
            if isinstance(layer, nn.MaxPool2d):
                stack.push(temp)
                temp = hip_ops.max_pool2x2(temp)
            # met a unpooling layer, take its output
            elif isinstance(layer, nn.Upsample):
                temp = hip_ops.upsample_bilinear2x(temp, align_corners=False)
                if name == 'offset':
                    temp = torch.cat((temp, stack.pop()), dim=1)
                else:
                    temp = temp + stack.pop()  # short cut here, but optical flow should concat instead of add
            else:
                temp = layer(temp)
            k += 1
        return temp

    '''keep this funtion'''
    def get_MonoNet5(self, channel_in, channel_out, name):
        '''
        Generally, the MonoNet is aimed to provide a basic module for generating either offset, or filter, or occlusion.

        :param channel_in: number of channels that composed of multiple useful information like reference frame, previous coarser-scale result
        :param channel_out: number of output the offset or filter or occlusion
        :param name: to distinguish between offset, filter and occlusion, since they should use different activations in the last network layer
        :return: output the network model
        '''
        model = []
        # block1
        model += self.conv_relu(channel_in * 2, 16, (3, 3), (1, 1))
        model += self.conv_relu_maxpool(16, 32, (3, 3), (1, 1), (2, 2))  # THE OUTPUT No.5
        # block2
        model += self.conv_relu_maxpool(32, 64, (3, 3), (1, 1), (2, 2))  # THE OUTPUT No.4
        # block3
        model += self.conv_relu_maxpool(64, 128, (3, 3), (1, 1), (2, 2))  # THE OUTPUT No.3
        # block4
        model += self.conv_relu_maxpool(128, 256, (3, 3), (1, 1), (2, 2))  # THE OUTPUT No.2
        # block5
        model += self.conv_relu_maxpool(256, 512, (3, 3), (1, 1), (2, 2))
        # intermediate block5_5
        model += self.conv_relu(512, 512, (3, 3), (1, 1))
        # block 6
        model += self.conv_relu_unpool(512, 256, (3, 3), (1, 1), 2)  # THE OUTPUT No.1 UP
        # block 7
        model += self.conv_relu_unpool(256, 128, (3, 3), (1, 1), 2)  # THE OUTPUT No.2 UP
        # block 8
        model += self.conv_relu_unpool(128, 64, (3, 3), (1, 1), 2)  # THE OUTPUT No.3 UP
        # block 9
        model += self.conv_relu_unpool(64, 32, (3, 3), (1, 1), 2)  # THE OUTPUT No.4 UP
        # block 10
        model += self.conv_relu_unpool(32, 16, (3, 3), (1, 1), 2)  # THE OUTPUT No.5 UP

        # output our final purpose
        branch1 = []
        branch2 = []
        branch1 += self.conv_relu_conv(16, channel_out, (3, 3), (1, 1))
        branch2 += self.conv_relu_conv(16, channel_out, (3, 3), (1, 1))
        return (nn.ModuleList(model), nn.ModuleList(branch1), nn.ModuleList(branch2))

    '''keep this function'''
    @staticmethod
    def FlowProject(inputs, depth=None):
        assert depth is not None, "the projection without depth is not part of MetaDAIN's forward"
        return [DepthFlowProjectionModule(input.requires_grad)(input, depth) for input in inputs]

    '''keep this function'''
    @staticmethod
    def FilterInterpolate_ctx(ctx0, ctx2, offset, filter):
        ctx0_offset = FilterInterpolationModule()(ctx0, offset[0].detach(), filter[0].detach())
        ctx2_offset = FilterInterpolationModule()(ctx2, offset[1].detach(), filter[1].detach())
        return ctx0_offset, ctx2_offset

    '''Keep this function'''
    @staticmethod
    def FilterInterpolate(ref0, ref2, offset, filter, filter_size2):
        ref0_offset = FilterInterpolationModule()(ref0, offset[0], filter[0])
        ref2_offset = FilterInterpolationModule()(ref2, offset[1], filter[1])
        return ref0_offset / 2.0 + ref2_offset / 2.0, ref0_offset, ref2_offset

    '''keep this function'''
    @staticmethod
    def conv_relu_conv(input_filter, output_filter, kernel_size, padding):
        # we actually don't need to use so much layer in the last stages.
        layers = nn.Sequential(
            nn.Conv2d(input_filter, input_filter, kernel_size, 1, padding),
            nn.ReLU(inplace=False),
            nn.Conv2d(input_filter, output_filter, kernel_size, 1, padding),
        )
        return layers

    '''keep this fucntion'''
    @staticmethod
    def conv_relu(input_filter, output_filter, kernel_size, padding):
        layers = nn.Sequential(*[
            nn.Conv2d(input_filter, output_filter, kernel_size, 1, padding),
            nn.ReLU(inplace=False)
        ])
        return layers

    '''keep this function'''
    @staticmethod
    def conv_relu_maxpool(input_filter, output_filter, kernel_size, padding, kernel_size_pooling):
        layers = nn.Sequential(*[
            nn.Conv2d(input_filter, output_filter, kernel_size, 1, padding),
            nn.ReLU(inplace=False),
            nn.MaxPool2d(kernel_size_pooling)
        ])
        return layers

    '''klkeep this function'''
    @staticmethod
    def conv_relu_unpool(input_filter, output_filter, kernel_size, padding, unpooling_factor):
        layers = nn.Sequential(*[
            nn.Upsample(scale_factor=unpooling_factor, mode='bilinear', align_corners=False),
            nn.Conv2d(input_filter, output_filter, kernel_size, 1, padding),
            nn.ReLU(inplace=False),
        ])
        return layers

    def zero_grad(self, params=None):
        zero_grad_params(self, params)

    def restore_backup_stats(self):
        pass
