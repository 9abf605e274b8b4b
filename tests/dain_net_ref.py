"""tests/dain_net_ref.py -- TEST INFRASTRUCTURE (never imported by the product path).

The networks of MetaDAIN around its own ops, restated with torch's host ops from a state dict with the reference's key names, in float64
(the yardstick) or float32 (the arithmetic the reference runs; |float32 - float64| is its own error E of the gates):

  hourglass_forward     dain/MegaDepth/pytorch_DIW_scratch.py        BatchNorm per group of samples, running buffers updated per group
  s2df_forward          dain/S2D_models/S2DF.py  (S2DF_3dense)
  filternet_forward     dain/networks/DAIN.py:662-739  (get_MonoNet5 + forward_singlePath, both heads)
  rectify_forward       dain/Resblock/BasicBlock.py  (MetaMultipleBasicBlock_4), differentiable
  charbonnier           dain/loss_function.py:14-16
  glue                  dain/networks/DAIN.py:572-601 on tests/dain_ops_ref.py: depth inverse, projection, four warps, 437 channels

Weights come from a numpy rule (numpy_rule_state): one default_rng(seed), one draw per key in sorted key order, scaled by fan-in, running
variances positive -- the same tensors wherever they are rebuilt.  tests/golden/dain_net.npz pins these restatements to the reference's
own modules (tools/gen_dain_golden.py); tests/test_dain_net_ref_cpu.py checks that.
"""
import numpy as np
import torch
import torch.nn.functional as F

from tests import dain_ops_ref as O

# inception blocks: (width of the 1x1 branch, ((kernel, middle, width), ...)); levels: the two branches of a ConcatTable
_A = (32, ((3, 32, 32), (5, 32, 32), (7, 32, 32)))
_B = (64, ((3, 32, 64), (5, 32, 64), (7, 32, 64)))
_C = (64, ((3, 64, 64), (7, 64, 64), (11, 64, 64)))
_E = (32, ((3, 64, 32), (7, 64, 32), (11, 64, 32)))
_F = (32, ((3, 64, 32), (5, 64, 32), (7, 64, 32)))
_G = (16, ((3, 32, 16), (7, 32, 16), (11, 32, 16)))
_H = (16, ((3, 64, 16), (7, 64, 16), (11, 64, 16)))
_L1 = [[_B, _B], ['avg', _B, _B, _B, 'up']]
_L2 = [[_B, _C], ['avg', _B, _B, _L1, _B, _C, 'up']]
_L3 = [['max', _A, _B, _L2, _B, _A, 'up'], [_A, _E]]
_L4 = [['max', _A, _A, _L3, _F, _G, 'up'], [_H]]


# ---------------------------------------------------------------------------------------------------------------------------------
# names and shapes
# ---------------------------------------------------------------------------------------------------------------------------------
def _bn_shapes(out, name, c, affine):
    if affine:
        out[name + '.weight'], out[name + '.bias'] = (c,), (c,)
    out[name + '.running_mean'], out[name + '.running_var'], out[name + '.num_batches_tracked'] = (c,), (c,), ()


def _conv_shapes(out, name, ci, co, k, bias=True):
    out[name + '.weight'] = (co, ci, k, k)
    if bias:
        out[name + '.bias'] = (co,)


def _level_shapes(out, pre, cin, spec):
    for j, items in enumerate(spec):
        c = cin
        for p, it in enumerate(items):
            here = '%s0.%d.%d' % (pre, j, p)
            if isinstance(it, str):
                continue
            if isinstance(it, list):
                _level_shapes(out, here + '.', c, it)
                continue
            first, rest = it
            _conv_shapes(out, here + '.0.0', c, first, 1)
            _bn_shapes(out, here + '.0.1', first, False)
            for b, (k, mid, width) in enumerate(rest, 1):
                _conv_shapes(out, '%s.%d.0' % (here, b), c, mid, 1)
                _bn_shapes(out, '%s.%d.1' % (here, b), mid, False)
                _conv_shapes(out, '%s.%d.3' % (here, b), mid, width, k)
                _bn_shapes(out, '%s.%d.4' % (here, b), width, False)
            c = first + sum(r[2] for r in rest)


def hourglass_shapes():
    """The 779 tensors of the reference's pytorch_DIW_scratch.state_dict(), in its order."""
    out = {}
    _conv_shapes(out, '0', 3, 128, 7)
    _bn_shapes(out, '1', 128, True)
    _level_shapes(out, '3.', 128, _L4)
    _conv_shapes(out, '4', 64, 1, 3)
    return out


def s2df_shapes():
    return {'block1.0.weight': (64, 3, 7, 7), 'block2.conv1.weight': (64, 64, 3, 3), 'block2.conv2.weight': (64, 64, 3, 3),
            'block3.conv1.weight': (64, 64, 3, 3), 'block3.conv2.weight': (64, 64, 3, 3)}


RECTIFY_NAMES = ['block1.0.weight', 'block1.0.bias'] + ['block%d.conv%d.weight' % (b, c) for b in (2, 3, 4) for c in (1, 2)] + \
                ['block5.0.weight', 'block5.0.bias']


def rectify_shapes(cin=437, mid=128):
    out = {'block1.0.weight': (mid, cin, 7, 7), 'block1.0.bias': (mid,)}
    for b in (2, 3, 4):
        out['block%d.conv1.weight' % b] = out['block%d.conv2.weight' % b] = (mid, mid, 3, 3)
    out['block5.0.weight'], out['block5.0.bias'] = (3, mid, 3, 3), (3,)
    return out


_TRUNK = [(0, 6, 16), (2, 16, 32), (5, 32, 64), (8, 64, 128), (11, 128, 256), (14, 256, 512), (17, 512, 512), (20, 512, 256),
          (23, 256, 128), (26, 128, 64), (29, 64, 32), (32, 32, 16)]
_POOLS, _UPS = (4, 7, 10, 13, 16), (19, 22, 25, 28, 31)


def filternet_shapes():
    """initScaleNets_filter (the flat ModuleList of get_MonoNet5), initScaleNets_filter1 / 2 (conv, ReLU, conv)."""
    out = {}
    for i, ci, co in _TRUNK:
        _conv_shapes(out, 'initScaleNets_filter.%d' % i, ci, co, 3)
    for head in ('initScaleNets_filter1', 'initScaleNets_filter2'):
        _conv_shapes(out, head + '.0', 16, 16, 3)
        _conv_shapes(out, head + '.2', 16, 16, 3)
    return out


def metadain_shapes():
    """Every tensor of MetaDAIN.state_dict() outside the flow estimator (tests/pwc_ref.py has that one)."""
    out = dict(filternet_shapes())
    out.update({'ctxNet.' + k: v for k, v in s2df_shapes().items()})
    out.update({'rectifyNet.' + k: v for k, v in rectify_shapes().items()})
    out.update({'depthNet.' + k: v for k, v in hourglass_shapes().items()})
    return out


def numpy_rule_state(shapes, seed, gain=1.0):
    """{name: tensor} for {name: shape}: one default_rng(seed), keys in sorted order.  Weights: normal * gain * sqrt(2 / fan_in);
    biases and running means: normal * 0.1; running variances and BatchNorm weights: uniform(0.5, 1.5); counters: 0."""
    rng = np.random.default_rng(seed)
    out = {}
    for name in sorted(shapes):
        shape = tuple(shapes[name])
        if name.endswith('num_batches_tracked'):
            out[name] = torch.zeros((), dtype=torch.int64)
            continue
        if name.endswith('running_var') or (len(shape) == 1 and name.endswith('.weight')):
            a = rng.uniform(0.5, 1.5, shape)
        elif len(shape) == 4:
            a = rng.standard_normal(shape) * (gain * np.sqrt(2.0 / (shape[1] * shape[2] * shape[3])))
        else:
            a = rng.standard_normal(shape) * 0.1
        out[name] = torch.from_numpy(a.astype(np.float32))
    return out


def numpy_rule_frames(shape, seed):
    return torch.from_numpy(np.random.default_rng(seed).uniform(0.0, 1.0, shape).astype(np.float32))


def golden_view(kind, size, a):
    """The part of an output tests/golden/dain_net.npz keeps (the fixture stays small): everything at the small size, a regular
    subsample of pixels (and of the context / filter channels) at the large one."""
    step = 1 if size <= 16 else size // 16
    if kind == 'ctx':
        return a[:, 3::32, ::step, ::step]
    if kind == 'heads':
        return a[:, :, ::4, ::step, ::step]
    return a[..., ::step, ::step] if size > 16 else a


def _golden_buffers():
    rv = [k for k in hourglass_shapes() if k.endswith('running_var')]
    picked = [rv[0], rv[len(rv) // 2], rv[-1]]
    return picked + [k.replace('running_var', 'running_mean') for k in picked] + ['1.num_batches_tracked']


GOLDEN_BUFFERS = _golden_buffers()      # the running buffers the fixture keeps whole (plus the sums over all of them)


def _cast(sd, dtype):
    return {k: (v.detach().to('cpu', dtype, copy=True) if v.is_floating_point() else v.detach().cpu().clone()) for k, v in sd.items()}      # (always a copy: the running buffers are updated in place)


# ---------------------------------------------------------------------------------------------------------------------------------
# the hourglass
# ---------------------------------------------------------------------------------------------------------------------------------
def bn_relu_groups(x, rm, rv, w, b, training, npg, eps=1e-5, momentum=0.1):
    """relu(BatchNorm2d(x)) with every group of npg consecutive samples a call of its own (rm, rv updated per group, in order)."""
    if not training:
        return F.relu(F.batch_norm(x, rm, rv, w, b, False, momentum, eps))
    return F.relu(torch.cat([F.batch_norm(x[g:g + npg], rm, rv, w, b, True, momentum, eps) for g in range(0, x.shape[0], npg)], 0))


def hourglass_forward(sd, x, dtype=torch.float64, training=True, n_per_group=None):
    """-> (log depth [N,1,H,W], state dict after the call: running buffers and counters moved as by one reference forward per group)."""
    sd = _cast(sd, dtype)
    x = x.detach().to('cpu', dtype)
    npg = x.shape[0] if n_per_group is None else n_per_group
    groups = x.shape[0] // npg

    def unit(name_conv, name_bn, t):
        w = sd[name_conv + '.weight']
        t = F.conv2d(t, w, sd[name_conv + '.bias'], 1, (w.shape[2] - 1) // 2)
        if training:
            sd[name_bn + '.num_batches_tracked'] += groups
        return bn_relu_groups(t, sd[name_bn + '.running_mean'], sd[name_bn + '.running_var'], sd.get(name_bn + '.weight'),
                              sd.get(name_bn + '.bias'), training, npg)

    def level(pre, t, spec):
        outs = []
        for j, items in enumerate(spec):
            y = t
            for p, it in enumerate(items):
                here = '%s0.%d.%d' % (pre, j, p)
                if it == 'max':
                    y = F.max_pool2d(y, 2, 2)
                elif it == 'avg':
                    y = F.avg_pool2d(y, 2, 2)
                elif it == 'up':
                    y = F.interpolate(y, scale_factor=2, mode='nearest')
                elif isinstance(it, list):
                    y = level(here + '.', y, it)
                else:
                    parts = [unit(here + '.0.0', here + '.0.1', y)]
                    for b in range(1, len(it[1]) + 1):
                        parts.append(unit('%s.%d.3' % (here, b), '%s.%d.4' % (here, b), unit('%s.%d.0' % (here, b), '%s.%d.1' % (here, b), y)))
                    y = torch.cat(parts, 1)
            outs.append(y)
        return outs[0] + outs[1]

    with torch.no_grad():
        y = unit('0', '1', x)
        y = level('3.', y, _L4)
        y = F.conv2d(y, sd['4.weight'], sd['4.bias'], 1, 1)
    return y, sd


def s2df_forward(sd, x, dtype=torch.float64):
    sd = _cast(sd, dtype)
    x = x.detach().to('cpu', dtype)
    with torch.no_grad():
        y = [x, F.relu(F.conv2d(x, sd['block1.0.weight'], None, 1, 3))]
        for blk, dil in (('block2', 4), ('block3', 8)):
            t = F.relu(F.conv2d(y[-1], sd[blk + '.conv1.weight'], None, 1, dil, dil))
            y.append(F.relu(F.conv2d(t, sd[blk + '.conv2.weight'], None, 1, 1) + y[-1]))
    return torch.cat(y, 1)


def filternet_forward(sd, x, dtype=torch.float64):
    """x [B,6,H,W] -> (trunk [B,16,H,W], head 1, head 2): forward_singlePath's stack logic over the flat module list."""
    sd = _cast(sd, dtype)
    t = x.detach().to('cpu', dtype)
    convs = {i for i, _, _ in _TRUNK}
    stack = []
    with torch.no_grad():
        for k in range(35):
            if k in convs:
                t = F.relu(F.conv2d(t, sd['initScaleNets_filter.%d.weight' % k], sd['initScaleNets_filter.%d.bias' % k], 1, 1))
            elif k in _POOLS:
                stack.append(t)
                t = F.max_pool2d(t, 2)
            elif k in _UPS:
                t = F.interpolate(t, scale_factor=2, mode='bilinear', align_corners=False) + stack.pop()
        heads = []
        for h in ('initScaleNets_filter1', 'initScaleNets_filter2'):
            u = F.relu(F.conv2d(t, sd[h + '.0.weight'], sd[h + '.0.bias'], 1, 1))
            heads.append(F.conv2d(u, sd[h + '.2.weight'], sd[h + '.2.bias'], 1, 1))
    return t, heads[0], heads[1]


def rectify_forward(params, x, masks=None):
    """MetaMultipleBasicBlock_4 on `params` ({name: tensor}, differentiable) in the dtype of x.  masks: the seven ReLU decisions
    (block1; then conv1's and the tail's of blocks 2-4) as 0 / 1 tensors taken elsewhere -- a device's own --: relu(z) becomes
    z * mask, the same function wherever the decisions agree and a smooth one in between, so that a pre-activation within rounding of
    0 cannot turn the rounding of a forward pass into a whole pixel's term of a gradient."""
    it = iter(masks) if masks is not None else None
    act = (lambda z: F.relu(z)) if it is None else (lambda z: z * next(it).to(z.dtype))
    t = act(F.conv2d(x, params['block1.0.weight'], params['block1.0.bias'], 1, 3))
    for b in (2, 3, 4):
        u = act(F.conv2d(t, params['block%d.conv1.weight' % b], None, 1, 1))
        t = act(F.conv2d(u, params['block%d.conv2.weight' % b], None, 1, 1) + t)
    return F.conv2d(t, params['block5.0.weight'], params['block5.0.bias'], 1, 1)


def charbonnier(a, b, eps=1e-8):
    d = a - b
    return torch.mean(torch.sqrt(d * d + eps * eps))


def rectify_loss_and_grads(sd, rectify_input, cur_output, target, dtype=torch.float64):
    """-> (rectified frame, loss, {name: gradient}) of charbonnier(rectifyNet(rectify_input) + cur_output - target)."""
    params = {k: v.detach().to('cpu', dtype).requires_grad_() for k, v in sd.items()}
    out = rectify_forward(params, rectify_input.detach().to('cpu', dtype)) + cur_output.detach().to('cpu', dtype)
    loss = charbonnier(out, target.detach().to('cpu', dtype))
    grads = torch.autograd.grad(loss, [params[k] for k in RECTIFY_NAMES])
    return out.detach(), loss.detach(), dict(zip(RECTIFY_NAMES, grads))


# ---------------------------------------------------------------------------------------------------------------------------------
# the glue of MetaDAIN.forward (DAIN.py:572-601) from the upstream tensors
# ---------------------------------------------------------------------------------------------------------------------------------
def glue(input0, input2, log_depth, ctx, filters, flows, dtype=np.float64, warp_offsets=None):
    """numpy arrays: frames [B,3,H,W], log_depth 2 x [B,1,H,W], ctx 2 x [B,195,H,W], filters 2 x [B,16,H,W], flows 2 x [B,2,H,W] (the
    x4 flows before the projection) -> dict with depth_inv, offsets, refs, ctx_warped, cur_output, rectify_input.  warp_offsets: the
    projected flows the four warps take their positions from (a device's own, so that its rounding of a projected flow cannot move a
    floor of the warp); default: this function's projections, rounded to float32."""
    tt = torch.float64 if dtype == np.float64 else torch.float32
    depth_inv = [(1e-6 + 1 / torch.exp(torch.from_numpy(d).to(tt))).numpy() for d in log_depth]
    # index decisions of the two ops are taken in float32 from float32 inputs, as the kernels take them
    offsets = [O.depthflowproj_forward(flows[i].astype(np.float32), depth_inv[i].astype(np.float32), True, dtype)[0] for i in range(2)]
    off32 = [o.astype(np.float32) for o in (offsets if warp_offsets is None else warp_offsets)]
    full = [np.concatenate((ctx[i], log_depth[i]), 1) for i in range(2)]
    ctx_warped = [O.filterinterp_forward(full[i], off32[i], filters[i], dtype) for i in range(2)]
    refs = [O.filterinterp_forward(f, off32[i], filters[i], dtype) for i, f in enumerate((input0, input2))]
    cur_output = refs[0] / dtype(2.0) + refs[1] / dtype(2.0)
    rectify_input = np.concatenate((cur_output, refs[0], refs[1], offsets[0], offsets[1], filters[0].astype(dtype),
                                    filters[1].astype(dtype), ctx_warped[0], ctx_warped[1]), 1)
    return {'depth_inv': depth_inv, 'offsets': offsets, 'refs': refs, 'ctx_warped': ctx_warped, 'cur_output': cur_output,
            'rectify_input': rectify_input}
