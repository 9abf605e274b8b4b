"""-m gpu: the kernels of csrc/dainnet.hip and the Charbonnier entries of csrc/loss.hip on the smallest shapes at which they can go wrong.

Numeric gate (the project's usual one): |kernel - float64| <= max(3 E, 4 * 2^-24 * scale), E = the largest |float32 host computation with
torch's own ops - float64| of the same quantity, scale = the largest |float64|.  Pooling, nearest x2 + add and add + ReLU are compared
bit for bit with the host composition.  Every kernel: a graph replay equals the eager result bit for bit.  A run with -s prints one
DAIN_OPS_PARITY line per comparison; the worst per kernel belong in profiles/dain_net_parity.txt.

BatchNorm shapes: a count of 2 (N=2, 1x1 planes), an odd plane that is no multiple of 4 in two groups, the hourglass's widest layer at
64x64, and one case on each side of the launcher's one partition threshold (16384 values per group and channel: one workgroup up to
it, 8192-value pieces of a plane above), the split also with a plane that is no multiple of 4 and with two groups.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from meta_interpolation_amd import hip_ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
FLOOR, K = 4 * 2.0 ** -24, 3.0


def gate_check(what, got, r32, r64):
    got, r32, r64 = (np.asarray(t, np.float64) for t in (got, r32, r64))
    assert got.shape == r64.shape and np.isfinite(got).all(), what
    E, scale = float(np.abs(r32 - r64).max()), float(np.abs(r64).max())
    gate = max(K * E, FLOOR * scale)
    err = float(np.abs(got - r64).max())
    print('DAIN_OPS_PARITY %s err=%.3e E=%.3e scale=%.3e gate=%.3e err/gate=%.3f' % (what, err, E, scale, gate, err / gate if gate else 0.0))
    assert err <= gate, (what, err, gate)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def rand(shape, seed, lo=-1.0, hi=1.0):
    return torch.from_numpy(np.random.default_rng(seed).uniform(lo, hi, shape).astype(np.float32))


# ---------------------------------------------------------------------------------------------------------------------------------
# BatchNorm
# ---------------------------------------------------------------------------------------------------------------------------------
BN_SHAPES = {                      # name: (N, n_per_group, C, H, W)
    'count2': (2, 2, 16, 1, 1),
    'odd_two_groups': (4, 2, 32, 3, 5),
    'wide_64x64': (2, 2, 128, 64, 64),
    'threshold_single': (2, 2, 3, 64, 128),          # 16384 values: the last size one workgroup reduces
    'threshold_split': (2, 2, 3, 64, 129),           # 16512: two pieces per plane
    'split_one_plane': (1, 1, 2, 1, 16385),          # three pieces, the last of one value
    'split_odd_plane': (2, 2, 3, 95, 97),            # 9215-value planes: no multiple of 4
    'split_two_groups': (4, 2, 2, 64, 129),
}


def bn_reference(x, npg, gamma, beta, eps, dtype):
    x = x.to(dtype)
    N, C = x.shape[:2]
    g = x.view(N // npg, npg, C, -1)
    mean = g.mean(dim=(1, 3))
    var = g.var(dim=(1, 3), unbiased=False)
    y = (g - mean[:, None, :, None]) / torch.sqrt(var[:, None, :, None] + eps)
    if gamma is not None:
        y = y * gamma.to(dtype)[None, None, :, None] + beta.to(dtype)[None, None, :, None]
    return mean, var, torch.relu(y).view(x.shape)


@pytest.mark.parametrize("name", sorted(BN_SHAPES))
@pytest.mark.parametrize("affine", (False, True))
def test_batchnorm_train_mode_into_a_channel_slice(name, affine):
    N, npg, C, H, W = BN_SHAPES[name]
    x = rand((N, C, H, W), 11, -2.0, 2.0) * rand((1, C, 1, 1), 12, 0.5, 2.0) + rand((1, C, 1, 1), 13, -3.0, 3.0)
    gamma, beta = (rand((C,), 14, 0.5, 1.5), rand((C,), 15)) if affine else (None, None)
    xd = x.to(DEV)
    mean, var = hip_ops.bn_stats(xd, npg)
    c_off, c_total = 5, C + 9
    fill = torch.full((N, c_total, H, W), 1.2345e-20, device=DEV)
    out = hip_ops.bn_apply_relu(xd, mean, var, npg, None if gamma is None else gamma.to(DEV), None if beta is None else beta.to(DEV),
                                1e-5, fill.clone(), c_off)
    torch.cuda.synchronize()
    m64, v64, y64 = bn_reference(x, npg, gamma, beta, 1e-5, torch.float64)
    m32, v32, y32 = bn_reference(x, npg, gamma, beta, 1e-5, torch.float32)
    gate_check('bn_mean %s' % name, mean.cpu(), m32, m64)
    gate_check('bn_var %s' % name, var.cpu(), v32, v64)
    gate_check('bn_out %s affine=%d' % (name, affine), out[:, c_off:c_off + C].cpu(), y32, y64)
    untouched = torch.ones(c_total, dtype=torch.bool)
    untouched[c_off:c_off + C] = False
    assert torch.equal(bits(out[:, untouched]), bits(fill[:, untouched]))            # the other channels: not one bit moved
    # a plain call (own output) gives the slice's bits
    assert torch.equal(hip_ops.bn_apply_relu(xd, mean, var, npg, None if gamma is None else gamma.to(DEV),
                                             None if beta is None else beta.to(DEV)), out[:, c_off:c_off + C])


@pytest.mark.parametrize("name", ('odd_two_groups', 'split_two_groups'))
def test_batchnorm_groups_do_not_depend_on_the_rest_of_the_batch(name):
    N, npg, C, H, W = BN_SHAPES[name]
    x = (rand((N, C, H, W), 21, -2.0, 2.0) + 1.5).to(DEV)
    flat = torch.zeros(2, N // npg, C + 7, device=DEV)                                  # statistics as column slices of a flat buffer
    mean, var = hip_ops.bn_stats(x, npg, flat[0][:, 3:3 + C], flat[1][:, 3:3 + C])
    out = hip_ops.bn_apply_relu(x, mean, var, npg)
    assert not flat[:, :, :3].any() and not flat[:, :, 3 + C:].any()
    for g in range(N // npg):
        alone = x[g * npg:(g + 1) * npg].clone()
        m1, v1 = hip_ops.bn_stats(alone, npg)
        assert torch.equal(m1[0], mean[g]) and torch.equal(v1[0], var[g]), g
        assert torch.equal(hip_ops.bn_apply_relu(alone, m1, v1, npg), out[g * npg:(g + 1) * npg]), g
        shifted = torch.empty(alone.numel() + 1, device=DEV)[1:].view_as(alone).copy_(alone)       # 4-byte aligned only: the same bits
        m2, v2 = hip_ops.bn_stats(shifted, npg)
        assert torch.equal(m2, m1) and torch.equal(v2, v1), g


def test_batchnorm_eval_mode_reads_running_buffers():
    N, C, H, W = 3, 16, 5, 7
    x = rand((N, C, H, W), 31, -2.0, 2.0)
    rm, rv, gamma, beta = rand((C,), 32), rand((C,), 33, 0.5, 1.5), rand((C,), 34, 0.5, 1.5), rand((C,), 35)
    out = hip_ops.bn_apply_relu(x.to(DEV), rm.to(DEV).view(1, C), rv.to(DEV).view(1, C), N, gamma.to(DEV), beta.to(DEV), 1e-5)
    ref = [F.relu(F.batch_norm(x.to(t), rm.to(t), rv.to(t), gamma.to(t), beta.to(t), False, 0.1, 1e-5)) for t in (torch.float32, torch.float64)]
    gate_check('bn_eval', out.cpu(), *ref)


def test_batchnorm_wrapper_errors_and_running_update():
    x = torch.zeros(3, 4, 2, 2, device=DEV)
    with pytest.raises(ValueError, match="multiple"):
        hip_ops.bn_stats(x, 2)
    with pytest.raises(ValueError, match="more than 1 value"):
        hip_ops.bn_stats(torch.zeros(2, 4, 1, 1, device=DEV), 1)
    with pytest.raises(NotImplementedError):
        with torch.enable_grad():
            hip_ops.bn_stats(x.clone().requires_grad_(), 3)
    with pytest.raises(ValueError):
        hip_ops.bn_apply_relu(x, torch.zeros(1, 4, device=DEV), torch.ones(1, 4, device=DEV), 3, out=torch.zeros(3, 6, 2, 2, device=DEV), c_off=3)
    # 100 buffers of odd sizes: three launches of the multi-tensor update
    sizes = [1 + (7 * i) % 67 for i in range(100)]
    run = [rand((n,), 40 + i) for i, n in enumerate(sizes)]
    stat = [rand((n,), 200 + i) for i, n in enumerate(sizes)]
    unbias = [1.0 + 1.0 / (i + 1) for i in range(100)]
    dev_run = [r.to(DEV) for r in run]
    hip_ops.bn_running_update(dev_run, [s.to(DEV) for s in stat], unbias, 0.1)
    for i in range(100):
        r64 = 0.9 * run[i].double() + 0.1 * (stat[i].double() * unbias[i])
        r32 = (1 - 0.1) * run[i] + 0.1 * (stat[i] * unbias[i])
        got, E = dev_run[i].cpu().double(), float((r32.double() - r64).abs().max())
        assert float((got - r64).abs().max()) <= max(K * E, FLOOR * float(r64.abs().max())), i


# ---------------------------------------------------------------------------------------------------------------------------------
# max-pool, nearest x2 + add, add + ReLU
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", ((2, 2), (5, 7), (64, 64)))
def test_maxpool_equals_torch_bit_for_bit(hw):
    x = rand((2, 3) + hw, 51, -4.0, 4.0)
    flat = x.view(-1)
    flat[::5] = float('-inf')
    flat[3::11] = float('nan')
    flat[0] = float('nan')
    x[1, 2, :2, :2] = float('-inf')                                                    # a window of -inf alone
    got = hip_ops.max_pool2x2(x.to(DEV))
    want = F.max_pool2d(x, 2, 2)
    assert got.shape == want.shape == (2, 3, hw[0] // 2, hw[1] // 2)
    assert torch.isnan(want).any() and torch.isinf(want).any()
    assert torch.equal(bits(got), bits(want))


@pytest.mark.parametrize("hw", ((1, 1), (3, 5)))
def test_upnearest2x_add_equals_the_host_composition(hw):
    low, skip = rand((2, 3) + hw, 61), rand((2, 3, 2 * hw[0], 2 * hw[1]), 62)
    got = hip_ops.upnearest2x_add(low.to(DEV), skip.to(DEV))
    assert torch.equal(bits(got), bits(skip + F.interpolate(low, scale_factor=2, mode='nearest')))
    with pytest.raises(ValueError, match="twice"):
        hip_ops.upnearest2x_add(low.to(DEV), skip[..., :-1].contiguous().to(DEV))


def test_add_relu_forward_and_gradient():
    a, r = rand((1, 3, 5, 7), 71), rand((1, 3, 5, 7), 72)
    r.view(-1)[::4] = -a.view(-1)[::4]                                                 # sums that are exactly 0
    ad, rd = a.to(DEV).requires_grad_(), r.to(DEV).requires_grad_()
    y = hip_ops.add_relu(ad, rd)
    want = torch.relu(a + r)
    assert torch.equal(bits(y), bits(want)) and int((want == 0).sum()) > 27
    g = rand(a.shape, 73)
    ga, gr = torch.autograd.grad(y, (ad, rd), g.to(DEV))
    assert torch.equal(ga, gr)
    assert torch.equal(ga.cpu(), g * (want > 0))
    assert not ga.cpu()[want == 0].any()


# ---------------------------------------------------------------------------------------------------------------------------------
# Charbonnier
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", (1, 2))
@pytest.mark.parametrize("n", (1, 3 * 5 * 7, 3 * 64 * 64))
def test_charbonnier_loss_and_gradients(rows, n):
    a = rand((rows, n), 81, 0.0, 255.0)
    b = rand((rows, n), 82, 0.0, 255.0)
    b[:, ::3] = a[:, ::3]                                                              # d == 0 exactly (every element when n == 1)
    if n > 1:
        a[:, 1], b[:, 1] = 255.0, 0.0
    ad, bd = a.to(DEV).requires_grad_(), b.to(DEV).requires_grad_()
    w = rand((rows,), 83, 0.5, 1.5)
    per = hip_ops.charbonnier_loss_per_sample(ad, bd)
    ga, gb = torch.autograd.grad((per * w.to(DEV)).sum(), (ad, bd))
    refs = []
    for t in (torch.float32, torch.float64):
        at, bt = a.to(t).requires_grad_(), b.to(t).requires_grad_()
        d = at - bt
        lt = torch.sqrt(d * d + 1e-8 * 1e-8).mean(1)
        refs.append((lt.detach(),) + torch.autograd.grad((lt * w.to(t)).sum(), (at, bt)))
    gate_check('charbonnier rows=%d n=%d' % (rows, n), per.detach().cpu(), refs[0][0], refs[1][0])
    gate_check('charbonnier_grad_a rows=%d n=%d' % (rows, n), ga.cpu(), refs[0][1], refs[1][1])
    gate_check('charbonnier_grad_b rows=%d n=%d' % (rows, n), gb.cpu(), refs[0][2], refs[1][2])
    zero = (a == b)
    assert not ga.cpu()[zero].any() and not gb.cpu()[zero].any()                      # exactly 0 where d == 0
    if n == 1:
        assert abs(float(per[0]) / 1e-8 - 1.0) < 1e-6                                 # the value there is eps
    if rows == 1:
        whole = hip_ops.charbonnier_loss(ad, bd)
        assert whole.shape == () and torch.equal(whole, per[0])


# ---------------------------------------------------------------------------------------------------------------------------------
# every kernel: a graph replay equals the eager result, bit for bit
# ---------------------------------------------------------------------------------------------------------------------------------
def _charbonnier_with_grad(a, b):
    with torch.enable_grad():
        a = a.detach().requires_grad_()
        loss = hip_ops.charbonnier_loss(a, b)
        return loss, torch.autograd.grad(loss, a)[0]


def _add_relu_with_grad(a, r):
    with torch.enable_grad():
        a = a.detach().requires_grad_()
        y = hip_ops.add_relu(a, r)
        return y, torch.autograd.grad(y, a, r)[0]


def _bn(x, _):
    mean, var = hip_ops.bn_stats(x, 2)
    return mean, var, hip_ops.bn_apply_relu(x, mean, var, 2)


def _running(x, y):
    run = [x.flatten()[:40].clone(), x.flatten()[40:51].clone()]
    hip_ops.bn_running_update(run, [y.flatten()[:40].contiguous(), y.flatten()[40:51].contiguous()], [1.0, 1.5])
    return tuple(run)


GRAPH_CASES = {
    'bn_single': (_bn, (4, 8, 6, 10), (4, 8, 6, 10)),
    'bn_split': (_bn, (2, 2, 64, 129), (2, 2, 64, 129)),
    'bn_running_update': (_running, (2, 4, 4, 4), (2, 4, 4, 4)),
    'maxpool': (lambda x, _: (hip_ops.max_pool2x2(x),), (2, 3, 5, 7), (1,)),
    'upnearest2x_add': (lambda lo, sk: (hip_ops.upnearest2x_add(lo, sk),), (2, 3, 3, 5), (2, 3, 6, 10)),
    'add_relu': (_add_relu_with_grad, (1, 3, 5, 7), (1, 3, 5, 7)),
    'charbonnier': (_charbonnier_with_grad, (1, 3, 5, 7), (1, 3, 5, 7)),
}


@pytest.mark.parametrize("name", sorted(GRAPH_CASES))
def test_graph_replay_equals_eager_bit_for_bit(name):
    fn, sa, sb = GRAPH_CASES[name]
    inputs = [(rand(sa, 90 + i).to(DEV), rand(sb, 95 + i).to(DEV)) for i in range(3)]
    sx, sy = torch.zeros(sa, device=DEV), torch.zeros(sb, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        fn(sx, sy)                                                                     # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        out_g = fn(sx, sy)
    for it, (x, y) in enumerate(inputs):
        sx.copy_(x)
        sy.copy_(y)
        graph.replay()
        torch.cuda.synchronize()
        with torch.no_grad():
            eager = fn(x.clone(), y.clone())
        for k, (p, q) in enumerate(zip(out_g, eager)):
            assert torch.equal(p, q), (name, it, k)
