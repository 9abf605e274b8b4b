"""Float64 restatements of the three groups of small kernels that run in every inner step, plus the seeded inputs their tests share:

* channel attention + residual of CAIN's RCAB (csrc/chanattn.hip; formulas of its header comment and include/savfi_hip.h):
      s = mean_hw t;  a1 = relu(W1 s + b1);  y = sigmoid(W2 a1 + b2);  out = t * y + x          (sample n uses weight set n % T)
  backward with r = sum_hw g * t:
      dz2 = r y (1 - y);  da1 = W2^T dz2;  dz1 = da1 [a1 > 0];  ds = W1^T dz1 / hw;  gt = g * y + ds;  gx = g
      gW2 = sum_n dz2 (x) a1;  gb2 = sum_n dz2;  gW1 = sum_n dz1 (x) s;  gb1 = sum_n dz1       (sums over the samples of a task)
* the four update rules of savfi_mt_update_f32 in both learning-rate modes, with coef = d out / d lr, the learning-rate backward,
  and the L2F per-tensor mean / scale / scale backward (csrc/mt_update.hip).  (1 - beta) is the double difference;
* mean-reduced L1 / MSE rows and their gradients with sign(0) = 0 (csrc/loss.hip).

Nothing here calls hip_ops: tests/test_small_ops_ref_cpu.py holds these statements to autograd and to oracle/rules.py in float64,
so that a wrong reference cannot hide a wrong kernel.
"""
import functools
import math

import numpy as np
import torch

RULE_SGD, RULE_ADAM, RULE_ADAMAX_LSLR, RULE_ADAMAX_MSGD = 0, 1, 2, 3
LR_SCALAR, LR_ELEMENT = 0, 1
BETA1, BETA2, EPS = 0.9, 0.99, 1e-8


# ---------------------------------------------------------------------------------------------
# channel attention
# ---------------------------------------------------------------------------------------------
def ca_inputs(N, T, C, Cr, H, W, seed=0):
    """Seeded fp32 inputs: t, x, g [N,C,H,W]; w1 [T,Cr,C], b1 [T,Cr], w2 [T,C,Cr], b2 [T,C]."""
    gen = torch.Generator().manual_seed(1000 * N + 100 * T + C + 7 * Cr + H * W + seed)
    r = lambda *s: torch.randn(*s, generator=gen)
    return dict(t=r(N, C, H, W), x=r(N, C, H, W), g=r(N, C, H, W), w1=r(T, Cr, C) / math.sqrt(C), b1=r(T, Cr) * 0.1,
                w2=r(T, C, Cr) / math.sqrt(Cr), b2=r(T, C) * 0.1)


def ca_forward(t, x, w1, b1, w2, b2):
    """-> dict(s [N,C], a1 [N,Cr], y [N,C], out [N,C,H,W]) in float64."""
    t, x, w1, b1, w2, b2 = (v.double() for v in (t, x, w1, b1, w2, b2))
    N, T = t.shape[0], w1.shape[0]
    k = torch.arange(N) % T
    s = t.mean((2, 3))
    a1 = torch.clamp(torch.einsum('njc,nc->nj', w1[k], s) + b1[k], min=0.0)
    y = torch.sigmoid(torch.einsum('ncj,nj->nc', w2[k], a1) + b2[k])
    return dict(s=s, a1=a1, y=y, out=t * y[:, :, None, None] + x)


def ca_backward(t, g, w1, w2, fwd):
    """-> dict(r, ds [N,C]; gt, gx [N,C,H,W]; gw1 [T,Cr,C], gb1 [T,Cr], gw2 [T,C,Cr], gb2 [T,C]) from ca_forward's dict."""
    t, g, w1, w2 = (v.double() for v in (t, g, w1, w2))
    N, T, hw = t.shape[0], w1.shape[0], t.shape[2] * t.shape[3]
    k = torch.arange(N) % T
    s, a1, y = fwd['s'], fwd['a1'], fwd['y']
    r = (g * t).sum((2, 3))
    dz2 = r * y * (1.0 - y)
    dz1 = torch.einsum('ncj,nc->nj', w2[k], dz2) * (a1 > 0).double()
    ds = torch.einsum('njc,nj->nc', w1[k], dz1) / hw
    per_task = lambda v: torch.zeros((T,) + v.shape[1:], dtype=torch.float64).index_add_(0, k, v)
    return dict(r=r, ds=ds, gt=g * y[:, :, None, None] + ds[:, :, None, None], gx=g,
                gw2=per_task(dz2[:, :, None] * a1[:, None, :]), gb2=per_task(dz2),
                gw1=per_task(dz1[:, :, None] * s[:, None, :]), gb1=per_task(dz1))


@functools.lru_cache(maxsize=None)
def ca_case(N, T, C, Cr, H, W):
    """(inputs, forward, backward) of one seeded case, computed once and shared (callers do not modify them)."""
    inp = ca_inputs(N, T, C, Cr, H, W)
    fwd = ca_forward(inp['t'], inp['x'], inp['w1'], inp['b1'], inp['w2'], inp['b2'])
    return inp, fwd, ca_backward(inp['t'], inp['g'], inp['w1'], inp['w2'], fwd)


# ---------------------------------------------------------------------------------------------
# update rules
# ---------------------------------------------------------------------------------------------
def mt_update(rule, w, g, lr, m, s, bc1, sqrt_bc2, beta1=BETA1, beta2=BETA2, eps=EPS):
    """One tensor of savfi_mt_update_f32 in float64.  lr: a scalar (LR_SCALAR) or an array like w (LR_ELEMENT); m / s: the moments
    before the step (ignored by the rules that do not use them).  -> (out, m', s', coef) with coef = d out / d lr per element;
    m' / s' are the inputs themselves where the rule leaves them alone."""
    w, g = np.asarray(w, np.float64), np.asarray(g, np.float64)
    lr = np.asarray(lr, np.float64)
    omb1, omb2 = 1.0 - beta1, 1.0 - beta2
    if rule == RULE_SGD:
        coef = -g
    elif rule == RULE_ADAM:
        m = beta1 * np.asarray(m, np.float64) + omb1 * g
        s = beta2 * np.asarray(s, np.float64) + omb2 * g * g
        coef = -(m / bc1) / (np.sqrt(s) / sqrt_bc2 + eps)
    elif rule == RULE_ADAMAX_LSLR:
        m = beta1 * np.asarray(m, np.float64) + omb1 * g
        coef = -(m / bc1) / (np.abs(g) + eps)
    elif rule == RULE_ADAMAX_MSGD:
        coef = -((omb1 * g) / bc1) / (np.abs(g) + eps)
    else:
        raise ValueError(rule)
    return w + lr * coef, m, s, coef


def mt_update_bwd(lr_mode, g_out, direction, scale):
    """savfi_mt_update_bwd_f32 for one tensor: scale * g_out * dir per element, or its sum (LR_SCALAR)."""
    v = scale * np.asarray(g_out, np.float64) * np.asarray(direction, np.float64)
    return v if lr_mode == LR_ELEMENT else v.sum()


def mt_mean(x):
    return np.asarray(x, np.float64).mean()


def mt_scale(gamma, w):
    return float(gamma) * np.asarray(w, np.float64)


def mt_scale_bwd(gamma, g_out, w):
    """-> (g_w = gamma * g_out, g_gamma = <g_out, w>)."""
    g_out, w = np.asarray(g_out, np.float64), np.asarray(w, np.float64)
    return float(gamma) * g_out, float((g_out * w).sum())


# The list of the multi-tensor tests: 110 tensors = 108 non-empty ones in three launch groups (48 + 48 + 12) and two empty ones,
# one inside the first group (caller's index 20) and one where the second group starts (index 49, after the 48th non-empty tensor).
MT_EMPTY = (20, 49)
MT_MISALIGNED = {6: 'w', 30: 'g', 70: 'out'}       # caller's index -> the ONE operand that starts a float past an aligned address
MT_LR_TABLE = (0.01, 0.02, 0.015, 0.03)            # LR_SCALAR: lr[i] = &table[i % 4]
MT_STEPS = 2


@functools.lru_cache(maxsize=None)
def mt_case():
    """Seeded fp32 inputs of the list: dict(sizes, steps [i] (step count of tensor i at the first update), w, lr (element-wise),
    m0, s0, go (a cotangent), g (one list per step)); gradients are randn with the magnitude floored at 1e-3."""
    gen = torch.Generator().manual_seed(20)
    sizes = [1, 3, 4, 5, 4095, 4096, 4097, 8191, 12288] + torch.randint(1, 5000, (99,), generator=gen).tolist()
    for i in MT_EMPTY:
        sizes.insert(i, 0)
    assert len(sizes) == 110 and all(sizes[i] == 0 for i in MT_EMPTY) and all(sizes[i] > 0 for i in MT_MISALIGNED)
    r = lambda n: torch.randn(n, generator=gen)

    def grad(n):
        v = r(n)
        return torch.where(v < 0, -1.0, 1.0) * v.abs().clamp_min(1e-3)
    return dict(sizes=sizes, steps=[1 + i % 5 for i in range(len(sizes))], w=[r(n) for n in sizes],
                lr=[0.01 * (1 + torch.rand(n, generator=gen)) for n in sizes], m0=[0.1 * r(n) for n in sizes],
                s0=[(0.1 * r(n)) ** 2 + 1e-6 for n in sizes], go=[r(n) for n in sizes],
                g=[[grad(n) for n in sizes] for _ in range(MT_STEPS)])


def mt_bias_corrections(step):
    """(bc1, sqrt_bc2) lists of the list's tensors at update `step` (0-based), in double like the caller computes them."""
    ks = [k + step for k in mt_case()['steps']]
    return [1 - BETA1 ** k for k in ks], [math.sqrt(1 - BETA2 ** k) for k in ks]


@functools.lru_cache(maxsize=None)
def mt_expected(rule, lr_mode):
    """Float64 results of MT_STEPS consecutive updates of the list (the moments carried from step to step, the weights the same
    each step): a list over steps of dict(out, m, s, coef), each a list of float64 arrays over the tensors."""
    c = mt_case()
    m, s = [v.double().numpy() for v in c['m0']], [v.double().numpy() for v in c['s0']]
    steps = []
    for step in range(MT_STEPS):
        bc1, sbc2 = mt_bias_corrections(step)
        res = dict(out=[], m=[], s=[], coef=[])
        for i in range(len(c['sizes'])):
            lr = np.float64(np.float32(MT_LR_TABLE[i % 4])) if lr_mode == LR_SCALAR else c['lr'][i].double().numpy()
            o, mi, si, co = mt_update(rule, c['w'][i].numpy(), c['g'][step][i].numpy(), lr, m[i], s[i], bc1[i], sbc2[i])
            for key, v in zip(('out', 'm', 's', 'coef'), (o, mi, si, co)):
                res[key].append(v)
        m, s = res['m'], res['s']
        steps.append(res)
    return steps


# What float32 arithmetic costs on this list: the float32 CPU oracle (oracle/rules.py, the reference's statements line by line) against
# mt_expected, largest |f32 - f64| / max(1, |f64|) over all tensors, both steps and both learning-rate modes, per rule and quantity,
# measured by tests/test_small_ops_ref_cpu.py::test_float32_oracle_error_sets_the_rule_tolerances (which fails when these figures go
# stale).  The kernel's operations come in another order (lr / bc1 first, a division where the oracle multiplies): 4 x the measured
# error.  0 = the float32 oracle is exact there (SGD's coef is -g), and so must the kernel be.
# Adamax as LSLR implements it divides the first moment by |g| + eps alone: where b1 m and (1 - b1) g cancel, the rounding of m is
# magnified by 1 / (bc1 |g|), up to 1e4 on this list, and the float32 oracle itself is 1.2e-6 * max(1, |want|) from float64 on `out`
# -- above the 1e-6 that the rule checks of the system tests hold on their three or four tensors.  Every other rule stays below it.
RULE_F32_ERR = {RULE_SGD: dict(out=6.1e-08, m=0.0, s=0.0, coef=0.0),
                RULE_ADAM: dict(out=2.5e-07, m=7.0e-08, s=2.6e-08, coef=3.8e-07),
                RULE_ADAMAX_LSLR: dict(out=1.16e-06, m=7.0e-08, s=0.0, coef=7.6e-06),
                RULE_ADAMAX_MSGD: dict(out=6.1e-08, m=0.0, s=0.0, coef=1.7e-07)}
RULE_TOL = {rule: {q: 4 * v for q, v in err.items()} for rule, err in RULE_F32_ERR.items()}


# ---------------------------------------------------------------------------------------------
# L1 / MSE
# ---------------------------------------------------------------------------------------------
def loss_rows(kind, a, b):
    """a, b [rows, n] -> float64 [rows]: mean |a - b| (kind 0) or mean (a - b)^2 (kind 1)."""
    d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    return (np.abs(d) if kind == 0 else d * d).mean(1)


def loss_rows_grad(kind, a, b, g_loss):
    """d (sum_r g_loss[r] * loss[r]) / d a: g_loss[r] * sign(a - b) / n with sign(0) = 0, or g_loss[r] * 2 (a - b) / n."""
    d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    gs = np.asarray(g_loss, np.float64)[:, None] / d.shape[1]
    return gs * np.sign(d) if kind == 0 else 2.0 * gs * d


def loss_inputs(rows, n, ties=False, seed=0):
    """Seeded fp32 a, b [rows, n] and g_loss [rows] (distinct per row); ties: every tenth element has a == b exactly."""
    gen = torch.Generator().manual_seed(rows * 31 + n % 9973 + seed)
    a, b = torch.rand(rows, n, generator=gen), torch.rand(rows, n, generator=gen)
    if ties:
        b.view(-1)[::10] = a.view(-1)[::10]
    return a, b, torch.randn(rows, generator=gen) + torch.arange(rows) * 0.25
