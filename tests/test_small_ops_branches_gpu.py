"""GPU: the channel-attention kernels (csrc/chanattn.hip), the multi-tensor kernels (csrc/mt_update.hip) and the loss kernels
(csrc/loss.hip) along their own branch structure -- every kernel, both sides of every host-side route switch -- against the float64
restatements of tests/small_ops_ref.py, through the C ABI where hip_ops cannot reach a route."""
import ctypes
import math

import numpy as np
import pytest
import torch

from meta_interpolation_amd import _hip, hip_ops
from tests import small_ops_ref as R
from tests.helpers import CANARY, PAD, Guarded as _Guarded       # canary-padded device buffers (shared with test_upsample_forms_gpu.py)

pytestmark = pytest.mark.gpu

DEV = "cuda"
E_SHAPE, E_UNSUPPORTED = -2, -3


def _rel(a, b):
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-12)


# =============================================================================================
# channel attention
# =============================================================================================
CA_CASES = [  # N, T, C, Cr, H, W
    (4, 2, 192, 12, 12, 20),        # CAIN's own channel counts
    (3, 3, 16, 2, 5, 7),
    (2, 1, 256, 16, 3, 5),          # the last shape of the one-round kernels ...
    (2, 2, 257, 16, 2, 3),          # ... and the first generic ones on either axis
    (2, 2, 256, 17, 1, 1),
    (4, 2, 320, 20, 4, 6),          # generic kernels, several samples per task: the parameter gradients add up in global memory
    (4, 2, 1024, 64, 1, 3),         # the limits of the ABI: dz2[4], hid[64], dz1s[64], a1s[64] full
    (2, 1, 1, 1, 1, 1),
    (6, 3, 5, 3, 7, 9),
    (1, 1, 16, 4, 65, 67),          # hw = 4355 >= 4096, odd: ca_pool_kernel<1024>, two chunks per plane, misaligned chunk starts
]
CA_KEYS_FWD = ('s', 'a1', 'y', 'out')
CA_KEYS_BWD = ('r', 'gt', 'gw1', 'gb1', 'gw2', 'gb2')


def _small(C, Cr):
    return Cr <= 16 and C <= 256


def _inv_hw(hw):
    return float(np.float32(1.0) / np.float32(hw))        # what the fused launch computes itself: 1.f / (float)hw


def _ca_run(case, fused, w_override=None):
    """One forward and backward of `case` through the C ABI: the fused launches (MLP inside the apply) or pool + MLP + apply as
    separate launches (the one-round kernels at Cr <= 16 and C <= 256, the generic ones above).  -> {name: flat CPU tensor}.
    Every output lives between canaries; the parameter gradients start as NaN (they must be fully overwritten)."""
    N, T, C, Cr, H, W = case
    hw = H * W
    inp = dict(R.ca_case(*case)[0])
    if w_override:
        inp.update(w_override)
        Cr = inp['w1'].shape[1]
    d = {k: v.contiguous().to(DEV) for k, v in inp.items()}
    lib, st = _hip.lib(), _hip.current_stream()
    G = _Guarded()
    s, r, y, ds = (G.new(k, N, C) for k in ('s', 'r', 'y', 'ds'))
    a1 = G.new('a1', N, Cr)
    out, gt = G.new('out', N, C, H, W), G.new('gt', N, C, H, W)
    nan = float('nan')
    gw1, gb1 = G.new('gw1', T, Cr, C, fill=nan), G.new('gb1', T, Cr, fill=nan)
    gw2, gb2 = G.new('gw2', T, C, Cr, fill=nan), G.new('gb2', T, C, fill=nan)
    p = lambda v: v.data_ptr()
    t, x, g, w1, b1, w2, b2 = (d[k] for k in ('t', 'x', 'g', 'w1', 'b1', 'w2', 'b2'))
    _hip.check(lib.savfi_ca_pool_f32(p(t), None, p(s), N * C, hw, 1.0 / hw, st), "pool")
    if fused:
        _hip.check(lib.savfi_ca_apply_mlp_f32(p(t), p(s), p(w1), p(b1), p(w2), p(b2), p(x), p(out), p(y), p(a1), N, T, C, Cr, hw, st),
                   "apply_mlp")
    else:
        _hip.check(lib.savfi_ca_mlp_fwd_f32(p(s), p(w1), p(b1), p(w2), p(b2), p(y), p(a1), N, T, C, Cr, st), "mlp_fwd")
        _hip.check(lib.savfi_ca_apply_f32(p(t), p(y), p(x), None, p(out), N * C, hw, st), "apply")
    _hip.check(lib.savfi_ca_pool_f32(p(g), p(t), p(r), N * C, hw, 1.0, st), "pool (g * t)")
    if fused:
        _hip.check(lib.savfi_ca_apply_bwd_mlp_f32(p(g), p(r), p(s), p(y), p(a1), p(w1), p(w2), p(gt), p(gw1), p(gb1), p(gw2), p(gb2),
                                                  N, T, C, Cr, hw, st), "apply_bwd_mlp")
    else:
        _hip.check(lib.savfi_ca_mlp_bwd_f32(p(r), p(s), p(y), p(a1), p(w1), p(w2), p(ds), p(gw1), p(gb1), p(gw2), p(gb2),
                                            N, T, C, Cr, _inv_hw(hw), st), "mlp_bwd")
        _hip.check(lib.savfi_ca_apply_f32(p(g), p(y), None, p(ds), p(gt), N * C, hw, st), "apply (backward)")
    torch.cuda.synchronize()
    G.check("fused" if fused else "separate")
    if fused:
        assert G.untouched('ds')                          # the fused backward keeps ds to itself
    return {k: buf[PAD:PAD + n].cpu() for k, (buf, n) in G.bufs.items()}


def _ca_against_float64(case, got, what, with_ds):
    """2e-6 of the scale on the forward results, 2e-5 on every gradient and gradient intermediate."""
    inp, fwd, bwd = R.ca_case(*case)
    N, T, C, Cr, H, W = case
    k = torch.arange(N) % T
    # s is a mean of hw terms and a1 a sum of C products + b1: held to the scale of their terms (the largest mean |t| of a plane, the
    # largest sum |w1 s| + |b1| of a hidden unit) -- a unit's value can be a cancellation of them, or zero behind the ReLU
    s_scale = inp['t'].double().abs().mean((2, 3)).max().item()
    a1_scale = (torch.einsum('njc,nc->nj', inp['w1'].double()[k].abs(), fwd['s'].abs()) + inp['b1'].double()[k].abs()).max().item()
    figures = {}
    for key in CA_KEYS_FWD + CA_KEYS_BWD + (('ds',) if with_ds else ()):
        want = (fwd[key] if key in fwd else bwd[key]).reshape(-1)
        scale = {'s': s_scale, 'a1': a1_scale}.get(key, max(want.abs().max().item(), 1e-12))
        figures[key] = (got[key].double() - want).abs().max().item() / scale
    print(what, case, {k_: "%.2e" % v for k_, v in figures.items()})
    for key, v in figures.items():
        assert math.isfinite(v) and v < (2e-6 if key in CA_KEYS_FWD else 2e-5), (what, key, v)


@pytest.mark.parametrize("case", CA_CASES)
def test_channel_attention_routes_through_the_abi_match_float64(case):
    """Every route the C ABI offers for a shape -- the fused launches and the separate ones (one-round kernels) at Cr <= 16 and
    C <= 256, the separate ones (generic kernels) above -- against float64; nothing is written outside the outputs and the
    parameter gradients are fully overwritten (they start as NaN).  Where both routes run, the fused forward gives the separate
    launches' y, a1 and out bit for bit ("the same y bit for bit"), and the fused backward their four parameter gradients.  Its gt
    does NOT come out bit for bit, against what the source used to say ("the same ds bit for bit"): ca_mlp_bwd_small hands bare
    products to the wave sum, where the compiler fuses each into the first addition, and the fused launch's streaming workgroups
    hand over selected (rounded) ones.  Measured on the MI355X: 12418 of 184320 elements of gt differ at (4, 2, 192, 12), 1496 of 7680
    at (2, 1, 256, 16), by 1.2e-7 at most (one ulp), none at C <= 16 (one wave holds every channel: the fused addend is zero).  The
    comments are corrected; the pair is held to float64 (both, 2e-5) and to each other at the same 2e-5 of the scale."""
    N, T, C, Cr, H, W = case
    sep = _ca_run(case, fused=False)
    _ca_against_float64(case, sep, "separate/" + ("small" if _small(C, Cr) else "generic"), with_ds=True)
    if _small(C, Cr):
        fus = _ca_run(case, fused=True)
        _ca_against_float64(case, fus, "fused", with_ds=False)
        for key in ('s', 'r', 'y', 'a1', 'out', 'gw1', 'gb1', 'gw2', 'gb2'):
            assert torch.equal(fus[key], sep[key]), "fused and separate launches differ in " + key
        differ = int((fus['gt'] != sep['gt']).sum())
        print("fused against separate gt: %d of %d elements differ, by %.2e at most" % (differ, fus['gt'].numel(),
                                                                                       float((fus['gt'] - sep['gt']).abs().max())))
        assert _rel(fus['gt'].double(), sep['gt'].double()) < 2e-5


def test_channel_attention_one_round_block_sums_equal_the_generic_kernels():
    """ "the association of block_sum: bit-identical to the generic kernels".  The generic kernels cannot be launched at Cr <= 16
    and C <= 256, so the one-round case (C = 256, Cr = 16) gets a seventeenth hidden unit whose outgoing weights w2[:, 16] are
    zero: that sends the same numbers through the generic kernels.  Forward, the block sums are the hidden pre-activations: a1 must
    be the one-round kernel's bit for bit.  Backward they are da (gb1 is their masked sum over a task's samples), and there the
    claim does not hold on the MI355X: ca_mlp_bwd_small's products are fused into the first addition of its wave sums, the generic
    kernel's are rounded first.  The comment in the source says so now; gb1, like what follows the block sums (y, ds, the weight
    gradients), is held to float64."""
    case = (4, 2, 256, 16, 3, 5)
    N, T, C, Cr, H, W = case
    inp = R.ca_case(*case)[0]
    small = _ca_run(case, fused=False)
    g = torch.Generator().manual_seed(17)
    w1p = torch.cat([inp['w1'], torch.randn(T, 1, C, generator=g) / math.sqrt(C)], 1)
    b1p = torch.cat([inp['b1'], torch.full((T, 1), 0.05)], 1)                     # (positive bias: the extra unit is active for some samples)
    w2p = torch.cat([inp['w2'], torch.zeros(T, C, 1)], 2)
    gen = _ca_run(case, fused=False, w_override=dict(w1=w1p, b1=b1p, w2=w2p))
    a1g, gb1g = gen['a1'].view(N, 17), gen['gb1'].view(T, 17)
    assert torch.equal(a1g[:, :16].contiguous().view(-1), small['a1']), "forward block sums differ between the one-round and the generic kernel"
    print("one-round against generic: y equal", torch.equal(gen['y'], small['y']), " ds equal", torch.equal(gen['ds'], small['ds']),
          " gb1 equal", torch.equal(gb1g[:, :16].contiguous().view(-1), small['gb1']))
    assert _rel(gen['y'].double(), small['y'].double()) < 2e-6 and _rel(gen['ds'].double(), small['ds'].double()) < 2e-5
    assert _rel(gb1g[:, :16].contiguous().view(-1).double(), small['gb1'].double()) < 2e-5
    _ca_against_float64(case, {k: (v if k not in ('a1', 'gb1', 'gw1', 'gw2') else
                                   {'a1': a1g[:, :16], 'gb1': gb1g[:, :16], 'gw1': gen['gw1'].view(T, 17, C)[:, :16],
                                    'gw2': gen['gw2'].view(T, C, 17)[:, :, :16]}[k].contiguous().view(-1)) for k, v in gen.items()},
                        "generic with a silent 17th unit", with_ds=True)


def test_channel_attention_refusals_are_returned_before_any_launch():
    """Only return codes: the admission checks come before the launch, so the (valid, tiny) buffers are never touched."""
    lib, st = _hip.lib(), _hip.current_stream()
    z = torch.zeros(64, device=DEV)
    p = z.data_ptr()
    fwd = lambda N, T, C, Cr: lib.savfi_ca_mlp_fwd_f32(p, p, p, p, p, p, p, N, T, C, Cr, st)
    bwd = lambda N, T, C, Cr: lib.savfi_ca_mlp_bwd_f32(p, p, p, p, p, p, p, p, p, p, p, N, T, C, Cr, 1.0, st)
    ffwd = lambda N, T, C, Cr: lib.savfi_ca_apply_mlp_f32(p, p, p, p, p, p, p, p, p, p, N, T, C, Cr, 4, st)
    fbwd = lambda N, T, C, Cr: lib.savfi_ca_apply_bwd_mlp_f32(p, p, p, p, p, p, p, p, p, p, p, p, N, T, C, Cr, 4, st)
    for f in (fwd, bwd):
        assert f(2, 1, 1025, 16) == E_UNSUPPORTED and f(2, 1, 64, 65) == E_UNSUPPORTED
        assert f(3, 2, 64, 4) == E_SHAPE
    for f in (ffwd, fbwd):
        assert f(2, 1, 256, 17) == E_UNSUPPORTED and f(2, 1, 257, 16) == E_UNSUPPORTED
        assert f(3, 2, 64, 4) == E_SHAPE
    torch.cuda.synchronize()
    assert float(z.abs().sum()) == 0


@pytest.mark.parametrize("fuse", [True, False])
@pytest.mark.parametrize("case", CA_CASES)
def test_channel_attention_op_takes_both_routes(case, fuse, monkeypatch):
    """hip_ops.channel_attention_residual with CA_FUSE_MLP on and off: the launches it makes are the route's, and value, attention
    and all six gradients match float64."""
    N, T, C, Cr, H, W = case
    inp, fwd, bwd = R.ca_case(*case)
    monkeypatch.setattr(hip_ops, "CA_FUSE_MLP", fuse)
    names = []
    real = _hip.launch
    monkeypatch.setattr(_hip, "launch", lambda name, fn, **kw: (names.append(name), real(name, fn, **kw))[1])
    leaves = [inp[k].to(DEV).requires_grad_() for k in ('t', 'x')]
    for k, shape in (('w1', (T, Cr, C, 1, 1)), ('b1', (T, Cr)), ('w2', (T, C, Cr, 1, 1)), ('b2', (T, C))):
        leaves.append(inp[k].view(*shape).to(DEV).requires_grad_())
    args = leaves if T > 1 else leaves[:2] + [v[0] for v in leaves[2:]]
    out, y = hip_ops.channel_attention_residual(*args)
    grads = torch.autograd.grad(out, leaves, inp['g'].to(DEV))
    if fuse and _small(C, Cr):
        assert names == ["ca_pool", "ca_apply", "ca_pool", "ca_apply"]
    else:
        assert names == ["ca_pool", "ca_mlp", "ca_apply", "ca_pool", "ca_mlp_bwd", "ca_apply"]
    assert _rel(out.detach().cpu().double(), fwd['out']) < 2e-6
    assert _rel(y.detach().cpu().double().view(N, C), fwd['y']) < 2e-6
    for got, key in zip(grads, ('gt', 'gx', 'gw1', 'gb1', 'gw2', 'gb2')):
        assert _rel(got.cpu().double().reshape(-1), bwd[key].reshape(-1)) < 2e-5, key


# =============================================================================================
# multi-tensor kernels
# =============================================================================================
class _Arena:
    """The tensors of a list inside ONE buffer: each starts on a 256-byte boundary (+ shifts[i] floats), with at least PAD canary
    floats between neighbours and at both ends.  One copy back and one comparison then check the values of every tensor and every
    float the call does not own."""

    def __init__(self, sizes, shifts=None):
        self.sizes, self.off = list(sizes), []
        pos = PAD
        for i, n in enumerate(sizes):
            start = pos + (shifts or {}).get(i, 0)
            self.off.append(start)
            pos = (start + n + PAD + 63) // 64 * 64
        self.total = pos
        self.inside = np.zeros(self.total, bool)
        for o, n in zip(self.off, sizes):
            self.inside[o:o + n] = True

    def host(self, values=None, dtype=np.float32):
        a = np.full(self.total, CANARY, dtype)
        if values is not None:
            for o, n, v in zip(self.off, self.sizes, values):
                if v is not None:
                    a[o:o + n] = np.asarray(v)
        return a

    def device(self, values=None):
        return torch.from_numpy(self.host(values)).to(DEV)

    def ptrs(self, buf, skip=()):
        """Host array of the tensors' device addresses inside `buf`; NULL for the empty ones and for the indices in `skip`."""
        arr = (ctypes.c_void_p * len(self.sizes))()
        for i, (o, n) in enumerate(zip(self.off, self.sizes)):
            arr[i] = None if (n == 0 or i in skip) else buf.data_ptr() + 4 * o
        return arr

    def compare(self, buf, want, tol, what):
        """|got - want| <= tol * max(1, |want|) on every element of every tensor (tol = 0: equal), canaries untouched."""
        got = buf.cpu().numpy().astype(np.float64)
        ref = self.host(want, np.float64)
        assert (got[~self.inside] == CANARY).all(), what + ": written outside the tensors"
        err = (np.abs(got - ref) / np.maximum(1.0, np.abs(ref)))[self.inside]
        worst = float(err.max()) if err.size else 0.0
        print("%s: worst %.3e (allowed %.3e)" % (what, worst, tol))
        assert np.isfinite(got[self.inside]).all() and worst <= tol, (what, worst, tol)


def _np(ts):
    return [t.numpy() for t in ts]


def _shift_of(operand):
    return {i: 1 for i, op in R.MT_MISALIGNED.items() if op == operand}


_MT = {}


def _mt_device():
    """The list's inputs on the device, once: arenas (w, g and out each with ONE tensor a float past an aligned address) and buffers."""
    if not _MT:
        c = R.mt_case()
        sizes = c['sizes']
        _MT.update(plain=_Arena(sizes), aw=_Arena(sizes, _shift_of('w')), ag=_Arena(sizes, _shift_of('g')), aout=_Arena(sizes, _shift_of('out')))
        _MT.update(w=_MT['aw'].device(_np(c['w'])), g=[_MT['ag'].device(_np(gs)) for gs in c['g']], lr=_MT['plain'].device(_np(c['lr'])),
                   go=_MT['plain'].device(_np(c['go'])), table=torch.tensor(R.MT_LR_TABLE, dtype=torch.float32, device=DEV))
    return _MT


RULES = [R.RULE_SGD, R.RULE_ADAM, R.RULE_ADAMAX_LSLR, R.RULE_ADAMAX_MSGD]
MODES = [R.LR_SCALAR, R.LR_ELEMENT]


@pytest.mark.parametrize("want_coef", [False, True])
@pytest.mark.parametrize("lr_mode", MODES)
@pytest.mark.parametrize("rule", RULES)
def test_mt_update_rules_over_three_launch_groups_match_float64(rule, lr_mode, want_coef):
    """savfi_mt_update_f32 on 110 tensors (three launch groups; an empty tensor inside the first group and one where the second
    starts; sizes around the 4096-element chunk; w, g and out each misaligned for one tensor, which takes that tensor alone down the
    scalar route; LR_SCALAR's lr[i] = &table[i % 4], LSLR's own 4-byte-aligned pointers), with bc1 / sqrt_bc2 of a different step
    count per tensor, two consecutive steps with the moments carried in place.

    Tolerances: R.RULE_TOL = 4 x what the float32 CPU oracle is away from float64 on these very inputs, per rule and quantity, as
    |err| / max(1, |want|) (measured on the CPU: tests/test_small_ops_ref_cpu.py):
        SGD          out 6.1e-8 -> 2.4e-7   coef exact (-g)
        Adam         out 2.5e-7 -> 1.0e-6   m 7.0e-8 -> 2.8e-7   s 2.6e-8 -> 1.0e-7   coef 3.8e-7 -> 1.5e-6
        Adamax/LSLR  out 1.16e-6 -> 4.6e-6  m 7.0e-8 -> 2.8e-7   coef 7.6e-6 -> 3.0e-5
        Adamax/MSGD  out 6.1e-8 -> 2.4e-7   coef 1.7e-7 -> 6.8e-7
    Only LSLR's Adamax is above the 1e-6 * max(1, |want|) of the system tests' rule checks: the float32 oracle itself is (m / (|g| +
    eps) magnifies the rounding of a cancelled first moment by up to 1e4 on this list).  Moments a rule does not use must come back
    untouched (tolerance 0), and so must every float between the tensors."""
    c, D = R.mt_case(), _mt_device()
    n = len(c['sizes'])
    lib, st = _hip.lib(), _hip.current_stream()
    plain, aw, ag, aout = D['plain'], D['aw'], D['ag'], D['aout']
    m, s = plain.device(_np(c['m0'])), plain.device(_np(c['s0']))
    if lr_mode == R.LR_SCALAR:
        lr_ptrs = (ctypes.c_void_p * n)(*[D['table'].data_ptr() + 4 * (i % 4) for i in range(n)])
    else:
        lr_ptrs = plain.ptrs(D['lr'])
    want, tol = R.mt_expected(rule, lr_mode), R.RULE_TOL[rule]
    for step in range(R.MT_STEPS):
        out = aout.device()
        coef = plain.device() if want_coef else None
        bc1, sbc2 = R.mt_bias_corrections(step)
        rc = lib.savfi_mt_update_f32(rule, lr_mode, n, aw.ptrs(D['w']), ag.ptrs(D['g'][step]), lr_ptrs, plain.ptrs(m), plain.ptrs(s),
                                     aout.ptrs(out), plain.ptrs(coef) if want_coef else None, _hip.i64_array(c['sizes']),
                                     _hip.f32_array(bc1), _hip.f32_array(sbc2), R.BETA1, R.BETA2, R.EPS, st)
        assert rc == 0
        torch.cuda.synchronize()
        tag = "rule %d lr_mode %d step %d " % (rule, lr_mode, step)
        aout.compare(out, want[step]['out'], tol['out'], tag + "out")
        plain.compare(m, want[step]['m'], tol['m'], tag + "m")
        plain.compare(s, want[step]['s'], tol['s'], tag + "s")
        if want_coef:
            plain.compare(coef, want[step]['coef'], tol['coef'], tag + "coef")
    assert torch.equal(D['w'], aw.device(_np(c['w']))) and torch.equal(D['g'][1], ag.device(_np(c['g'][1])))     # inputs are inputs


def _sum_close(got, ref, abs_sum):
    """A float32 sum of products against float64, relative to the sum of magnitudes (the measure of the bias sums of
    test_bias_act_kernels_on_odd_planes)."""
    return abs(got - ref) <= 1e-5 * abs_sum + 1e-6


@pytest.mark.parametrize("lr_mode", MODES)
def test_mt_update_backward_over_three_launch_groups(lr_mode):
    """savfi_mt_update_bwd_f32 on the same list with dir = g and scale = -1 (SGD's form).  ELEMENT: -(g_out * g) is one float32
    product, so the result is the rounded float64 product exactly, and nothing lands between the tensors.  SCALAR: the
    destinations are the 110 elements of one zero-filled buffer as _MtUpdate.backward makes them, attached again slot by slot after
    the host skipped the empties; each is an atomic sum over chunks, and the empties' destinations stay zero."""
    c, D = R.mt_case(), _mt_device()
    sizes = c['sizes']
    n = len(sizes)
    lib, st = _hip.lib(), _hip.current_stream()
    plain, ag, aout = D['plain'], D['ag'], D['aout']
    if lr_mode == R.LR_ELEMENT:
        dst = aout.device()
        dst_ptrs = aout.ptrs(dst)
    else:
        guard = torch.full((n + 2 * PAD,), CANARY, device=DEV)
        dst = guard[PAD:PAD + n].zero_()
        dst_ptrs = (ctypes.c_void_p * n)(*[dst.data_ptr() + 4 * i for i in range(n)])
    rc = lib.savfi_mt_update_bwd_f32(lr_mode, n, plain.ptrs(D['go']), ag.ptrs(D['g'][0]), dst_ptrs, _hip.i64_array(sizes), -1.0, st)
    assert rc == 0
    torch.cuda.synchronize()
    prods = [c['go'][i].double().numpy() * c['g'][0][i].double().numpy() for i in range(n)]
    if lr_mode == R.LR_ELEMENT:
        want = [R.mt_update_bwd(lr_mode, c['go'][i].numpy(), c['g'][0][i].numpy(), -1.0).astype(np.float32) for i in range(n)]
        aout.compare(dst, want, 0.0, "g_lr (element)")
    else:
        got = dst.cpu().double().numpy()
        assert bool((guard[:PAD] == CANARY).all()) and bool((guard[PAD + n:] == CANARY).all())
        for i in range(n):
            if sizes[i] == 0:
                assert got[i] == 0.0, i
            else:
                ref = R.mt_update_bwd(lr_mode, c['go'][i].numpy(), c['g'][0][i].numpy(), -1.0)
                assert _sum_close(got[i], ref, np.abs(prods[i]).sum()), (i, sizes[i], got[i], ref)


def test_mt_mean_scale_and_scale_backward_over_three_launch_groups():
    """savfi_mt_mean_f32, savfi_mt_scale_f32 and savfi_mt_scale_bwd_f32 on the 108 non-empty tensors of the list (48 + 48 + 12: the
    per-tensor vectors are handed to the later groups at an offset), w and out / g_w misaligned for one tensor each; with the two
    empty tensors in the list all three refuse with SAVFI_E_SHAPE.  gamma * x is one float32 product: the rounded float64
    product exactly; the means and <g_out, w> are atomic sums over chunks: relative to the sum of magnitudes."""
    c, D = R.mt_case(), _mt_device()
    lib, st = _hip.lib(), _hip.current_stream()
    full_n = len(c['sizes'])
    z = torch.zeros(full_n, device=DEV)
    pw, po, sizes_full = D['aw'].ptrs(D['w']), D['plain'].ptrs(D['go']), _hip.i64_array(c['sizes'])
    for i in R.MT_EMPTY:                                   # (an empty tensor with a non-NULL address is refused for its size)
        pw[i] = po[i] = z.data_ptr()
    assert lib.savfi_mt_mean_f32(full_n, pw, sizes_full, z.data_ptr(), st) == E_SHAPE
    assert lib.savfi_mt_scale_f32(full_n, pw, z.data_ptr(), po, sizes_full, st) == E_SHAPE
    assert lib.savfi_mt_scale_bwd_f32(full_n, po, pw, z.data_ptr(), None, z.data_ptr(), sizes_full, st) == E_SHAPE
    torch.cuda.synchronize()
    assert float(z.abs().sum()) == 0

    live = [i for i, k in enumerate(c['sizes']) if k > 0]
    sizes = [c['sizes'][i] for i in live]
    n = len(sizes)
    w, go = [c['w'][i].numpy() for i in live], [c['go'][i].numpy() for i in live]
    a_in, a_w, a_out = _Arena(sizes), _Arena(sizes, {5: 1}), _Arena(sizes, {60: 1})
    dw, dgo = a_w.device(w), a_in.device(go)
    nums = _hip.i64_array(sizes)
    gamma = torch.randn(n, generator=torch.Generator().manual_seed(4))
    dgamma = gamma.to(DEV)

    def vec():
        guard = torch.full((n + 2 * PAD,), CANARY, device=DEV)
        return guard, guard[PAD:PAD + n].zero_()

    def vec_ok(guard):
        return bool((guard[:PAD] == CANARY).all()) and bool((guard[PAD + n:] == CANARY).all())

    # mean
    guard, mean = vec()
    assert lib.savfi_mt_mean_f32(n, a_w.ptrs(dw), nums, mean.data_ptr(), st) == 0
    got = mean.cpu().double().numpy()
    assert vec_ok(guard)
    for i in range(n):
        assert _sum_close(got[i] * sizes[i], R.mt_mean(w[i]) * sizes[i], np.abs(w[i]).sum()), (i, sizes[i])
    # scale
    out = a_out.device()
    assert lib.savfi_mt_scale_f32(n, a_w.ptrs(dw), dgamma.data_ptr(), a_out.ptrs(out), nums, st) == 0
    a_out.compare(out, [R.mt_scale(gamma[i].item(), w[i]).astype(np.float32) for i in range(n)], 0.0, "mt_scale")
    # scale backward: every g_w and g_gamma; g_w absent; some g_w absent; g_gamma absent
    ref = [R.mt_scale_bwd(gamma[i].item(), go[i], w[i]) for i in range(n)]
    ref_gw = [r[0].astype(np.float32) for r in ref]
    holes = set(range(0, n, 3))

    def gamma_ok(gg):
        got = gg.cpu().double().numpy()
        for i in range(n):
            assert _sum_close(got[i], ref[i][1], np.abs(go[i].astype(np.float64) * w[i]).sum()), (i, sizes[i], got[i], ref[i][1])

    for what, skip, want_gamma in (("all", None, True), ("no g_w", "all", True), ("holes in g_w", holes, True), ("no g_gamma", None, False)):
        gw = a_out.device()
        guard, gg = vec()
        p_gw = None if skip == "all" else a_out.ptrs(gw, skip or ())
        rc = lib.savfi_mt_scale_bwd_f32(n, a_in.ptrs(dgo), a_w.ptrs(dw), dgamma.data_ptr(), p_gw, gg.data_ptr() if want_gamma else None,
                                        nums, st)
        assert rc == 0, what
        torch.cuda.synchronize()
        assert vec_ok(guard)
        if want_gamma:
            gamma_ok(gg)
        else:
            assert float(gg.abs().sum()) == 0
        if skip == "all":
            assert bool((gw == CANARY).all())
        else:          # (a tensor without a g_w keeps its canaries: its slot of the expected arena is left as it is)
            a_out_want = [None if (skip and i in skip) else ref_gw[i] for i in range(n)]
            got = gw.cpu().numpy()
            exp = a_out.host(a_out_want)
            assert np.array_equal(got, exp), what


def _dense(t):
    return t.detach().cpu().double().contiguous()


@pytest.mark.parametrize("lr_mode", MODES)
def test_mt_update_op_reads_strided_gradients_and_learning_rates_by_value(lr_mode):
    """hip_ops.mt_update hands data_ptr()s to the kernel, which reads them as dense arrays: a transposed gradient, an expanded one
    (stride 0) and a transposed element-wise learning-rate table are made dense on the way in.  SGD with learnable learning rates,
    so the backward multiplies by the saved gradients (ctx.dirs): value and learning-rate gradient against float64 on the dense
    values.  LR_SCALAR takes its learning rates as LSLR does, table[num_step]: 0-dim views at 4-byte offsets."""
    g = torch.Generator().manual_seed(12)
    ws = [torch.randn(6, 7, generator=g).to(DEV), torch.randn(5, 4, generator=g).to(DEV), torch.randn(9, generator=g).to(DEV)]
    gs = [torch.randn(7, 6, generator=g).to(DEV).t(), torch.randn(5, 1, generator=g).to(DEV).expand(5, 4), torch.randn(9, generator=g).to(DEV)]
    assert not gs[0].is_contiguous() and not gs[1].is_contiguous()
    if lr_mode == R.LR_ELEMENT:
        bases = [(0.01 + 0.02 * torch.rand(7, 6, generator=g)).to(DEV).requires_grad_(), (0.01 + 0.02 * torch.rand(5, 4, generator=g)).to(DEV).requires_grad_(),
                 (0.01 + 0.02 * torch.rand(9, generator=g)).to(DEV).requires_grad_()]
        lrs = [bases[0].t(), bases[1], bases[2]]
        assert not lrs[0].is_contiguous()
    else:
        bases = [(0.01 + 0.02 * torch.rand(4, generator=g)).to(DEV).requires_grad_() for _ in ws]
        lrs = [b[k + 1] for k, b in enumerate(bases)]
    outs = hip_ops.mt_update(_hip.RULE_SGD, lr_mode, ws, gs, lrs)
    cots = [torch.randn(w.shape, generator=g).to(DEV) for w in ws]
    g_lr = torch.autograd.grad(outs, bases, cots)
    for k in range(3):
        w64, g64, lr64, co64 = _dense(ws[k]), _dense(gs[k]), _dense(lrs[k]), _dense(cots[k])
        want = w64 - lr64 * g64
        err = ((_dense(outs[k]) - want).abs() / want.abs().clamp_min(1.0)).max().item()
        assert err <= R.RULE_TOL[R.RULE_SGD]['out'], (k, err)
        prod = -(co64 * g64)
        if lr_mode == R.LR_ELEMENT:
            want_lr = prod.t() if k == 0 else prod
            assert torch.equal(g_lr[k].cpu(), want_lr.float()), k                 # one float32 product: the rounded float64 product
        else:
            got = g_lr[k].cpu().double()
            assert _sum_close(got[k + 1].item(), prod.sum().item(), prod.abs().sum().item()), k
            assert float(got.abs().sum() - got[k + 1].abs()) == 0                # the other steps' learning rates get no gradient


def test_mt_update_op_refuses_strided_moments():
    """m and s are updated in place: a dense copy would lose the update, so a non-contiguous moment is refused, and named."""
    g = torch.Generator().manual_seed(13)
    w, gr = torch.randn(6, 7, generator=g).to(DEV), torch.randn(6, 7, generator=g).to(DEV)
    lr = torch.tensor(0.01, device=DEV)
    dense, strided = torch.zeros(6, 7, device=DEV), torch.zeros(7, 6, device=DEV).t()
    kw = dict(bc1=[0.1], sqrt_bc2=[0.1])
    for m, s, name in ((strided, dense, "m"), (dense, strided, "s")):
        with pytest.raises(ValueError, match="`%s`" % name):
            hip_ops.mt_update(_hip.RULE_ADAM, _hip.LR_SCALAR, [w], [gr], [lr], m=[m], s=[s], **kw)
    assert float(dense.abs().sum()) == 0 and float(strided.abs().sum()) == 0     # refused before the launch
    # ... and a strided gradient next to dense moments goes through, moments updated in place
    out, = hip_ops.mt_update(_hip.RULE_ADAM, _hip.LR_SCALAR, [w], [gr.t().contiguous().t()], [lr], m=[dense], s=[torch.zeros(6, 7, device=DEV)], **kw)
    m64 = (1.0 - R.BETA1) * _dense(gr)
    assert ((_dense(dense) - m64).abs() / m64.abs().clamp_min(1.0)).max().item() <= R.RULE_TOL[R.RULE_ADAM]['m']
    want = R.mt_update(R.RULE_ADAM, w.cpu().numpy(), gr.cpu().numpy(), np.float64(np.float32(0.01)), np.zeros((6, 7)), np.zeros((6, 7)), 0.1, 0.1)[0]
    assert (np.abs(out.cpu().double().numpy() - want) / np.maximum(1.0, np.abs(want))).max() <= R.RULE_TOL[R.RULE_ADAM]['out']


# =============================================================================================
# L1 / MSE
# =============================================================================================
LOSS_CASES = [(1, 1), (1, 4095), (1, 4097), (3, 4096), (3, 4099), (5, 7), (2, 12289), (3, 65 * 4096 + 5),
              (2, 65 * 4096 + 4)]         # (the last one: more than 64 partial sums per row on the vector route too)
LOSS_SHIFTS = [(0, 0), (1, 0), (0, 3), (2, 2)]              # floats past an aligned address: a, b


def _shifted(t, shift):
    buf = torch.empty(t.numel() + 8, device=DEV)
    view = buf[shift:shift + t.numel()]
    view.copy_(t.reshape(-1).to(DEV))
    return view


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("rows,n", LOSS_CASES)
def test_l1_mse_rows_through_the_abi_match_float64(rows, n, kind):
    """savfi_l1_mse_f32 / savfi_l1_mse_bwd_f32 on both sides of `aligned && (rows == 1 || n % 4 == 0)`: rows of 1 .. 65 * 4096 + 5
    elements (more than 64 partial sums per row: loss_finish's strided loop; rows that end one element before, on and after the
    4096-element block), aligned operands and a, b or both off by one to three floats.  Values: 1e-6 * max(1, |ref|) + 1e-7 and
    bit-equal when run twice, with exactly savfi_l1_mse_scratch_floats(rows, n) floats of scratch between canaries.  Gradients:
    one rounding each, 1e-6 relative per element, with a distinct g_loss per row; every tenth element has a == b, where L1's
    gradient is exactly 0 (sign(0) = 0 as in torch) and MSE's a zero of either sign."""
    lib, st = _hip.lib(), _hip.current_stream()
    a, b, gl = R.loss_inputs(rows, n, ties=True)
    want = R.loss_rows(kind, a.numpy(), b.numpy())
    want_g = R.loss_rows_grad(kind, a.numpy(), b.numpy(), gl.numpy()).reshape(-1)
    tie = (a == b).reshape(-1).numpy()
    assert tie[::10].all()
    ns = int(lib.savfi_l1_mse_scratch_floats(rows, n))
    assert ns == rows * ((n + 4095) // 4096)
    dgl = gl.to(DEV)
    for sa, sb in LOSS_SHIFTS:
        av, bv = _shifted(a, sa), _shifted(b, sb)
        runs = []
        for _ in range(2):
            G = _Guarded()
            res, scratch, ga = G.new('result', rows), G.new('scratch', ns), G.new('g_a', rows * n)
            assert lib.savfi_l1_mse_f32(kind, av.data_ptr(), bv.data_ptr(), res.data_ptr(), scratch.data_ptr(), rows, n, st) == 0
            assert lib.savfi_l1_mse_bwd_f32(kind, av.data_ptr(), bv.data_ptr(), dgl.data_ptr(), ga.data_ptr(), rows, n, st) == 0
            torch.cuda.synchronize()
            G.check("l1_mse shifts %d %d" % (sa, sb))
            runs.append((res.cpu(), ga.cpu()))
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
        got, got_g = runs[0][0].double().numpy(), runs[0][1].double().numpy()
        assert (np.abs(got - want) <= 1e-6 * np.maximum(1.0, np.abs(want)) + 1e-7).all(), (sa, sb, got, want)
        assert (np.abs(got_g - want_g) <= 1e-6 * np.abs(want_g)).all(), (sa, sb)
        assert (got_g[tie] == 0).all()
        assert torch.equal(av.cpu(), a.reshape(-1)) and torch.equal(bv.cpu(), b.reshape(-1))
    # the same rows through the op
    ad = a.to(DEV).requires_grad_()
    fn = hip_ops.l1_loss_per_sample if kind == 0 else hip_ops.mse_loss_per_sample
    loss = fn(ad, b.to(DEV))
    g_op, = torch.autograd.grad((loss * dgl).sum(), ad)
    got = loss.detach().cpu().double().numpy()
    assert got.shape == (rows,) and (np.abs(got - want) <= 1e-6 * np.maximum(1.0, np.abs(want)) + 1e-7).all()
    got_g = g_op.cpu().double().numpy().reshape(-1)
    assert (np.abs(got_g - want_g) <= 1e-6 * np.abs(want_g)).all() and (got_g[tie] == 0).all()


def test_l1_mse_refusals():
    lib, st = _hip.lib(), _hip.current_stream()
    z = torch.zeros(64, device=DEV)
    p = z.data_ptr()
    for rows, n, kind, code in ((0, 8, 0, E_SHAPE), (2, 0, 1, E_SHAPE), (2, 8, 2, E_UNSUPPORTED)):
        assert lib.savfi_l1_mse_f32(kind, p, p, p, p, rows, n, st) == code
        assert lib.savfi_l1_mse_bwd_f32(kind, p, p, p, p, rows, n, st) == code
    assert lib.savfi_l1_mse_scratch_floats(0, 8) == E_SHAPE and lib.savfi_l1_mse_scratch_floats(2, 0) == E_SHAPE
    torch.cuda.synchronize()
    assert float(z.abs().sum()) == 0
