"""CPU: the float64 restatements of tests/small_ops_ref.py against autograd (channel attention, loss gradients) and against
oracle/rules.py evaluated in float64 (update rules), and the float32 oracle's own error on the list of the GPU test, which sets the
tolerances that test holds the kernels to."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import rules as orules
from tests import small_ops_ref as R

RULES = [R.RULE_SGD, R.RULE_ADAM, R.RULE_ADAMAX_LSLR, R.RULE_ADAMAX_MSGD]
MODES = [R.LR_SCALAR, R.LR_ELEMENT]


@pytest.mark.parametrize("N,T,C,Cr,H,W", [(4, 2, 12, 3, 3, 5), (3, 3, 16, 2, 1, 1), (6, 3, 5, 3, 2, 7), (2, 1, 1, 1, 1, 1), (4, 2, 40, 20, 4, 4)])
def test_channel_attention_restatement_matches_autograd(N, T, C, Cr, H, W):
    """The composition the reference uses (mean -> conv2d 1x1 -> relu -> conv2d 1x1 -> sigmoid -> scale -> + skip) through autograd
    in float64 gives the restatement's values, map gradients and per-task parameter gradients; the intermediates the C ABI exposes
    (r, ds) are tied to them by gt = g * y + ds and r = sum_hw g * t."""
    inp, fwd, bwd = R.ca_case(N, T, C, Cr, H, W)
    leaves = [inp[k].double().requires_grad_() for k in ('t', 'x', 'w1', 'b1', 'w2', 'b2')]
    t, x, w1, b1, w2, b2 = leaves
    outs, ys, hid = [], [], []
    for n in range(N):
        k = n % T
        s = t[n:n + 1].mean((2, 3), keepdim=True)
        h = F.relu(F.conv2d(s, w1[k].view(Cr, C, 1, 1), b1[k]))
        y = torch.sigmoid(F.conv2d(h, w2[k].view(C, Cr, 1, 1), b2[k]))
        hid.append(h.view(1, Cr)), ys.append(y.view(1, C)), outs.append(t[n:n + 1] * y + x[n:n + 1])
    out = torch.cat(outs, 0)
    grads = torch.autograd.grad(out, leaves, inp['g'].double())
    close = lambda a, b: float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))
    assert close(fwd['out'], out.detach()) and close(fwd['y'], torch.cat(ys, 0).detach()) and close(fwd['a1'], torch.cat(hid, 0).detach())
    assert close(fwd['s'], t.detach().mean((2, 3)))
    for key, want in zip(('gt', 'gx', 'gw1', 'gb1', 'gw2', 'gb2'), grads):
        assert close(bwd[key], want), key
    assert close(bwd['r'], (inp['g'].double() * t.detach()).sum((2, 3)))
    assert close(bwd['gt'], inp['g'].double() * fwd['y'][:, :, None, None] + bwd['ds'][:, :, None, None])
    assert any(float(v.abs().max()) > 0 for v in (bwd['gw1'], bwd['ds']))          # some hidden unit is active: the ReLU mask is exercised


@pytest.mark.parametrize("ties", [False, True])
@pytest.mark.parametrize("kind", [0, 1])
def test_loss_restatement_matches_autograd(kind, ties):
    a, b, gl = R.loss_inputs(3, 37, ties=ties)
    ad = a.double().requires_grad_()
    d = ad - b.double()
    rows = (d.abs() if kind == 0 else d * d).mean(1)
    want, = torch.autograd.grad((rows * gl.double()).sum(), ad)
    assert np.abs(R.loss_rows(kind, a.numpy(), b.numpy()) - rows.detach().numpy()).max() <= 1e-15
    got = R.loss_rows_grad(kind, a.numpy(), b.numpy(), gl.numpy())
    assert np.abs(got - want.numpy()).max() <= 1e-15
    if ties:
        assert (got.reshape(-1)[::10] == 0).all() and (a.view(-1)[::10] == b.view(-1)[::10]).all()     # sign(0) = 0, as torch has it


def _oracle_run(rule, lr_mode, dtype):
    """oracle/rules.py on the list of R.mt_case() in `dtype`: MT_STEPS updates with the moments carried in its state; -> per step
    dict(out, m, s, coef) of lists over the non-empty tensors' indices (None where the oracle has nothing: unused moments)."""
    c = R.mt_case()
    idx = [i for i, n in enumerate(c['sizes']) if n > 0]
    key = lambda i: 'p%d' % i
    st = orules.RuleState()
    for i in idx:                                # the state the kernels start from (Meta-SGD's Adamax never writes its zero moments)
        m0 = torch.zeros_like(c['m0'][i]) if rule == R.RULE_ADAMAX_MSGD else c['m0'][i]
        st.state[key(i)] = dict(step=c['steps'][i] - 1, exp_avg=m0.to(dtype).clone(), exp_avg_sq=c['s0'][i].to(dtype).clone(),
                                exp_inf=torch.zeros(c['sizes'][i], dtype=dtype))
    weights = {key(i): c['w'][i].to(dtype) for i in idx}
    steps = []
    for step in range(R.MT_STEPS):
        grads = {key(i): c['g'][step][i].to(dtype) for i in idx}
        if lr_mode == R.LR_SCALAR:
            lr = {key(i): torch.tensor(R.MT_LR_TABLE[i % 4], dtype=torch.float32).to(dtype).requires_grad_() for i in idx}
        else:
            lr = {key(i): c['lr'][i].to(dtype).clone().requires_grad_() for i in idx}
        # LSLR's Adamax indexes its table by the step, Meta-SGD's takes the entry as it is: hand each the view it expects
        if rule == R.RULE_SGD:
            out = orules.update_sgd(weights, grads, lr, 0, False)
        elif rule == R.RULE_ADAM:
            out = orules.update_adam(weights, grads, lr, 0, False, st)
        elif rule == R.RULE_ADAMAX_LSLR:
            out = orules.update_adamax_lslr(weights, grads, {k: v.unsqueeze(0) for k, v in lr.items()}, 0, st)
        else:
            out = orules.update_adamax_metasgd(weights, grads, lr, st)
        res = dict(out=[], m=[], s=[], coef=[])
        for i in idx:
            o = out[key(i)]
            g_lr, = torch.autograd.grad(o.sum(), lr[key(i)])
            res['out'].append(o.detach().double().numpy())
            res['coef'].append(g_lr.double().numpy())                    # element-wise lr: d sum(out) / d lr[e] = coef[e]; scalar: its sum
            res['m'].append(st.state[key(i)]['exp_avg'].double().numpy() if rule in (R.RULE_ADAM, R.RULE_ADAMAX_LSLR) else None)
            res['s'].append(st.state[key(i)]['exp_avg_sq'].double().numpy() if rule == R.RULE_ADAM else None)
        steps.append(res)
    return idx, steps


@pytest.mark.parametrize("lr_mode", MODES)
@pytest.mark.parametrize("rule", RULES)
def test_rule_restatement_matches_the_oracle_in_float64(rule, lr_mode):
    """oracle/rules.py restates the reference's update rules line by line; run in float64 on the list of the GPU test it gives what
    tests/small_ops_ref.py gives -- new weights, carried moments, and d out / d lr through autograd -- on every tensor, over two
    steps, with nothing excluded: every value of the restatement is finite."""
    idx, steps = _oracle_run(rule, lr_mode, torch.float64)
    want = R.mt_expected(rule, lr_mode)
    c = R.mt_case()
    for step in range(R.MT_STEPS):
        for j, i in enumerate(idx):
            for q in ('out', 'm', 's', 'coef'):
                ref, got = want[step][q][i], steps[step][q][j]
                assert np.isfinite(ref).all()
                if got is None:                                           # a moment the rule does not use stays what it was
                    src = c['m0'][i] if q == 'm' else c['s0'][i]
                    assert np.array_equal(ref, src.double().numpy()), (q, i)
                    continue
                if q == 'coef' and lr_mode == R.LR_SCALAR:
                    assert abs(got - ref.sum()) <= 1e-12 * max(1.0, np.abs(ref).sum()), (step, i)
                else:
                    assert np.abs(got - ref).max() <= 1e-13 * max(1.0, np.abs(ref).max()), (q, step, i)
    for i in R.MT_EMPTY:
        assert all(want[s][q][i].size == 0 for s in range(R.MT_STEPS) for q in ('out', 'coef'))


@pytest.mark.parametrize("rule", RULES)
def test_float32_oracle_error_sets_the_rule_tolerances(rule):
    """The float32 oracle against the float64 restatement on the same list: the largest |f32 - f64| / max(1, |f64|) per quantity is
    what R.RULE_F32_ERR records (not above it, and not below half of it: the recorded figure is a measurement, not a margin), and
    the GPU test allows 4 x that.  On `out` that stays under the 1e-6 * max(1, |want|) the rule checks of the system tests hold,
    except for LSLR's Adamax, whose float32 oracle is itself further than that from float64 (see tests/small_ops_ref.py)."""
    worst = dict(out=0.0, m=0.0, s=0.0, coef=0.0)
    for lr_mode in MODES:
        idx, steps = _oracle_run(rule, lr_mode, torch.float32)
        want = R.mt_expected(rule, lr_mode)
        for step in range(R.MT_STEPS):
            for j, i in enumerate(idx):
                for q in worst:
                    got, ref = steps[step][q][j], want[step][q][i]
                    if got is None or (q == 'coef' and lr_mode == R.LR_SCALAR):
                        continue
                    worst[q] = max(worst[q], float((np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max()))
    print("float32 oracle against float64, rule %d:" % rule, worst)
    for q, v in worst.items():
        assert 0.5 * R.RULE_F32_ERR[rule][q] <= v <= R.RULE_F32_ERR[rule][q], (q, v, R.RULE_F32_ERR[rule][q])
        assert R.RULE_TOL[rule][q] == 4 * R.RULE_F32_ERR[rule][q]
    assert (R.RULE_TOL[rule]['out'] <= 1e-6) == (rule != R.RULE_ADAMAX_LSLR)
    assert worst['out'] > 1e-6 or rule != R.RULE_ADAMAX_LSLR             # the one bound above 1e-6 is there because the oracle is


def test_small_reductions_and_lr_backward_restatements():
    g = np.random.default_rng(0)
    go, d, w = g.standard_normal(37), g.standard_normal(37), g.standard_normal(37)
    assert np.array_equal(R.mt_update_bwd(R.LR_ELEMENT, go, d, -1.0), -go * d)
    assert abs(R.mt_update_bwd(R.LR_SCALAR, go, d, 1.0) - float(np.dot(go, d))) <= 1e-13
    wt = torch.tensor(w, requires_grad=True)
    gam = torch.tensor(0.7, dtype=torch.float64, requires_grad=True)
    gw, gg = torch.autograd.grad(((gam * wt) * torch.tensor(go)).sum(), (wt, gam))
    rw, rg = R.mt_scale_bwd(0.7, go, w)
    assert np.abs(rw - gw.numpy()).max() <= 1e-15 and abs(rg - gg.item()) <= 1e-13
    assert np.array_equal(R.mt_scale(0.7, w), 0.7 * w) and abs(R.mt_mean(w) - w.sum() / 37) <= 1e-15
