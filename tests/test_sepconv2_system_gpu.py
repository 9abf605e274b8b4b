"""-m gpu: --model sepconv --second_order with --sepconv_second_order 1 / 0 against the CPU oracle's recorded second-order run
(tests/golden/system_sepconv_second_order_2step.npz, tools/gen_sepconv2_golden.py): `full64` through a twice-differentiable 51-tap op,
`drop64` through a once-differentiable one (the reference's behaviour), `full32` for the oracle's own fp32 spread."""
import functools

import pytest
import torch

from meta_interpolation_amd import hip_ops, model_utils, synthetic
from tests import sepconv2_ref as R
from tests.helpers import assert_fp_close, build_system, golden, observe, parse_case_args

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _run(flag):
    """loss and {name: fingerprint} of the outer gradients of one meta-iteration of the fixture's configuration"""
    fx = golden(R.FIXTURE)
    system = build_system('sepconv', dict(parse_case_args(fx), sepconv_second_order=flag))
    assert system.net.sepconv_second_order == bool(flag)
    rec = observe(system)
    frames = synthetic.septuplet_batch(int(fx['B']), int(fx['H']), int(fx['W']), model='sepconv')
    flags = (hip_ops.double_backward(), model_utils.fuse_conv_act())       # the pass switches are per thread and outlive the pass:
    try:                                                                   # hand the later suites the thread as it was
        losses, _, _ = system.run_train_iter(data_batch=frames, epoch=0, do_evaluation=False)
        torch.cuda.synchronize()
    finally:
        hip_ops.set_double_backward(flags[0])
        model_utils.set_fuse_conv_act(flags[1])
    return losses['loss'].item(), rec['outer_grad_fp']


def _compare(flag, key):
    """(tensors checked, worst distance / gate) of the run with `flag` against the fixture's run `key`"""
    fx = golden(R.FIXTURE)
    loss, got = _run(flag)
    want_loss = float(fx[key + '_loss'])
    assert abs(loss - want_loss) <= R.LOSS_RTOL * abs(want_loss), (loss, want_loss)
    checked, worst = 0, 0.0
    for i, n in enumerate(str(s) for s in fx['names']):
        ratio = R.fp_dist(got['net.' + n], fx[key + '_fp'][i]) / R.fp_gate(fx['full64_fp'][i], fx['full32_fp'][i])
        worst = max(worst, ratio)
        checked += 1
    return checked, worst, got


def test_flag_1_matches_the_full_second_order_run():
    fx = golden(R.FIXTURE)
    checked, worst, got = _compare(1, 'full64')
    print("flag 1 vs full64: worst distance / gate %.3f over %d tensors" % (worst, checked))
    for i, n in enumerate(str(s) for s in fx['names']):
        f64, f32 = fx['full64_fp'][i], fx['full32_fp'][i]
        # max(2e-3 of the abs-sum, 3 x the oracle's own fp32-vs-fp64 spread): the contract through rtol, the rest as an allowance
        assert_fp_close(got['net.' + n], f64, R.FP_RTOL, ('second-order sepconv', n), extra_abs=max(0.0, R.fp_gate(f64, f32) - R.fp_contract(f64)))
    assert checked == R.N_TENSORS == 94


def test_flag_0_is_unchanged_and_the_test_can_tell():
    fx = golden(R.FIXTURE)
    checked, worst, got = _compare(0, 'drop64')
    print("flag 0 vs drop64: worst distance / gate %.3f over %d tensors" % (worst, checked))
    for i, n in enumerate(str(s) for s in fx['names']):
        f64, f32, d64 = fx['full64_fp'][i], fx['full32_fp'][i], fx['drop64_fp'][i]
        assert_fp_close(got['net.' + n], d64, R.FP_RTOL, ('first-order terms only', n), extra_abs=max(0.0, R.fp_gate(f64, f32) - R.fp_contract(f64)))
    assert checked == 94
    # ... and against the full run it fails by more than 10 x the gate (the two losses agree: the forward is the same)
    far = [n for i, n in enumerate(str(s) for s in fx['names'])
           if R.fp_dist(got['net.' + n], fx['full64_fp'][i]) > 10 * R.fp_gate(fx['full64_fp'][i], fx['full32_fp'][i])]
    print("flag 0 vs full64: %d of %d tensors further than 10 x the gate" % (len(far), checked))
    assert len(far) >= 1
