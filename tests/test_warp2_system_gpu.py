"""-m gpu: --second_order --warp_second_order 1 through the whole meta-iteration, against the oracle's second-order run on the CPU.

Modelled on test_second_order_voxelflow_matches_oracle (tests/test_system_gpu.py): 1 task, 64 x 64, SGD, 1*MSE, 2 inner steps; the
loss to 5e-5 relative and the outer-gradient fingerprints to 2e-3 of their abs-sum.  The weights are those of tests/warp2_system.py --
VoxelFlow's 'smooth' recipe; RRIN's and Super SloMo's seeded weights with the flow heads' last convolutions scaled, the same state on
both sides -- for which tests/test_warp2_ref_cpu.py shows the oracle's float32 and float64 runs inside a quarter of this gate.  The
product's six runs share one child process (tests/warp2_system.py says why)."""
import pytest

from tests import warp2_system as S
from tests.helpers import assert_fp_close

pytestmark = pytest.mark.gpu


def _device_run(model, flag):
    """(loss, outer-gradient fingerprints) of the product's meta-iteration with --warp_second_order `flag`; raises what the run raised"""
    got = S.device_runs()[(model, flag)]
    if isinstance(got, str):
        raise RuntimeError(got)
    return got


def _hold(got, want_loss, want_fp, prefix, what):
    loss, fps = got
    assert abs(loss - want_loss) <= S.LOSS_GATE * abs(want_loss), (what, loss, want_loss)
    checked = 0
    for name, want in want_fp.items():
        if prefix + name in fps:
            assert_fp_close(fps[prefix + name], want, S.FP_GATE, (what, name))
            checked += 1
    return checked


def test_second_order_voxelflow_on_the_fused_warp_matches_the_oracle_and_the_composed_path():
    loss, fps = S.oracle_run('voxelflow')
    fused, composed = _device_run('voxelflow', 1), _device_run('voxelflow', 0)
    assert _hold(fused, loss, fps, 'net.', 'fused against the oracle') >= 20
    assert _hold(composed, loss, fps, 'net.', 'composed against the oracle') >= 20
    assert _hold(fused, composed[0], composed[1], '', 'fused against composed') >= 20


@pytest.mark.parametrize("model,n_grads", [("rrin", 160), ("superslomo", 90)])
def test_second_order_through_the_flow_warp_matches_the_oracle(model, n_grads):
    """RRIN: 162 parameter tensors, Super SloMo: 92 -- every one whose outer gradient both sides hold is compared"""
    loss, fps = S.oracle_run(model)
    assert _hold(_device_run(model, 1), loss, fps, 'net.', model + ' against the oracle') >= n_grads


@pytest.mark.parametrize("model", ["rrin", "superslomo"])
def test_second_order_through_the_flow_warp_raises_without_the_flag(model):
    """--warp_second_order 0: the warp's backward is once differentiable, the second-order pass fails loudly as it always did"""
    with pytest.raises(RuntimeError, match=S.ONCE):
        _device_run(model, 0)
