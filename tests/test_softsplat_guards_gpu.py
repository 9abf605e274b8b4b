"""-m gpu: hip_ops.softsplat, forward and backward, on the ragged shapes with every launch between canaries (helpers.guarded_calls: each
tensor's storage, the 64-bit scratch included, sits between 4 KB canary regions) and on poisoned allocations (helpers.poisoned_empties:
torch.empty hands out NaN floats and 0xff scratch bytes).  No canary is touched, no NaN and no integer poison reaches a result -- every
output element is written and the scratch is cleared by the op's own kernel before it is read -- and the results are those of the plain
run bit for bit."""
import pytest
import torch

from tests import softsplat_ref as R
from tests.helpers import guarded_calls, integer_poison, poisoned_empties
from tests.test_softsplat_gpu import bits, ids, op_run

pytestmark = pytest.mark.gpu

RAGGED = [(2, 3, 7, 9), (1, 3, 33, 130), (1, 8, 5, 67)]           # no multiple of the 256-pixel workgroup, odd widths, C neither 1 nor 3


@pytest.mark.parametrize("shape", RAGGED, ids=ids)
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("kind", ['fractional', 'leave'])
def test_ragged_shape_between_canaries_on_poisoned_allocations(kind, mode, shape):
    tensors = R.inputs(kind, shape)
    plain = op_run(tensors, mode)
    with guarded_calls() as rec, poisoned_empties() as poison:
        got = op_run(tensors, mode)                                 # (a touched canary raises inside)
        torch.cuda.synchronize()
    assert rec.guarded["savfi_softsplat_fwd_f32"] == 1 and rec.guarded["savfi_softsplat_bwd_f32"] == 1
    assert poison.filled >= 5 + (3 if mode == 'soft' else 2)       # out, hit, D, M, scratch and the gradients
    big = float(integer_poison(torch.uint8))
    for name, p, q in zip(('out', 'hit', 'g_x', 'g_flow', 'g_metric'), plain, got):
        assert (p is None) == (q is None), name
        if p is None:
            continue
        assert not torch.isnan(q).any(), name
        assert torch.equal(bits(p), bits(q)), name
    # the scratch's poison is the byte 0xff: as a 64-bit accumulator -1, as a key the largest one -- either would show in hit / out
    assert set(got[1].unique().tolist()) <= {0.0, 1.0} and big == 255.0
