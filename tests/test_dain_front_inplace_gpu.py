"""-m gpu: MetaDAIN.front(..., out=alloc_front(...)) -- the frozen front built in place, its four warps writing their channel slices of the
rectify input -- against front() as it was: the same rectify_input and cur_output bit for bit and the same batch statistics, at 64 x 64
with one and three pairs and at 40 x 72 (padded to 64 x 128) with two; a second call into the same Front leaves nothing of the first;
front_evaluations counts pairs as before.
"""
import functools

import pytest
import torch

from meta_interpolation_amd.dain.networks.DAIN import MetaDAIN
from tests import dain_net_ref as R
from tests.test_dain_net_gpu import SEED, weights

pytestmark = pytest.mark.gpu
DEV = "cuda"


@functools.lru_cache(maxsize=None)
def network():
    net = MetaDAIN()
    net.load_state_dict({k: v.clone() for k, v in weights().items()}, strict=True)
    net.freeze_front()
    return net.to(DEV).train()


def pairs(B, H, W, salt=0):
    return tuple(R.numpy_rule_frames((B, 3, H, W), SEED + 700 + salt + 10 * i + B + W).to(DEV) for i in range(2))


def same_front(got, want):
    assert torch.equal(got.rectify_input, want.rectify_input)
    assert torch.equal(got.cur_output, want.cur_output)
    assert tuple(got.padding) == tuple(want.padding)
    assert set(got.bn_stats['count']) == set(want.bn_stats['count']) and got.bn_stats['count'] == want.bn_stats['count']
    assert got.bn_stats['npg'] == want.bn_stats['npg']
    for key in ('mean', 'var'):
        assert torch.equal(got.bn_stats[key], want.bn_stats[key]), key


@pytest.mark.parametrize("B, H, W", ((1, 64, 64), (3, 64, 64), (2, 40, 72)))
def test_front_in_place_equals_front(B, H, W):
    net = network()
    f0, f1 = pairs(B, H, W)
    n0 = net.front_evaluations
    want = net.front(f0, f1)
    assert net.front_evaluations == n0 + B
    out = MetaDAIN.alloc_front(B, H, W, DEV)
    Hp, Wp = (H + 63) // 64 * 64, (W + 63) // 64 * 64
    assert tuple(out.rectify_input.shape) == (B, 437, Hp, Wp) and tuple(out.cur_output.shape) == (B, 3, Hp, Wp)
    assert tuple(out.padding) == tuple(MetaDAIN.paddings(H, W)) and out.bn_stats is None
    addresses = (out.rectify_input.data_ptr(), out.cur_output.data_ptr())
    out.rectify_input.fill_(float('nan'))              # every element must be written
    out.cur_output.fill_(float('nan'))
    got = net.front(f0, f1, out=out)
    assert got is out and (out.rectify_input.data_ptr(), out.cur_output.data_ptr()) == addresses
    assert net.front_evaluations == n0 + 2 * B
    same_front(got, want)
    # the forward on either front gives the same frame, at the input's size
    with torch.no_grad():
        a = net.forward(f0, f1, front=want, update_stats=False)
        b = net.forward(f0, f1, front=got, update_stats=False)
    assert tuple(a.shape) == (B, 3, H, W) and torch.equal(a, b)


def test_second_call_into_the_same_front_leaves_nothing_stale():
    net = network()
    B, H, W = 2, 64, 64
    out = MetaDAIN.alloc_front(B, H, W, DEV)
    first = pairs(B, H, W)
    second = pairs(B, H, W, salt=3)
    net.front(*first, out=out)
    kept = out.rectify_input.clone()
    net.front(*second, out=out)
    want = net.front(*second)
    same_front(out, want)
    assert not torch.equal(out.rectify_input, kept)
    with pytest.raises(ValueError):
        net.front(*pairs(1, H, W), out=out)            # a Front for another batch


def test_update_stats_false_leaves_the_running_buffers_alone():
    net = network()
    f0, f1 = pairs(1, 64, 64)
    fr = net.front(f0, f1)
    before = {k: v.clone() for k, v in net.depthNet.state_dict().items()}
    with torch.no_grad():
        net.forward(f0, f1, front=fr, update_stats=False)
    assert all(torch.equal(v, net.depthNet.state_dict()[k]) for k, v in before.items())
    with torch.no_grad():
        net.forward(f0, f1, front=fr)
    tracked = [k for k in before if k.endswith('num_batches_tracked')]
    assert tracked and all(int(net.depthNet.state_dict()[k]) == int(before[k]) + 1 for k in tracked)
