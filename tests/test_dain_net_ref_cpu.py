"""The restatements of tests/dain_net_ref.py against tests/golden/dain_net.npz (written by tools/gen_dain_golden.py from the reference's own
modules with the same numpy-rule weights), the names and shapes of the product's DAIN modules against the same fixture, and the argument
errors of the new C entries (csrc/dainnet.hip, the Charbonnier entries of csrc/loss.hip) -- all without a GPU.

float64 restatement vs. float64 reference: 1e-12 relative to the output's largest value; float32 vs. float32: a few ulps of the same
(torch's host convolutions may pick another summation order for another batch slicing, the BatchNorm per group is sliced differently).
"""
import functools

import numpy as np
import pytest
import torch

from meta_interpolation_amd import _hip
from tests import dain_net_ref as R
from tests.helpers import golden

SEED = 4100          # tools/gen_dain_golden.py
E_NULL, E_SHAPE, E_UNSUPPORTED, E_TOOBIG = -1, -2, -3, -4
P = 0x10000          # a non-null, 16-byte aligned "device pointer": never dereferenced, every call below returns before a launch
NEW = ("savfi_bn_stats_scratch_floats", "savfi_bn_stats_f32", "savfi_bn_apply_relu_f32", "savfi_bn_running_update_f32",
       "savfi_maxpool2x2_f32", "savfi_upnearest2x_add_f32", "savfi_add_relu_f32", "savfi_charbonnier_f32", "savfi_charbonnier_bwd_f32")


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(golden("dain_net"))


def close(got, want, rel, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err, scale = float(np.abs(got - want).max()), float(np.abs(want).max())
    assert err <= rel * max(scale, 1e-30), (what, err, scale)


DTYPES = ((torch.float64, 'f64', 1e-12), (torch.float32, 'f32', 2e-5))


@pytest.fixture(autouse=True)
def _one_host_thread():
    """The fixture was computed with one host thread: torch's host reductions are cut by the thread count, and the hourglass's deepest
    BatchNorms (two values per channel at 16x16) amplify a last-bit difference to 1e-11."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


# ---------------------------------------------------------------------------------------------------------------------------------
# names and shapes
# ---------------------------------------------------------------------------------------------------------------------------------
def _shape_list(shapes):
    return [','.join(str(s) for s in v) for v in shapes.values()]


def test_restated_names_and_shapes_are_the_references():
    fx = fixture()
    hg = R.hourglass_shapes()
    assert len(hg) == 779
    assert list(hg) == list(fx['hourglass_keys']) and _shape_list(hg) == list(fx['hourglass_shapes'])
    ours = R.metadain_shapes()
    assert set(ours) == set(fx['metadain_keys'])
    want = dict(zip(fx['metadain_keys'], fx['metadain_shapes']))
    assert all(','.join(str(s) for s in ours[k]) == want[k] for k in ours)


def test_product_modules_have_the_references_names_and_shapes():
    from meta_interpolation_amd.dain.MegaDepth import HourGlass
    from meta_interpolation_amd.dain.networks.DAIN import MetaDAIN
    fx = fixture()
    torch.manual_seed(3)
    hg = HourGlass()
    sd = hg.state_dict()
    assert list(sd) == list(fx['hourglass_keys'])
    assert [','.join(str(s) for s in v.shape) for v in sd.values()] == list(fx['hourglass_shapes'])
    state = R.numpy_rule_state(R.hourglass_shapes(), SEED)
    hg.load_state_dict(state, strict=True)                                      # a strict load round-trips
    assert all(torch.equal(v, state[k]) for k, v in hg.state_dict().items())

    net = MetaDAIN()
    own = {k: v for k, v in net.state_dict().items() if not k.startswith('flownets.')}
    want = dict(zip(fx['metadain_keys'], fx['metadain_shapes']))
    assert list(own) == list(fx['metadain_keys'])
    assert all(','.join(str(s) for s in v.shape) == want[k] for k, v in own.items())
    from tests import pwc_ref
    assert {k[len('flownets.'):] for k in net.state_dict() if k.startswith('flownets.')} == set(pwc_ref.expected_state_dict_shapes())
    other = {k: torch.full_like(v, 2) for k, v in net.state_dict().items()}
    net.load_state_dict(other, strict=True)
    assert all(bool((v == 2).all()) for v in net.state_dict().values())


def test_inner_loop_names_are_the_ten_rectify_tensors_once_frozen():
    from meta_interpolation_amd.dain.networks.DAIN import MetaDAIN
    torch.manual_seed(3)
    net = MetaDAIN()
    assert sum(p.requires_grad for p in net.parameters()) > 10
    net.freeze_front()
    assert [k for k, p in net.named_parameters() if p.requires_grad] == ['rectifyNet.' + k for k in R.RECTIFY_NAMES]
    assert [tuple(p.shape) for k, p in net.named_parameters() if p.requires_grad] == [R.rectify_shapes()[k] for k in R.RECTIFY_NAMES]
    assert MetaDAIN.paddings(64, 64) == (0, 0, 0, 0) and MetaDAIN.paddings(40, 72) == (28, 28, 12, 12)
    assert MetaDAIN.paddings(256, 448) == (0, 0, 0, 0) and MetaDAIN.paddings(65, 130) == (31, 31, 31, 32)


# ---------------------------------------------------------------------------------------------------------------------------------
# the restatements equal the reference's modules
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", (16, 64))
def test_hourglass_restatement(size):
    fx = fixture()
    state = R.numpy_rule_state(R.hourglass_shapes(), SEED)
    x = R.numpy_rule_frames((2, 3, size, size), SEED + 10 + size)
    for dtype, tag, rel in DTYPES:
        y1, after1 = R.hourglass_forward(state, x, dtype, training=True)
        y2, after2 = R.hourglass_forward(after1, x.to(dtype).flip(0) * 0.5, dtype, training=True)
        close(R.golden_view('hg', size, y1.numpy()), fx['hg_train_%s_%d' % (tag, size)], rel, ('train', tag))
        close(R.golden_view('hg', size, y2.numpy()), fx['hg_train2_%s_%d' % (tag, size)], rel, ('train2', tag))
        for name, after in (('after1', after1), ('after2', after2)):
            for key in R.GOLDEN_BUFFERS:
                close(after[key].numpy(), fx['hg_%s_%s_%d_%s' % (name, tag, size, key)], rel, (name, key, tag))
            for kind in ('mean', 'var'):
                total = sum(float(v.double().sum()) for k, v in after.items() if k.endswith('running_' + kind))
                close(total, fx['hg_%s_%s_%d_sum_%s' % (name, tag, size, kind)], 10 * rel, (name, kind, tag))
        assert int(after2['1.num_batches_tracked']) == 2
        ye, same = R.hourglass_forward(state, x, dtype, training=False)
        close(R.golden_view('hg', size, ye.numpy()), fx['hg_eval_%s_%d' % (tag, size)], rel, ('eval', tag))
        assert all(torch.equal(same[k], state[k].to(same[k].dtype)) for k in state)          # eval mode updates nothing


def test_hourglass_groups_are_calls_of_their_own():
    """Two groups of two samples in one call: each group's output and the buffers are those of two calls in a row."""
    state = R.numpy_rule_state(R.hourglass_shapes(), SEED)
    x = R.numpy_rule_frames((4, 3, 16, 16), SEED + 40)
    y, after = R.hourglass_forward(state, x, torch.float64, training=True, n_per_group=2)
    ya, mid = R.hourglass_forward(state, x[:2], torch.float64, training=True)
    yb, end = R.hourglass_forward(mid, x[2:], torch.float64, training=True)
    close(y.numpy(), torch.cat((ya, yb)).numpy(), 1e-13, 'groups')
    for k in R.GOLDEN_BUFFERS:
        close(after[k].numpy(), end[k].numpy(), 1e-13, k)


@pytest.mark.parametrize("size", (16, 64))
def test_context_net_restatement(size):
    fx = fixture()
    state = R.numpy_rule_state(R.s2df_shapes(), SEED + 1)
    x = R.numpy_rule_frames((2, 3, size, size), SEED + 10 + size)
    for dtype, tag, rel in DTYPES:
        y = R.s2df_forward(state, x, dtype).numpy()
        assert y.shape == (2, 195, size, size) and np.array_equal(y[:, :3], x.to(dtype).numpy())
        close(R.golden_view('ctx', size, y), fx['ctx_%s_%d' % (tag, size)], rel, ('ctx', tag))
        close(y.astype(np.float64).sum(), fx['ctx_sum_%s_%d' % (tag, size)], 100 * rel, ('ctx sum', tag))


@pytest.mark.parametrize("size", (32, 64))
def test_filter_net_restatement(size):
    fx = fixture()
    state = R.numpy_rule_state(R.filternet_shapes(), SEED + 2)
    x6 = R.numpy_rule_frames((2, 6, size, size), SEED + 20 + size)
    for dtype, tag, rel in DTYPES:
        trunk, h1, h2 = R.filternet_forward(state, x6, dtype)
        heads = torch.stack((h1, h2)).numpy()
        assert trunk.shape == (2, 16, size, size) and heads.shape == (2, 2, 16, size, size)
        close(R.golden_view('heads', size, heads), fx['filter_heads_%s_%d' % (tag, size)], rel, ('heads', tag))
        close(heads.astype(np.float64).sum(), fx['filter_heads_sum_%s_%d' % (tag, size)], 100 * rel, ('heads sum', tag))


def test_rectify_net_and_charbonnier_restatement():
    fx = fixture()
    state = R.numpy_rule_state(R.rectify_shapes(), SEED + 3)
    ri = R.numpy_rule_frames((1, 437, 16, 16), SEED + 30) - 0.5
    cur = R.numpy_rule_frames((1, 3, 16, 16), SEED + 31)
    for dtype, tag, rel in DTYPES:
        tgt = torch.from_numpy(fx['rect_target_%s' % tag])
        frame, loss, grads = R.rectify_loss_and_grads(state, ri, cur, tgt, dtype)
        close(frame.numpy(), fx['rect_frame_%s' % tag], rel, ('frame', tag))
        close(loss.numpy(), fx['rect_loss_%s' % tag], rel, ('loss', tag))
        for k in R.RECTIFY_NAMES:
            flat = grads[k].double().flatten()
            got = np.concatenate(([float(flat.sum()), float(flat.abs().sum())], flat[:32].numpy()))
            want = fx['rect_grad_%s_%s' % (tag, k)]
            # the sum of a gradient cancels: its error is measured against the absolute sum
            assert abs(got[0] - want[0]) <= 100 * rel * want[1], (k, tag)
            close(got[1:], want[1:], 10 * rel, (k, tag))
    assert float(R.charbonnier(torch.zeros(4, dtype=torch.float64), torch.zeros(4, dtype=torch.float64))) == 1e-8


# ---------------------------------------------------------------------------------------------------------------------------------
# the C entries validate before they launch
# ---------------------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_new_symbols_under_abi_24():
    lib = _hip.lib()
    assert lib.savfi_version() == 24 and _hip.ABI_VERSION == 24
    declared = _hip.declared_symbols()
    with open(_hip.HEADER_PATH) as fh:
        listed = fh.read().split("#define SAVFI_ABI_VERSION")[0]
    for name in NEW:
        assert name in declared and name in _hip._PROTOTYPES and getattr(lib, name) is not None
        assert name in listed                                                    # listed as added under 24


def test_batchnorm_argument_errors():
    lib = _hip.lib()
    stats, apply_, scratch = lib.savfi_bn_stats_f32, lib.savfi_bn_apply_relu_f32, lib.savfi_bn_stats_scratch_floats
    for k in range(3):
        a = [P, P, P]
        a[k] = None
        assert stats(*a, 16, P, 2, 16, 4, 4, 2, None) == E_NULL
    assert stats(P, P, P, 16, None, 2, 4, 128, 128, 2, None) == E_NULL           # scratch is required above the split
    for dims in ((0, 16, 4, 4), (2, 0, 4, 4), (2, 16, 0, 4), (2, 16, 4, -1)):
        assert stats(P, P, P, 16, P, *dims, 2, None) == E_SHAPE
        assert apply_(P, P, P, 16, None, None, 1e-5, P, *dims, 2, 0, 16, None) == E_SHAPE
        assert scratch(*dims, 2) == E_SHAPE
    # a batch that is not a multiple of n_per_group
    for npg in (0, -1, 2, 4):
        assert stats(P, P, P, 16, P, 3, 16, 4, 4, npg, None) == E_SHAPE
        assert apply_(P, P, P, 16, None, None, 1e-5, P, 3, 16, 4, 4, npg, 0, 16, None) == E_SHAPE
        assert scratch(3, 16, 4, 4, npg) == E_SHAPE
    # a count of one value per channel
    assert stats(P, P, P, 16, P, 1, 16, 1, 1, 1, None) == E_SHAPE
    assert stats(P, P, P, 16, P, 4, 16, 1, 1, 1, None) == E_SHAPE
    # C_total smaller than c_off + C, a negative offset
    for c_off, c_total in ((0, 15), (5, 20), (-1, 32), (1, 16)):
        assert apply_(P, P, P, 16, None, None, 1e-5, P, 2, 16, 4, 4, 2, c_off, c_total, None) == E_SHAPE
    for k in (0, 1, 2, 7):
        a = [P, P, P, 16, None, None, 1e-5, P]
        a[k] = None
        assert apply_(*a, 2, 16, 4, 4, 2, 0, 16, None) == E_NULL
    assert apply_(P, P, P, 16, None, None, -1.0, P, 2, 16, 4, 4, 2, 0, 16, None) == E_UNSUPPORTED
    assert apply_(P, P, P, 16, None, None, float('nan'), P, 2, 16, 4, 4, 2, 0, 16, None) == E_UNSUPPORTED
    for dims in ((65536, 1, 2, 2), (2, 65536, 2, 2), (2, 2, 65536, 65536), (4, 65535, 4096, 4096)):
        assert stats(P, P, P, 16, P, *dims, 2, None) == E_TOOBIG, dims
        assert apply_(P, P, P, 16, None, None, 1e-5, P, *dims, 2, 0, dims[1], None) == E_TOOBIG, dims
    # the order: NULL before SHAPE before TOOBIG
    assert stats(None, P, P, 16, P, 0, 16, 4, 4, 2, None) == E_NULL
    assert stats(P, P, P, 16, P, 65536, 1, 1, 1, 1, None) == E_SHAPE
    # the split: one workgroup up to 16384 values per (group, channel), pieces of 8192 values of a plane above
    assert scratch(2, 16, 64, 128, 2) == 0 and scratch(1, 16, 128, 128, 1) == 0
    assert scratch(2, 16, 64, 129, 2) == 2 * 16 * 2 * 2 and scratch(1, 3, 1, 16385, 1) == 2 * 3 * 3
    assert scratch(4, 16, 64, 129, 2) == 2 * scratch(2, 16, 64, 129, 2)          # per group: what the batch holds besides changes nothing

    upd = lib.savfi_bn_running_update_f32
    ptrs, n1 = _hip.ptr_array([]), _hip.i64_array([4])
    one = (_hip.c_void_p * 1)(P)
    null = (_hip.c_void_p * 1)(None)
    assert upd(0, None, None, None, None, 0.1, None) == 0 and upd(-1, ptrs, ptrs, n1, None, 0.1, None) == E_SHAPE
    assert upd(1, None, one, n1, None, 0.1, None) == E_NULL and upd(1, null, one, n1, None, 0.1, None) == E_NULL
    assert upd(1, one, null, n1, None, 0.1, None) == E_NULL
    assert upd(1, one, one, _hip.i64_array([0]), None, 0.1, None) == E_SHAPE
    assert upd(1, one, one, _hip.i64_array([2 ** 31]), None, 0.1, None) == E_TOOBIG
    assert upd(1, one, one, n1, None, 1.5, None) == E_UNSUPPORTED


def test_pool_upsample_add_relu_and_charbonnier_argument_errors():
    lib = _hip.lib()
    pool, up, add = lib.savfi_maxpool2x2_f32, lib.savfi_upnearest2x_add_f32, lib.savfi_add_relu_f32
    assert pool(None, P, 4, 8, 8, None) == E_NULL and pool(P, None, 4, 8, 8, None) == E_NULL
    for planes, h, w in ((0, 8, 8), (4, 1, 8), (4, 8, 1), (4, 0, 0), (-1, 8, 8)):
        assert pool(P, P, planes, h, w, None) == E_SHAPE
    assert pool(P, P, 65536, 8, 8, None) == E_TOOBIG and pool(P, P, 4, 65536, 65536, None) == E_TOOBIG
    for k in range(3):
        a = [P, P, P]
        a[k] = None
        assert up(*a, 4, 3, 5, 6, 10, None) == E_NULL
        assert add(*a, 16, None) == E_NULL
    # a skip that is not exactly twice low
    for h, w, H, W in ((3, 5, 6, 11), (3, 5, 7, 10), (3, 5, 3, 5), (3, 5, 5, 10), (0, 5, 0, 10), (3, -5, 6, -10)):
        assert up(P, P, P, 4, h, w, H, W, None) == E_SHAPE
    assert up(P, P, P, 0, 3, 5, 6, 10, None) == E_SHAPE and up(P, P, P, 65536, 3, 5, 6, 10, None) == E_TOOBIG
    assert add(P, P, P, 0, None) == E_SHAPE and add(P, P, P, -4, None) == E_SHAPE and add(P, P, P, 2 ** 40, None) == E_TOOBIG

    fwd, bwd = lib.savfi_charbonnier_f32, lib.savfi_charbonnier_bwd_f32
    for k in range(4):
        a = [P, P, P, P]
        a[k] = None
        assert fwd(*a, 1, 16, 1e-8, None) == E_NULL and bwd(*a, 1, 16, 1e-8, None) == E_NULL
    for rows, n in ((0, 16), (1, 0), (65536, 16), (-1, 16)):
        assert fwd(P, P, P, P, rows, n, 1e-8, None) == E_SHAPE and bwd(P, P, P, P, rows, n, 1e-8, None) == E_SHAPE
    for eps in (0.0, -1e-8, float('nan')):
        assert fwd(P, P, P, P, 1, 16, eps, None) == E_UNSUPPORTED and bwd(P, P, P, P, 1, 16, eps, None) == E_UNSUPPORTED
    assert fwd(None, P, P, P, 0, 16, 0.0, None) == E_NULL and fwd(P, P, P, P, 0, 16, 0.0, None) == E_SHAPE


def test_new_ops_refuse_host_tensors_and_a_count_of_one():
    from meta_interpolation_amd import hip_ops
    from meta_interpolation_amd.dain.MegaDepth import HourGlass
    from meta_interpolation_amd.dain.S2D_models import S2DF_3dense
    from meta_interpolation_amd.dain.Resblock import MetaMultipleBasicBlock_4
    from meta_interpolation_amd.dain.networks.DAIN import MetaDAIN
    x, s = torch.zeros(2, 4, 4, 4), torch.zeros(1, 4)
    for call in (lambda: hip_ops.bn_stats(x, 2), lambda: hip_ops.bn_apply_relu(x, s, s, 2), lambda: hip_ops.max_pool2x2(x),
                 lambda: hip_ops.upnearest2x_add(x, torch.zeros(2, 4, 8, 8)), lambda: hip_ops.add_relu(x, x),
                 lambda: hip_ops.charbonnier_loss(x, x), lambda: hip_ops.charbonnier_loss_per_sample(x, x),
                 lambda: hip_ops.bn_running_update([s[0]], [s[0]], [1.0])):
        with pytest.raises(NotImplementedError):
            call()
    torch.manual_seed(0)
    with pytest.raises(NotImplementedError):
        HourGlass()(torch.zeros(2, 3, 16, 16))
    with pytest.raises(NotImplementedError):
        S2DF_3dense()(torch.zeros(1, 3, 16, 16))
    with pytest.raises(NotImplementedError):
        MetaMultipleBasicBlock_4(8, 8)(torch.zeros(1, 8, 8, 8))
    net = MetaDAIN()
    with pytest.raises(NotImplementedError):
        net.front(torch.zeros(1, 3, 64, 64), torch.zeros(1, 3, 64, 64))
    with pytest.raises(NotImplementedError):
        net(torch.zeros(1, 3, 64, 64), torch.zeros(1, 3, 64, 64))
    assert net.front_evaluations == 0
