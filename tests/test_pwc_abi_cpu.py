"""The C ABI of PWC-Net's correlation and warp (csrc/correlation.hip, added under ABI 24) and the module surface of dain/PWCNet as far
as they can be exercised without a GPU: the exported symbols, the unchanged version, the argument errors (every entry validates before
it launches, in the order NULL, SHAPE, UNSUPPORTED, TOOBIG), the refusal of host tensors and of other correlation configurations, and
the reference's 128 state-dict names and shapes."""
import subprocess

import pytest
import torch

from meta_interpolation_amd import _hip
from tests import pwc_ref as R

NEW = ("savfi_correlation_fwd_f32", "savfi_correlation_bwd_f32", "savfi_pwcwarp_fwd_f32")
E_NULL, E_SHAPE, E_UNSUPPORTED, E_TOOBIG = -1, -2, -3, -4
P = 0x10000          # a non-null, 16-byte aligned "device pointer": never dereferenced, every call below returns before a launch
BAD_DIMS = ((0, 3, 8, 8), (1, 0, 8, 8), (1, 3, 0, 8), (1, 3, 8, -1))


def test_library_exports_the_three_symbols_and_abi_is_still_24():
    lib = _hip.lib()
    assert lib.savfi_version() == 24 and _hip.ABI_VERSION == 24
    declared = _hip.declared_symbols()
    for name in NEW:
        assert name in declared and name in _hip._PROTOTYPES
        assert getattr(lib, name) is not None
    dyn = subprocess.run(["nm", "-D", "--defined-only", _hip.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in dyn.splitlines() if line.strip()}
    assert set(NEW) <= exported
    with open(_hip.HEADER_PATH) as fh:
        header = fh.read()
    assert "#define SAVFI_ABI_VERSION 24" in header and "INCOMPATIBLE" in header
    assert all(name in header.split("#define SAVFI_ABI_VERSION")[0] for name in NEW)       # listed as added under 24


def test_correlation_argument_errors():
    lib = _hip.lib()
    fwd, bwd = lib.savfi_correlation_fwd_f32, lib.savfi_correlation_bwd_f32
    for k in range(3):
        args = [P] * 3
        args[k] = None
        assert fwd(*args, 1, 3, 8, 8, 4, 1.0, None) == E_NULL
        assert bwd(*args, P, 0.1, P, P, 1, 3, 8, 8, 4, None) == E_NULL             # f1, f2, gout are required ...
    for dims in BAD_DIMS:
        assert fwd(P, P, P, *dims, 4, 1.0, None) == E_SHAPE
        assert bwd(P, P, P, P, 0.1, P, P, *dims, 4, None) == E_SHAPE
    # the order: NULL before SHAPE before UNSUPPORTED before TOOBIG
    assert fwd(None, P, P, 0, 3, 8, 8, 3, 1.0, None) == E_NULL
    assert fwd(P, P, P, 0, 3, 8, 8, 3, 1.0, None) == E_SHAPE
    assert fwd(P, P, P, 1, 3, 65536, 65536, 3, 1.0, None) == E_UNSUPPORTED
    assert bwd(P, P, P, None, 1.0, P, P, 1, 3, 65536, 65536, 3, None) == E_UNSUPPORTED
    for md in (3, 5, 0, -4, 20):
        assert fwd(P, P, P, 1, 3, 8, 8, md, 1.0, None) == E_UNSUPPORTED
        assert bwd(P, P, P, P, 0.1, P, P, 1, 3, 8, 8, md, None) == E_UNSUPPORTED
    for dims in ((1, 3, 65536, 65536),           # H W past the 32-bit in-plane index
                 (1, 3, 1, 2 ** 31 - 100),       # 2^31 - 257 < H W < 2^31: block * threads + thread would wrap
                 (1, 3, 4 * 65535 + 1, 2),       # more than 65535 rows of workgroups
                 (4, 65535, 4096, 4096),         # N C H W >= 2^40
                 (16, 1, 32768, 32768),          # 81 output channels: N 81 H W >= 2^40 although N C H W is not
                 (65536, 1, 2, 2), (1, 65536, 2, 2),
                 (4096, 256, 2, 2)):             # N ceil(C / 16) > 65535: the backward's grid
        assert fwd(P, P, P, *dims, 4, 1.0, None) == E_TOOBIG, dims
        assert bwd(P, P, P, P, 0.1, P, P, *dims, 4, None) == E_TOOBIG, dims
    # ... `out` and the two gradients are optional: with no gradient asked for there is nothing to launch
    assert bwd(P, P, P, None, 1.0, None, None, 1, 3, 8, 8, 4, None) == 0
    assert bwd(P, P, P, P, 0.1, None, None, 2, 196, 4, 7, 4, None) == 0


def test_pwcwarp_argument_errors():
    fwd = _hip.lib().savfi_pwcwarp_fwd_f32
    for k in range(3):
        args = [P, P, 1.0, P]
        args[k + (k == 2)] = None
        assert fwd(*args, 1, 3, 8, 8, None) == E_NULL
    for dims in BAD_DIMS:
        assert fwd(P, P, 1.0, P, *dims, None) == E_SHAPE
    assert fwd(None, P, 1.0, P, 0, 3, 8, 8, None) == E_NULL
    for dims in ((1, 3, 65536, 65536), (1, 3, 1, 2 ** 31 - 100), (4, 65535, 4096, 4096), (65536, 1, 2, 2), (1, 65536, 2, 2),
                 (4096, 136, 2, 2)):             # N ceil(C / 8) > 65535
        assert fwd(P, P, 0.625, P, *dims, None) == E_TOOBIG, dims


def test_ops_and_modules_refuse_host_tensors():
    from meta_interpolation_amd import hip_ops
    from meta_interpolation_amd.dain.PWCNet.PWCNet import PWCDCNet
    from meta_interpolation_amd.dain.PWCNet.correlation_package_pytorch1_0.correlation import Correlation
    a, b, fl = torch.zeros(1, 3, 4, 4), torch.zeros(1, 3, 4, 4), torch.zeros(1, 2, 4, 4)
    with pytest.raises(NotImplementedError):
        hip_ops.correlation(a, b)
    with pytest.raises(NotImplementedError):
        hip_ops.correlation(a, b, md=4, slope=0.1)
    with pytest.raises(NotImplementedError):
        hip_ops.pwc_warp(a, fl, 0.625)
    with pytest.raises(NotImplementedError):
        Correlation(pad_size=4, kernel_size=1, max_displacement=4, stride1=1, stride2=1, corr_multiply=1)(a, b)
    torch.manual_seed(0)
    with pytest.raises(NotImplementedError):
        PWCDCNet()(torch.zeros(1, 6, 64, 64))
    assert hip_ops.correlation_bytes(1, 32, 64, 112) == 4 * 64 * 112 * (64 + 81)
    assert hip_ops.correlation_bytes(1, 32, 64, 112, grads=1) == 4 * 64 * 112 * (128 + 162)
    assert hip_ops.pwc_warp_bytes(2, 32, 64, 112) == 4 * 2 * 64 * 112 * 66


def test_correlation_refuses_other_configurations():
    from meta_interpolation_amd.dain.PWCNet.correlation_package_pytorch1_0.correlation import Correlation, CorrelationFunction
    ok = dict(pad_size=4, kernel_size=1, max_displacement=4, stride1=1, stride2=1, corr_multiply=1)
    Correlation(**ok)
    for key, value in (('pad_size', 3), ('kernel_size', 3), ('max_displacement', 20), ('stride1', 2), ('stride2', 2), ('corr_multiply', 2)):
        with pytest.raises(NotImplementedError, match="pad_size = max_displacement = 4, kernel_size = 1, stride1 = stride2 = 1"):
            Correlation(**dict(ok, **{key: value}))
    with pytest.raises(NotImplementedError, match="kernel_size = 1"):
        Correlation()                                                            # the reference's defaults are not PWC-Net's either
    with pytest.raises(NotImplementedError, match="kernel_size = 1"):
        CorrelationFunction.apply(torch.zeros(1, 3, 4, 4), torch.zeros(1, 3, 4, 4), 3, 3, 20, 1, 2, 1)


def test_state_dict_has_the_reference_names_and_shapes():
    from meta_interpolation_amd.dain.PWCNet.PWCNet import PWCDCNet, pwc_dc_net
    torch.manual_seed(1)
    net = PWCDCNet()
    sd = net.state_dict()
    expected = R.expected_state_dict_shapes()
    assert len(expected) == 128 and set(sd) == set(expected)
    for k, shape in expected.items():
        assert tuple(sd[k].shape) == shape, k
    assert hasattr(net, 'deconv2') and not hasattr(net, 'upfeat2')
    # Kaiming (fan_in, gain sqrt 2) weights and zero biases, as the reference initialises every Conv2d and ConvTranspose2d
    for k, v in sd.items():
        if k.endswith('bias'):
            assert not v.any(), k
    w = sd['conv5_1.0.weight']
    assert abs(float(w.std()) / (2.0 / (w.shape[1] * 9)) ** 0.5 - 1.0) < 0.02
    w = sd['upfeat6.weight']                                                     # ConvTranspose2d [in, out, k, k]: torch's fan_in is out * k * k
    assert abs(float(w.std()) / (2.0 / (w.shape[1] * 16)) ** 0.5 - 1.0) < 0.05
    # a strict load of reference-named tensors round-trips, through pwc_dc_net's two file layouts as well
    other = {k: torch.full_like(v, 0.5) for k, v in sd.items()}
    net.load_state_dict(other, strict=True)
    assert all(bool((v == 0.5).all()) for v in net.state_dict().values())
    assert isinstance(pwc_dc_net(), PWCDCNet)


def test_model_dain_says_the_flow_estimator_exists():
    import argparse
    from meta_interpolation_amd import meta_learning_system as mls
    args = argparse.Namespace(cuda=False, batch_size=1, mode='train', random_seed=0, model='dain', resume=False)
    with pytest.raises(NotImplementedError, match="flow estimator") as exc:
        mls.SceneAdaptiveInterpolation(args)
    assert "PWCDCNet" in str(exc.value) and "two own ops" in str(exc.value)
