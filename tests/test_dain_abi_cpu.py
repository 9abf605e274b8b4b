"""The C ABI of DAIN's two ops (csrc/dainwarp.hip, ABI 24) as far as it can be exercised without a GPU: the exported symbols, the
version, the argument errors (every entry validates before it launches, in the order NULL, SHAPE, UNSUPPORTED, TOOBIG) and the module
surface's refusal of host tensors."""
import subprocess

import pytest
import torch

from meta_interpolation_amd import _hip

NEW = ("savfi_filterinterp_fwd_f32", "savfi_filterinterp_bwd_f32", "savfi_depthflowproj_scratch_bytes",
       "savfi_depthflowproj_fwd_f32", "savfi_depthflowproj_bwd_f32")
E_NULL, E_SHAPE, E_UNSUPPORTED, E_TOOBIG = -1, -2, -3, -4
P = 0x10000          # a non-null, 16-byte aligned "device pointer": never dereferenced, every call below returns before a launch


def test_library_exports_the_five_symbols_and_abi_24():
    lib = _hip.lib()
    assert lib.savfi_version() == 24 and _hip.ABI_VERSION == 24
    declared = _hip.declared_symbols()
    for name in NEW:
        assert name in declared and name in _hip._PROTOTYPES
        assert getattr(lib, name) is not None
    dyn = subprocess.run(["nm", "-D", "--defined-only", _hip.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in dyn.splitlines() if line.strip()}
    assert set(NEW) <= exported


def test_filterinterp_argument_errors():
    lib = _hip.lib()
    fwd, bwd = lib.savfi_filterinterp_fwd_f32, lib.savfi_filterinterp_bwd_f32
    for k in range(4):
        args = [P] * 4
        args[k] = None
        assert fwd(*args, 1, 3, 8, 8, 4, None) == E_NULL
        assert bwd(*args, P, P, P, 1, 3, 8, 8, 4, None) == E_NULL          # in, flow, filt, gout are required ...
    for dims in ((0, 3, 8, 8), (1, 0, 8, 8), (1, 3, 0, 8), (1, 3, 8, -1)):
        assert fwd(P, P, P, P, *dims, 4, None) == E_SHAPE
        assert bwd(P, P, P, P, P, P, P, *dims, 4, None) == E_SHAPE
    assert fwd(None, P, P, P, 0, 3, 8, 8, 3, None) == E_NULL               # the order: NULL before SHAPE before UNSUPPORTED before TOOBIG
    assert fwd(P, P, P, P, 0, 3, 8, 8, 3, None) == E_SHAPE
    assert fwd(P, P, P, P, 1, 3, 65536, 65536, 3, None) == E_UNSUPPORTED
    for fs in (3, 5, 0, 6):
        assert fwd(P, P, P, P, 1, 3, 8, 8, fs, None) == E_UNSUPPORTED
        assert bwd(P, P, P, P, P, P, P, 1, 3, 8, 8, fs, None) == E_UNSUPPORTED
    for dims in ((1, 3, 65536, 65536),           # H W past the 32-bit in-plane index
                 (1, 3, 1, 2 ** 31 - 100),       # 2^31 - 257 < H W < 2^31: block * 256 + thread would wrap
                 (4, 65535, 4096, 4096),         # B C H W >= 2^40
                 (65536, 1, 2, 2), (1, 65536, 2, 2)):
        assert fwd(P, P, P, P, *dims, 4, None) == E_TOOBIG
        assert bwd(P, P, P, P, P, P, P, *dims, 4, None) == E_TOOBIG
    # ... and the three gradients are optional: with none asked for there is nothing to launch
    assert bwd(P, P, P, P, None, None, None, 1, 3, 8, 8, 4, None) == 0


def test_depthflowproj_argument_errors():
    lib = _hip.lib()
    fwd, bwd, size = lib.savfi_depthflowproj_fwd_f32, lib.savfi_depthflowproj_bwd_f32, lib.savfi_depthflowproj_scratch_bytes
    for k in range(5):
        args = [P] * 5
        args[k] = None
        assert fwd(*args, 1, 8, 8, 1, None) == E_NULL
    for k in range(5):                                                       # flow, w, count, out, gout are required ...
        args = [P] * 7
        args[k] = None
        assert bwd(*args, 1, 8, 8, None) == E_NULL
    assert bwd(P, P, P, P, P, None, None, 1, 8, 8, None) == 0                # ... the two gradients are optional: nothing to launch
    for dims in ((0, 8, 8), (1, 0, 8), (1, 8, -3)):
        assert fwd(P, P, P, P, P, *dims, 0, None) == E_SHAPE
        assert bwd(P, P, P, P, P, P, P, *dims, None) == E_SHAPE
        assert size(*dims) == E_SHAPE
    assert fwd(None, P, P, P, P, 0, 8, 8, 0, None) == E_NULL
    for dims in ((1, 65536, 65536), (1, 1, 2 ** 31 - 100), (65536, 2, 2), (30000, 4096, 4096)):
        assert fwd(P, P, P, P, P, *dims, 1, None) == E_TOOBIG
        assert bwd(P, P, P, P, P, P, P, *dims, None) == E_TOOBIG
        assert size(*dims) == E_TOOBIG
    assert fwd(P, P, P, P, P + 4, 1, 8, 8, 1, None) == E_UNSUPPORTED        # the 64-bit accumulators need an 8-byte aligned scratch
    # three 64-bit sums a pixel and one 32-bit maximum a sample, rounded up to 8 bytes
    assert size(1, 8, 8) == 64 * 24 + 8 and size(2, 7, 9) == 2 * 63 * 24 + 8 and size(3, 4, 4) == 3 * 16 * 24 + 16
    assert size(2, 720, 1280) == 2 * 720 * 1280 * 24 + 8


def test_modules_refuse_host_tensors():
    from meta_interpolation_amd import hip_ops
    from meta_interpolation_amd.dain.my_package.DepthFlowProjection import DepthFlowProjectionModule
    from meta_interpolation_amd.dain.my_package.FilterInterpolation import FilterInterpolationModule
    x, fl, ft, w = torch.zeros(1, 3, 4, 4), torch.zeros(1, 2, 4, 4), torch.zeros(1, 16, 4, 4), torch.ones(1, 1, 4, 4)
    with pytest.raises(NotImplementedError):
        FilterInterpolationModule()(x, fl, ft)
    for requires_grad in (True, False):
        m = DepthFlowProjectionModule(requires_grad)
        assert m.requires_grad is requires_grad
        with pytest.raises(NotImplementedError):
            m(fl, w)
    with pytest.raises(NotImplementedError):
        hip_ops.filter_interpolation(x, fl, ft)
    with pytest.raises(NotImplementedError):
        hip_ops.depth_flow_projection(fl, w, True)


def test_model_dain_still_raises_and_says_what_exists():
    import argparse
    from meta_interpolation_amd import meta_learning_system as mls
    args = argparse.Namespace(cuda=False, batch_size=1, mode='train', random_seed=0, model='dain', resume=False)
    with pytest.raises(NotImplementedError, match="ops exist|two own ops"):
        mls.SceneAdaptiveInterpolation(args)
