"""The C ABI of multi-scale SSIM (csrc/ssim.hip, added under ABI 24) as far as it can be exercised without a GPU: the exported symbols,
the version, the argument errors (validated before any launch, in the order NULL, SHAPE, UNSUPPORTED, TOOBIG) and the scratch query."""
import re
import subprocess

from meta_interpolation_amd import _hip

NEW = ("savfi_msssim_scratch_bytes", "savfi_msssim_f32", "savfi_msssim_bwd_f32")
E_NULL, E_SHAPE, E_UNSUPPORTED, E_TOOBIG = -1, -2, -3, -4
P = 0x10000          # a non-null, 16-byte aligned "device pointer": never dereferenced, every call below returns before a launch


def test_library_exports_the_three_symbols_under_abi_24():
    lib = _hip.lib()
    assert lib.savfi_version() == 24 and _hip.ABI_VERSION == 24
    declared = _hip.declared_symbols()
    for name in NEW:
        assert name in declared and name in _hip._PROTOTYPES
        assert getattr(lib, name) is not None
    dyn = subprocess.run(["nm", "-D", "--defined-only", _hip.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(NEW) <= {line.split()[-1] for line in dyn.splitlines() if line.strip()}
    with open(_hip.HEADER_PATH) as fh:
        text = fh.read()
    comment = text[:text.index("#define SAVFI_ABI_VERSION 24")].rsplit("/*", 1)[1]
    assert "Added under 24" in comment
    for name in NEW:
        assert re.search(r"\b%s\b" % name, comment), name


def test_argument_errors_come_before_any_launch():
    lib = _hip.lib()
    fwd, bwd, size = lib.savfi_msssim_f32, lib.savfi_msssim_bwd_f32, lib.savfi_msssim_scratch_bytes
    for k in range(4):
        args = [P] * 4
        args[k] = None
        assert fwd(*args, 1, 3, 64, 64, 0, 0, 0, None) == E_NULL
    for k in range(5):
        args = [P] * 5
        args[k] = None
        assert bwd(*args, 1, 3, 64, 64, 0, None) == E_NULL
    for dims in ((1, 3, 31, 64), (1, 3, 64, 31), (0, 3, 64, 64), (1, 0, 64, 64), (1, 3, 0, 64), (1, 3, 64, -1)):
        assert fwd(P, P, P, P, *dims, 0, 0, 0, None) == E_SHAPE
        assert bwd(P, P, P, P, P, *dims, 0, None) == E_SHAPE
        assert size(*dims) == E_SHAPE
    for mode in (-1, 6):
        assert fwd(P, P, P, P, 1, 3, 64, 64, mode, 0, 0, None) == E_UNSUPPORTED
        assert bwd(P, P, P, P, P, 1, 3, 64, 64, mode, None) == E_UNSUPPORTED
    for dims in ((1, 3, 65536, 65536), (65536, 1, 64, 64), (2, 32768, 64, 64)):      # the limits of the SSIM entries
        assert fwd(P, P, P, P, *dims, 0, 0, 0, None) == E_TOOBIG
        assert bwd(P, P, P, P, P, *dims, 0, None) == E_TOOBIG
        assert size(*dims) == E_TOOBIG
        assert lib.savfi_ssim_scratch_floats(*dims) == E_TOOBIG
    # the order
    assert fwd(None, P, P, P, 1, 3, 31, 64, -1, 0, 0, None) == E_NULL
    assert fwd(P, P, P, P, 1, 3, 31, 64, -1, 0, 0, None) == E_SHAPE
    assert fwd(P, P, P, P, 1, 3, 65536, 65536, -1, 0, 0, None) == E_UNSUPPORTED
    assert fwd(P, P, P, P, 1, 3, 65536, 65536, 0, 0, 0, None) == E_TOOBIG


def test_scratch_query_by_hand():
    """32-bit words, every region rounded up to four: 16 per row of head; for the pooled levels 1..4 two images and one gradient of
    rows C (H >> s) (W >> s); per level 2 partial sums per workgroup of the 16 x 64 tiling of its (H_s - n_s + 1) x (W_s - n_s + 1) map;
    partial extrema: 2 x 256 per row for level 0, 2 per workgroup of the level above after that."""
    size = _hip.lib().savfi_msssim_scratch_bytes
    # 1 x 3 x 32 x 32: sizes 32 16 8 4 2, taps 11 11 8 4 2, maps 22 6 1 1 1 -> workgroups per plane 2 1 1 1 1
    head = 16
    pooled = 3 * (3 * 16 * 16 + 3 * 8 * 8 + 3 * 4 * 4 + 3 * 2 * 2)
    partial = 2 * 3 * 2 + 4 * 8                       # 12, then 6 -> 8 four times
    extrema = 2 * 256 + 2 * 3 * 2 + 3 * 8             # level 1 reads level 0's 6 workgroups; 6 -> 8 three times
    assert size(1, 3, 32, 32) == 4 * (head + pooled + partial + extrema) == 14672
    # 2 x 3 x 37 x 53: sizes 37x53 18x26 9x13 4x6 2x3, taps 11 11 9 4 2, maps 27x43 8x16 1x5 1x3 1x2 -> workgroups per plane 2 1 1 1 1
    head = 32
    pooled = 3 * (6 * 18 * 26 + 704 + 6 * 4 * 6 + 6 * 2 * 3)          # 6 * 9 * 13 = 702 -> 704
    partial = 2 * 6 * 2 + 4 * 12
    extrema = 2 * 2 * 256 + 2 * 6 * 2 + 3 * 12
    assert size(2, 3, 37, 53) == 4 * (head + pooled + partial + extrema) == 49056
