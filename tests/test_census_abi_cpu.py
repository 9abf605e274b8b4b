"""The C ABI of the census loss (csrc/census.hip, added under ABI 24) as far as it can be exercised without a GPU: the exported symbols,
the version, the argument errors (validated before any launch, in the order NULL, SHAPE, UNSUPPORTED, TOOBIG) and the scratch query
against the layout include/savfi_hip.h documents."""
import re
import subprocess

from meta_interpolation_amd import _hip

NEW = ("savfi_census_scratch_bytes", "savfi_census_f32", "savfi_census_bwd_f32")
E_NULL, E_SHAPE, E_UNSUPPORTED, E_TOOBIG = -1, -2, -3, -4
P = 0x10000          # non-null, 16-byte aligned "device pointers": never dereferenced, every call below returns before a launch
A, B, C, D = 0x10000, 0x20000, 0x30000, 0x40000


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
    fwd, bwd, size = lib.savfi_census_f32, lib.savfi_census_bwd_f32, lib.savfi_census_scratch_bytes
    good = (1, 1, 3, 64, 64)          # rows, n, C, H, W
    for k in range(4):
        args = [A, B, C, D]
        args[k] = None
        assert fwd(*args, *good, None) == E_NULL
        assert bwd(*args, *good, None) == E_NULL
    # a dimension <= 0, or H or W below 3
    bad = [(0, 1, 3, 64, 64), (1, 0, 3, 64, 64), (1, 1, 0, 64, 64), (1, 1, 3, 0, 64), (1, 1, 3, 64, -1), (-2, 1, 3, 64, 64),
           (1, 1, 3, 2, 64), (1, 1, 3, 64, 2), (1, 1, 1, 2, 2)]
    for dims in bad:
        assert fwd(A, B, C, D, *dims, None) == E_SHAPE
        assert bwd(A, B, C, D, *dims, None) == E_SHAPE
        assert size(*dims) == E_SHAPE
    for dims in ((1, 1, 3, 3, 3), (1, 1, 1, 3, 3), (2, 3, 3, 7, 9), (65535, 1, 1, 3, 3), (1, 65535, 3, 3, 3)):
        assert size(*dims) > 0 and size(*dims) % 16 == 0
    # the channel count
    for ch in (2, 4, 6):
        dims = (1, 1, ch, 64, 64)
        assert fwd(A, B, C, D, *dims, None) == E_UNSUPPORTED
        assert bwd(A, B, C, D, *dims, None) == E_UNSUPPORTED
        assert size(*dims) == E_UNSUPPORTED
    # an output that is an operand or the other output
    for args in ((A, B, A, D), (A, B, B, D), (A, B, C, A), (A, B, C, B), (A, B, C, C)):
        assert fwd(*args, *good, None) == E_UNSUPPORTED
    for args in ((A, B, C, A), (A, B, C, B), (A, B, C, C)):
        assert bwd(*args, *good, None) == E_UNSUPPORTED
    # a float pointer that is not 4-byte aligned, a scratch that is not 8-byte aligned; 4 and 8 bytes off a 16-byte boundary are fine
    # for the floats (those calls would launch: not made here)
    for k in range(4):
        for off in (1, 2, 3):
            args = [A, B, C, D]
            args[k] += off
            assert fwd(*args, *good, None) == E_UNSUPPORTED
            assert bwd(*args, *good, None) == E_UNSUPPORTED
    assert fwd(A, B, C, D + 4, *good, None) == E_UNSUPPORTED
    # the limits of the SSIM entries: rows * n <= 65535, H * W < 2^31
    for dims in ((1, 1, 3, 65536, 65536), (1, 1, 3, 32768, 65536), (65536, 1, 3, 64, 64), (1, 65536, 3, 64, 64), (256, 256, 1, 64, 64)):
        assert fwd(A, B, C, D, *dims, None) == E_TOOBIG
        assert bwd(A, B, C, D, *dims, None) == E_TOOBIG
        assert size(*dims) == E_TOOBIG
    assert lib.savfi_ssim_scratch_floats(1, 3, 65536, 65536) == E_TOOBIG and lib.savfi_ssim_scratch_floats(65536, 1, 64, 64) == E_TOOBIG
    assert size(1, 1, 3, 32768, 65535) > 0          # H * W = 2^31 - 32768
    # the order
    assert fwd(None, B, C, D, 1, 1, 2, 2, 65536, None) == E_NULL
    assert fwd(A, B, C, D, 1, 1, 2, 2, 65536, None) == E_SHAPE
    assert fwd(A, B, A, D, 1, 1, 3, 2, 65536, None) == E_SHAPE
    assert fwd(A, B, C, D, 1, 1, 2, 65536, 65536, None) == E_UNSUPPORTED
    assert fwd(A, B, A, D, 1, 1, 3, 65536, 65536, None) == E_UNSUPPORTED
    assert fwd(A + 2, B, C, D, 1, 1, 3, 65536, 65536, None) == E_UNSUPPORTED
    assert fwd(A, B, C, D, 1, 1, 3, 65536, 65536, None) == E_TOOBIG
    assert bwd(A, B, None, D, 1, 1, 2, 2, 65536, None) == E_NULL
    assert bwd(A, B, C, D, 65536, 1, 2, 2, 64, None) == E_SHAPE
    assert bwd(A, B, C, A, 65536, 1, 3, 64, 64, None) == E_UNSUPPORTED
    assert bwd(A, B, C, D, 65536, 1, 3, 64, 64, None) == E_TOOBIG
    assert size(65536, 1, 2, 2, 64) == E_SHAPE and size(65536, 1, 2, 64, 64) == E_UNSUPPORTED


def test_scratch_query_by_hand():
    """One double per workgroup of the tiling of every sample into tiles of 8 rows x 32 columns, rows * n * ceil(H / 8) * ceil(W / 32)
    of them, the total rounded up to a multiple of 16 bytes."""
    size = _hip.lib().savfi_census_scratch_bytes
    # 1 x 1 sample of 3 x 37 x 53: 5 x 2 workgroups -> 10 doubles
    assert size(1, 1, 3, 37, 53) == 10 * 8 == 80
    # rows = 3, n = 1 at 40 x 300: 5 x 10 workgroups per sample -> 150 doubles
    assert size(3, 1, 3, 40, 300) == 150 * 8 == 1200
    # rows = 1, n = 3 at 64 x 64, C = 1: 8 x 2 per sample -> 48 doubles; the same for rows = 3, n = 1 and whatever C
    assert size(1, 3, 1, 64, 64) == size(3, 1, 3, 64, 64) == 384
    # an odd number of workgroups is rounded up: 3 x 3 -> 1 double -> 16 bytes; rows = 1, n = 3 at 7 x 9 -> 3 doubles -> 32 bytes
    assert size(1, 1, 3, 3, 3) == 16
    assert size(1, 3, 3, 7, 9) == 32
    # 65 x 33: 9 x 2 workgroups, rows = 2, n = 2 -> 72 doubles; 9 x 33 with rows = 1, n = 1: 2 x 2 -> 4
    assert size(2, 2, 3, 65, 33) == 72 * 8
    assert size(1, 1, 1, 9, 33) == 32
    # the training frame: 256 x 448 -> 32 x 14 = 448 workgroups
    assert size(1, 1, 3, 256, 448) == 448 * 8
