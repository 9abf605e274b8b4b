"""The C ABI of the Laplacian-pyramid loss (csrc/laploss.hip, added under ABI 24) as far as it can be exercised without a GPU: the
exported symbols, the version, the argument errors (validated before any launch, in the order NULL, SHAPE, UNSUPPORTED, TOOBIG) and
the scratch query against the layout include/savfi_hip.h documents."""
import re
import subprocess

from meta_interpolation_amd import _hip

NEW = ("savfi_laploss_scratch_bytes", "savfi_laploss_f32", "savfi_laploss_bwd_f32")
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
    fwd, bwd, size = lib.savfi_laploss_f32, lib.savfi_laploss_bwd_f32, lib.savfi_laploss_scratch_bytes
    for k in range(4):
        args = [P] * 4
        args[k] = None
        assert fwd(*args, 1, 3, 64, 64, 5, None) == E_NULL
    for k in range(5):
        args = [P] * 5
        args[k] = None
        assert bwd(*args, 1, 3, 64, 64, 5, None) == E_NULL
    # every filtered level needs both sides >= 3: 17 for five levels, 9 for four, 5 for three, 3 for two
    bad = [((1, 3, 16, 64), 5), ((1, 3, 64, 16), 5), ((1, 3, 8, 9), 4), ((1, 3, 5, 4), 3), ((1, 3, 2, 3), 2), ((0, 3, 64, 64), 5),
           ((1, 0, 64, 64), 5), ((1, 3, 0, 64), 5), ((1, 3, 64, -1), 5)]
    for dims, levels in bad:
        assert fwd(P, P, P, P, *dims, levels, None) == E_SHAPE
        assert bwd(P, P, P, P, P, *dims, levels, None) == E_SHAPE
        assert size(*dims, levels) == E_SHAPE
    for dims, levels in (((1, 3, 17, 17), 5), ((1, 3, 9, 9), 4), ((1, 3, 5, 5), 3), ((1, 3, 3, 3), 2), ((2, 3, 7, 9), 3)):
        assert size(*dims, levels) > 0
    for levels in (-1, 0, 1, 6):
        assert fwd(P, P, P, P, 1, 3, 64, 64, levels, None) == E_UNSUPPORTED
        assert bwd(P, P, P, P, P, 1, 3, 64, 64, levels, None) == E_UNSUPPORTED
        assert size(1, 3, 64, 64, levels) == E_UNSUPPORTED
    for dims in ((1, 3, 65536, 65536), (65536, 1, 64, 64), (2, 32768, 64, 64)):      # the limits of the SSIM entries
        assert fwd(P, P, P, P, *dims, 5, None) == E_TOOBIG
        assert bwd(P, P, P, P, P, *dims, 5, None) == E_TOOBIG
        assert size(*dims, 5) == E_TOOBIG
        assert lib.savfi_ssim_scratch_floats(*dims) == E_TOOBIG
    # the order
    assert fwd(None, P, P, P, 1, 3, 16, 64, 9, None) == E_NULL
    assert fwd(P, P, P, P, 1, 3, 16, 64, 9, None) == E_SHAPE
    assert fwd(P, P, P, P, 1, 3, 65536, 65536, 9, None) == E_UNSUPPORTED
    assert fwd(P, P, P, P, 1, 3, 65536, 65536, 5, None) == E_TOOBIG
    assert bwd(P, P, None, P, P, 1, 3, 16, 64, 9, None) == E_NULL
    assert bwd(P, P, P, P, P, 1, 3, 65536, 65536, 9, None) == E_UNSUPPORTED


def test_scratch_query_by_hand():
    """32-bit words, every region rounded up to four, P = rows * C planes: c_s for s = 1..L-1 (P H_s W_s each), g_{c_s} for s = 1..L-2
    (the same sizes), then one double = two words per workgroup of the 32 x 32 tiling of the levels 0..L-2."""
    size = _hip.lib().savfi_laploss_scratch_bytes
    # 1 x 3 x 17 x 17, five levels: sides 17 9 5 3 2 -> planes of 81 25 9 4 elements, one workgroup per plane on every level
    c = 244 + 76 + 28 + 12                        # 243, 75, 27, 12 rounded up to four
    g = 244 + 76 + 28
    partial = 4 * 8                               # 3 doubles = 6 words -> 8, four filtered levels
    assert size(1, 3, 17, 17, 5) == 4 * (c + g + partial) == 2960
    # 2 x 3 x 37 x 53, five levels: 37x53 19x27 10x14 5x7 3x4 -> planes of 513 140 35 12; workgroups per plane 2x2 1 1 1
    c = 3080 + 6 * 140 + 212 + 6 * 12             # 6 * 513 = 3078 -> 3080, 6 * 35 = 210 -> 212
    g = 3080 + 6 * 140 + 212
    partial = 2 * 6 * 4 + 3 * (2 * 6)
    assert size(2, 3, 37, 53, 5) == 4 * (c + g + partial) == 33680
    # fewer levels: 1 x 1 x 7 x 9 with three (7x9 4x5 2x3) and 9 x 7 with two
    assert size(1, 1, 7, 9, 3) == 4 * ((20 + 8) + 20 + 2 * 4)
    assert size(1, 1, 9, 7, 2) == 4 * (20 + 0 + 4)
