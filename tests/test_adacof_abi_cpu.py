"""The C ABI of AdaCoF's deformable-tap op (csrc/adacof.hip, added under ABI 24) as far as it can be exercised without a GPU: the exported
symbols, the version, the header's comment and documentation block, the prototypes, and the argument errors (validated before any
launch, in the order NULL, SHAPE, UNSUPPORTED, TOOBIG)."""
import re
import subprocess
from ctypes import c_int, c_void_p

from meta_interpolation_amd import _hip

NEW = ("savfi_adacof_fwd_f32", "savfi_adacof_bwd_f32")
E_NULL, E_SHAPE, E_UNSUPPORTED, E_TOOBIG = -1, -2, -3, -4
# non-null, 16-byte aligned "device pointers": never dereferenced, every call below returns before a launch
X, W, A, B, O, GW, GA, GB = (0x10000 * k for k in range(1, 9))
GOOD = (1, 3, 64, 64, 5, 1)          # N, C, H, W, F, dilation


def test_library_exports_the_two_symbols_under_abi_24():
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
        assert re.search(r"\b%s\b" % name, comment.split("Added under 24", 1)[1]), name
    # the documentation block above the two prototypes: the definition and the error order
    block = text[:text.index("int savfi_adacof_fwd_f32(")].rsplit("/* ---", 1)[1]
    for word in ("csrc/adacof.hip", "added under ABI 24", "floor", "border replicate", "SAVFI_E_NULL", "SAVFI_E_SHAPE", "SAVFI_E_UNSUPPORTED",
                 "SAVFI_E_TOOBIG", "g_w", "g_a", "g_b", "NaN"):
        assert word in block, word
    assert block.index("SAVFI_E_NULL") < block.index("SAVFI_E_SHAPE") < block.index("SAVFI_E_UNSUPPORTED") < block.index("SAVFI_E_TOOBIG")


def test_prototypes_match_the_header():
    assert _hip._PROTOTYPES["savfi_adacof_fwd_f32"] == [c_void_p] * 5 + [c_int] * 6 + [c_void_p]
    assert _hip._PROTOTYPES["savfi_adacof_bwd_f32"] == [c_void_p] * 8 + [c_int] * 6 + [c_void_p]
    with open(_hip.HEADER_PATH) as fh:
        text = fh.read()
    fwd = re.search(r"int savfi_adacof_fwd_f32\(([^;]*)\);", text).group(1)
    bwd = re.search(r"int savfi_adacof_bwd_f32\(([^;]*)\);", text).group(1)
    names = lambda sig: [p.split()[-1].lstrip("*") for p in sig.replace("\n", " ").split(",")]
    assert names(fwd) == ["x", "w", "a", "b", "out", "N", "C", "H", "W", "F", "dilation", "stream"]
    assert names(bwd) == ["x", "w", "a", "b", "g_out", "g_w", "g_a", "g_b", "N", "C", "H", "W", "F", "dilation", "stream"]
    assert fwd.count("const float*") == 4 and bwd.count("const float*") == 5


def test_argument_errors_come_before_any_launch():
    lib = _hip.lib()
    fwd, bwd = lib.savfi_adacof_fwd_f32, lib.savfi_adacof_bwd_f32
    # a required pointer is NULL; in bwd each gradient may be NULL, but not all three
    for k in range(5):
        args = [X, W, A, B, O]
        args[k] = None
        assert fwd(*args, *GOOD, None) == E_NULL
        args = [X, W, A, B, O, GW, GA, GB]
        args[k] = None
        assert bwd(*args, *GOOD, None) == E_NULL
    assert bwd(X, W, A, B, O, None, None, None, *GOOD, None) == E_NULL
    # a dimension <= 0
    for k in range(6):
        for v in (0, -1):
            dims = list(GOOD)
            dims[k] = v
            assert fwd(X, W, A, B, O, *dims, None) == E_SHAPE
            assert bwd(X, W, A, B, O, GW, GA, GB, *dims, None) == E_SHAPE
            assert bwd(X, W, A, B, O, None, GA, None, *dims, None) == E_SHAPE
    # C not 1 or 3; F even or above 11; dilation above 8
    bad = [(1, 2, 64, 64, 5, 1), (1, 4, 64, 64, 5, 1), (1, 3, 64, 64, 2, 1), (1, 3, 64, 64, 4, 1), (1, 3, 64, 64, 12, 1), (1, 3, 64, 64, 13, 1),
           (1, 3, 64, 64, 5, 9), (1, 1, 64, 64, 10, 8)]
    for dims in bad:
        assert fwd(X, W, A, B, O, *dims, None) == E_UNSUPPORTED
        assert bwd(X, W, A, B, O, GW, GA, GB, *dims, None) == E_UNSUPPORTED
    # an output equal to an operand or to another output
    for alias in (X, W, A, B):
        assert fwd(X, W, A, B, alias, *GOOD, None) == E_UNSUPPORTED
    for alias in (X, W, A, B, O):
        for k in (5, 6, 7):
            args = [X, W, A, B, O, GW, GA, GB]
            args[k] = alias
            assert bwd(*args, *GOOD, None) == E_UNSUPPORTED
    for args in ((GW, GW, GB), (GW, GA, GW), (GW, GA, GA), (None, GA, GA)):
        assert bwd(X, W, A, B, O, *args, *GOOD, None) == E_UNSUPPORTED
    # a pointer that is not 4-byte aligned (4 bytes off a 16-byte boundary is fine: those calls would launch and are not made here)
    for off in (1, 2, 3):
        for k in range(5):
            args = [X, W, A, B, O]
            args[k] += off
            assert fwd(*args, *GOOD, None) == E_UNSUPPORTED
        for k in range(8):
            args = [X, W, A, B, O, GW, GA, GB]
            args[k] += off
            assert bwd(*args, *GOOD, None) == E_UNSUPPORTED
    # N F^2 H W or N C Hp Wp >= 2^31
    big = [(1, 3, 65536, 32768, 1, 1),            # F^2 H W = 2^31
           (1, 1, 46341, 46341, 1, 1),            # Hp Wp = 2147488281
           (1, 3, 32768, 32768, 1, 1),            # C Hp Wp = 3 * 2^30
           (2, 1, 32768, 32768, 1, 1),            # N Hp Wp = 2^31
           (1, 1, 9000, 9000, 7, 1),              # F^2 H W = 3.97e9
           (86, 3, 1024, 1024, 5, 1)]             # N F^2 H W = 2.25e9
    for dims in big:
        assert fwd(X, W, A, B, O, *dims, None) == E_TOOBIG, dims
        assert bwd(X, W, A, B, O, GW, GA, GB, *dims, None) == E_TOOBIG, dims
    # the order
    assert fwd(None, W, A, B, O, 0, 2, 64, 64, 4, 9, None) == E_NULL
    assert fwd(X, W, A, B, X, 0, 2, 64, 64, 4, 9, None) == E_SHAPE
    assert fwd(X + 1, W, A, B, X, 1, 2, 65536, 65536, 4, 9, None) == E_UNSUPPORTED
    assert fwd(X, W, A, B, X, 1, 3, 65536, 65536, 5, 1, None) == E_UNSUPPORTED
    assert fwd(X + 2, W, A, B, O, 1, 3, 65536, 65536, 5, 1, None) == E_UNSUPPORTED
    assert fwd(X, W, A, B, O, 1, 3, 65536, 65536, 5, 1, None) == E_TOOBIG
    assert bwd(X, W, A, B, None, GW, GA, GB, 1, 3, 0, 64, 5, 1, None) == E_NULL
    assert bwd(X, W, A, B, O, GW, GA, GW, 1, 3, 0, 64, 5, 1, None) == E_SHAPE
    assert bwd(X, W, A, B, O, GW, GA, GW, 1, 3, 65536, 65536, 5, 1, None) == E_UNSUPPORTED
    assert bwd(X, W, A, B, O, GW, GA, GB, 1, 3, 65536, 65536, 5, 1, None) == E_TOOBIG
