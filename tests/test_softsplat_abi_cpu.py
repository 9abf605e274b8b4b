"""The C ABI of softmax splatting (csrc/softsplat.hip, added under ABI 24) as far as it can be exercised without a GPU: the exported
symbols, the version, the header's comment and documentation block, the prototypes, and the argument errors (validated before any
launch, in the order NULL, SHAPE, UNSUPPORTED, TOOBIG)."""
import re
import subprocess
from ctypes import c_int, c_void_p

from meta_interpolation_amd import _hip

NEW = ("savfi_softsplat_scratch_bytes", "savfi_softsplat_fwd_f32", "savfi_softsplat_bwd_f32")
E_NULL, E_SHAPE, E_UNSUPPORTED, E_TOOBIG = -1, -2, -3, -4
# non-null, 16-byte aligned "device pointers": never dereferenced, every call below returns before a launch
X, F, Z, O, HIT, DEN, MX, S, G, GX, GF, GZ = (0x10000 * k for k in range(1, 13))
GOOD = (1, 3, 64, 64)                # N, C, H, W
SUM, AVG, SOFT = 0, 1, 2
FWD = [X, F, Z, O, HIT, DEN, MX, S]
BWD = [X, F, Z, O, DEN, MX, G, GX, GF, GZ]


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
        assert re.search(r"\b%s\b" % name, comment.split("Added under 24", 1)[1]), name
    # the documentation block above the prototypes: the definition and the error order
    block = text[:text.index("int64_t savfi_softsplat_scratch_bytes(")].rsplit("/* ---", 1)[1]
    for word in ("csrc/softsplat.hip", "added\n * under ABI 24", "ONE fp32 addition", "floor", "TAKES PART", "on the factors", "expf(Z_p - M(q))",
                 "sum:", "avg:", "soft:", "linear", "hit = 0", "NaN", "g_x", "g_flow", "g_metric", "s_k", "never a memset", "No float atomics",
                 "SAVFI_E_NULL", "SAVFI_E_SHAPE", "SAVFI_E_UNSUPPORTED", "SAVFI_E_TOOBIG"):
        assert word in block, word
    assert block.index("SAVFI_E_NULL") < block.index("SAVFI_E_SHAPE") < block.index("SAVFI_E_UNSUPPORTED") < block.index("SAVFI_E_TOOBIG")
    assert _hip.SOFTSPLAT_MODES == {'sum': SUM, 'avg': AVG, 'soft': SOFT}


def test_prototypes_match_the_header():
    assert _hip._PROTOTYPES["savfi_softsplat_scratch_bytes"] == [c_int] * 4
    assert _hip._PROTOTYPES["savfi_softsplat_fwd_f32"] == [c_void_p] * 8 + [c_int] * 5 + [c_void_p]
    assert _hip._PROTOTYPES["savfi_softsplat_bwd_f32"] == [c_void_p] * 10 + [c_int] * 5 + [c_void_p]
    with open(_hip.HEADER_PATH) as fh:
        text = fh.read()
    fwd = re.search(r"int savfi_softsplat_fwd_f32\(([^;]*)\);", text).group(1)
    bwd = re.search(r"int savfi_softsplat_bwd_f32\(([^;]*)\);", text).group(1)
    names = lambda sig: [p.split()[-1].lstrip("*") for p in sig.replace("\n", " ").split(",")]
    assert names(fwd) == ["x", "flow", "metric", "out", "hit", "den", "mx", "scratch", "N", "C", "H", "W", "mode", "stream"]
    assert names(bwd) == ["x", "flow", "metric", "out", "den", "mx", "g_out", "g_x", "g_flow", "g_metric", "N", "C", "H", "W", "mode", "stream"]
    assert fwd.count("const float*") == 3 and bwd.count("const float*") == 7
    assert re.search(r"int64_t savfi_softsplat_scratch_bytes\(int N, int C, int H, int W\);", text)


def test_the_scratch_query_counts_the_accumulators_the_keys_and_the_words():
    q = _hip.lib().savfi_softsplat_scratch_bytes
    for N, C, H, W in ((1, 1, 4, 4), (2, 3, 7, 9), (1, 3, 33, 130), (2, 64, 8, 12), (1, 256, 1, 1)):
        want = N * (C + 1) * H * W * 8 + N * H * W * 4 + N * 8
        assert q(N, C, H, W) == (want + 15) // 16 * 16
    assert q(0, 3, 4, 4) == E_SHAPE and q(1, 3, 4, -1) == E_SHAPE
    assert q(1, 257, 4, 4) == E_UNSUPPORTED
    assert q(0, 257, 4, 4) == E_SHAPE
    assert q(1, 3, 65536, 32768) == E_TOOBIG and q(65536, 3, 4, 4) == E_TOOBIG and q(1, 256, 65536, 65535) == E_TOOBIG
    assert q(1, 257, 65536, 32768) == E_UNSUPPORTED


def test_argument_errors_come_before_any_launch():
    lib = _hip.lib()
    fwd, bwd = lib.savfi_softsplat_fwd_f32, lib.savfi_softsplat_bwd_f32
    # a required pointer is NULL; the metric may be NULL outside soft mode (those calls would launch and are not made here)
    for k in (0, 1, 3, 4, 5, 6, 7):
        args = list(FWD)
        args[k] = None
        for mode in (SUM, AVG, SOFT):
            assert fwd(*args, *GOOD, mode, None) == E_NULL
    for k in (0, 1, 3, 4, 5, 6):
        args = list(BWD)
        args[k] = None
        for mode in (SUM, AVG, SOFT):
            assert bwd(*args, *GOOD, mode, None) == E_NULL
    # in bwd each gradient may be NULL, but not all three
    assert bwd(*BWD[:7], None, None, None, *GOOD, SOFT, None) == E_NULL
    # a dimension <= 0
    for k in range(4):
        for v in (0, -1):
            dims = list(GOOD)
            dims[k] = v
            assert fwd(*FWD, *dims, SOFT, None) == E_SHAPE
            assert bwd(*BWD, *dims, SOFT, None) == E_SHAPE
            assert bwd(*BWD[:7], None, GF, None, *dims, AVG, None) == E_SHAPE
    # C above 256; an unknown mode; soft mode without a metric
    assert fwd(*FWD, 1, 257, 64, 64, SOFT, None) == E_UNSUPPORTED and bwd(*BWD, 1, 257, 64, 64, SOFT, None) == E_UNSUPPORTED
    for mode in (-1, 3, 7):
        assert fwd(*FWD, *GOOD, mode, None) == E_UNSUPPORTED and bwd(*BWD, *GOOD, mode, None) == E_UNSUPPORTED
    assert fwd(X, F, None, O, HIT, DEN, MX, S, *GOOD, SOFT, None) == E_UNSUPPORTED
    assert bwd(X, F, None, O, DEN, MX, G, GX, GF, GZ, *GOOD, SOFT, None) == E_UNSUPPORTED
    # an output equal to an operand or to another output
    for k in (3, 4, 5, 6):
        for alias in (X, F, Z, S) + tuple(FWD[3:k]):
            args = list(FWD)
            args[k] = alias
            assert fwd(*args, *GOOD, SOFT, None) == E_UNSUPPORTED
    for k in (7, 8, 9):
        for alias in tuple(BWD[:7]) + tuple(BWD[7:k]):
            args = list(BWD)
            args[k] = alias
            assert bwd(*args, *GOOD, SOFT, None) == E_UNSUPPORTED
    assert bwd(*BWD[:7], None, GF, GF, *GOOD, SOFT, None) == E_UNSUPPORTED
    # a float pointer that is not 4-byte aligned, a scratch that is not 8-byte aligned
    for off in (1, 2, 3):
        for k in range(8):
            args = list(FWD)
            args[k] += off
            assert fwd(*args, *GOOD, SOFT, None) == E_UNSUPPORTED
        for k in range(10):
            args = list(BWD)
            args[k] += off
            assert bwd(*args, *GOOD, SOFT, None) == E_UNSUPPORTED
    assert fwd(X, F, Z, O, HIT, DEN, MX, S + 4, *GOOD, SOFT, None) == E_UNSUPPORTED
    # H W > 2^31 - 1 - 256, N > 65535, N (C + 1) H W >= 2^40
    big = [(1, 3, 65536, 32768), (1, 1, 46341, 46341), (65536, 1, 4, 4), (1, 255, 65536, 65536), (8, 128, 32768, 32768)]
    for dims in big:
        assert fwd(*FWD, *dims, SOFT, None) == E_TOOBIG, dims
        assert bwd(*BWD, *dims, SOFT, None) == E_TOOBIG, dims
    # the order
    assert fwd(None, F, Z, O, HIT, DEN, MX, S, 0, 257, 64, 64, 9, None) == E_NULL
    assert fwd(X, F, Z, X, HIT, DEN, MX, S, 0, 257, 64, 64, 9, None) == E_SHAPE
    assert fwd(X, F, Z, X, HIT, DEN, MX, S, 1, 257, 65536, 65536, SOFT, None) == E_UNSUPPORTED
    assert fwd(X, F, Z, O, HIT, DEN, MX, S, 1, 3, 65536, 65536, 9, None) == E_UNSUPPORTED
    assert fwd(X, F, Z, X, HIT, DEN, MX, S, 1, 3, 65536, 65536, SOFT, None) == E_UNSUPPORTED
    assert fwd(X + 2, F, Z, O, HIT, DEN, MX, S, 1, 3, 65536, 65536, SOFT, None) == E_UNSUPPORTED
    assert fwd(X, F, Z, O, HIT, DEN, MX, S, 1, 3, 65536, 65536, SOFT, None) == E_TOOBIG
    assert bwd(X, F, Z, O, DEN, MX, None, GX, GF, GZ, 1, 3, 0, 64, SOFT, None) == E_NULL
    assert bwd(X, F, Z, O, DEN, MX, G, GX, GF, GX, 1, 3, 0, 64, SOFT, None) == E_SHAPE
    assert bwd(X, F, Z, O, DEN, MX, G, GX, GF, GX, 1, 3, 65536, 65536, SOFT, None) == E_UNSUPPORTED
    assert bwd(X, F, Z, O, DEN, MX, G, GX, GF, GZ, 1, 3, 65536, 65536, SOFT, None) == E_TOOBIG
