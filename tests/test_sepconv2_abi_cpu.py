"""The C ABI of SepConv's second backward (csrc/sepconv_bwd2.hip, added under ABI 24) as far as it can be exercised without a GPU: the
exported symbol, the version, and the argument errors -- validated before any launch, in the order NULL, SHAPE, UNSUPPORTED, TOOBIG."""
import re
import subprocess

from meta_interpolation_amd import _hip

NAME = "savfi_sepconv_bwd2_f32"
E_NULL, E_SHAPE, E_UNSUPPORTED, E_TOOBIG = -1, -2, -3, -4
# distinct non-null, 16-byte aligned "device pointers": never dereferenced, every call below returns before a launch
IN, V, H, GO, GGV, GGH, DGO, DV, DH = (0x10000 * (k + 1) for k in range(9))
DIMS = (1, 3, 8, 8, 51)


def _call(in_=IN, v=V, h=H, gO=GO, ggV=GGV, ggH=GGH, d_gO=DGO, dV=DV, dH=DH, dims=DIMS):
    return _hip.lib().savfi_sepconv_bwd2_f32(in_, v, h, gO, ggV, ggH, d_gO, dV, dH, *dims, None)


def test_library_exports_the_symbol_under_abi_24():
    lib = _hip.lib()
    assert lib.savfi_version() == 24 and _hip.ABI_VERSION == 24
    assert NAME in _hip.declared_symbols() and NAME in _hip._PROTOTYPES
    assert len(_hip._PROTOTYPES[NAME]) == 15
    assert getattr(lib, NAME) is not None
    dyn = subprocess.run(["nm", "-D", "--defined-only", _hip.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert NAME in {line.split()[-1] for line in dyn.splitlines() if line.strip()}
    with open(_hip.HEADER_PATH) as fh:
        text = fh.read()
    comment = text[:text.index("#define SAVFI_ABI_VERSION 24")].rsplit("/*", 1)[1]
    assert "Added under 24" in comment and re.search(r"\b%s\b" % NAME, comment)


def test_null_rules():
    for k in ("in_", "v", "h", "gO"):
        assert _call(**{k: None}) == E_NULL, k
    assert _call(ggV=None, ggH=None) == E_NULL                        # no cotangent
    assert _call(d_gO=None, dV=None, dH=None) == E_NULL               # no output
    assert _call(ggV=None) == E_NULL                                  # dH without ggV
    assert _call(ggH=None) == E_NULL                                  # dV without ggH
    assert _call(ggV=None, d_gO=None, dV=None) == E_NULL              # ... also when it is the only output
    assert _call(ggH=None, d_gO=None, dH=None) == E_NULL


def test_shape_unsupported_toobig():
    for dims in ((0, 3, 8, 8, 51), (1, 0, 8, 8, 51), (1, 3, 0, 8, 51), (1, 3, 8, -1, 51), (1, 3, 8, 8, 0)):
        assert _call(dims=dims) == E_SHAPE, dims
    # an output that is an operand or another output; a pointer that is not a float's
    assert _call(d_gO=GO) == E_UNSUPPORTED
    assert _call(dV=V) == E_UNSUPPORTED
    assert _call(dH=GGV) == E_UNSUPPORTED
    assert _call(dV=DH) == E_UNSUPPORTED
    assert _call(v=V + 2) == E_UNSUPPORTED
    assert _call(dH=DH + 1) == E_UNSUPPORTED
    # the limits of savfi_sepconv_bwd_f32
    for dims in ((65536, 1, 4, 4, 1), (2000, 3, 4, 4, 51), (30000, 3, 4, 4, 1), (1, 3, 65536, 4, 3), (1, 3, 1 << 20, 1 << 20, 1)):
        assert _call(dims=dims) == E_TOOBIG, dims
        assert _hip.lib().savfi_sepconv_bwd_f32(IN, V, H, GO, None, DV, DH, *dims, None) == E_TOOBIG, dims


def test_the_order_of_the_checks():
    assert _call(in_=None, d_gO=GO, dims=(1, 3, 0, 8, 51)) == E_NULL
    assert _call(ggH=None, d_gO=GO, dims=(1, 3, 0, 8, 51)) == E_NULL          # (dV asked for without ggH)
    assert _call(d_gO=GO, dims=(1, 3, 0, 8, 51)) == E_SHAPE
    assert _call(d_gO=GO, dims=(65536, 1, 4, 4, 1)) == E_UNSUPPORTED
    assert _call(dims=(65536, 1, 4, 4, 1)) == E_TOOBIG
