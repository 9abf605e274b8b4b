"""No GPU: the slice-writing forward of DAIN's adaptive warp is part of the C ABI (declared in include/savfi_hip.h among the entries added
under ABI 24, exported by the built library, bound by _hip.py) and --dain_task_modes exists and is off by default."""
import ctypes
import re

from meta_interpolation_amd import _hip
from meta_interpolation_amd.config import default_args, get_args

ENTRY = "savfi_filterinterp_fwd_slice_f32"


def test_header_lists_the_entry_under_abi_24():
    with open(_hip.HEADER_PATH) as fh:
        text = fh.read()
    head, sep, _ = text.partition("#define SAVFI_ABI_VERSION 24")
    assert sep, "the ABI version stays 24: adding an entry is no incompatible change"
    assert ENTRY in head, "the comment above SAVFI_ABI_VERSION lists every entry added without a version change"
    assert ENTRY in _hip.declared_symbols()
    proto = re.search(r"int\s+%s\s*\(([^;]*)\)\s*;" % ENTRY, text)
    assert proto is not None
    args = [a.strip() for a in proto.group(1).replace("\n", " ").split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ["in", "flow", "filt", "out", "B", "C", "H", "W", "filter_size", "C_total", "c_off",
                                                        "stream"]
    assert len(_hip._PROTOTYPES[ENTRY]) == len(args)


def test_library_exports_the_entry():
    handle = ctypes.CDLL(_hip.LIB_PATH)
    assert hasattr(handle, ENTRY)
    assert hasattr(handle, "savfi_filterinterp_fwd_f32")          # its sibling stays
    assert handle.savfi_version() == 24


def test_dain_task_modes_is_off_by_default():
    assert default_args().dain_task_modes == 0
    assert default_args(model='dain').dain_task_modes == 0
    assert get_args(['--model', 'dain', '--dain_task_modes', '1'])[0].dain_task_modes == 1
