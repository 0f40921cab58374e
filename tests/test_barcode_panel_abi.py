"""The barcode panel entry points exist at every layer that needs no device: declared in include/sarlacc_amd.h, bound in
sarlacc_amd._lib.PROTOTYPES (tests/test_abi_table.py holds the two together type by type), and reachable from the package."""
import ctypes as C

from sarlacc_amd import _lib, calls
from sarlacc_amd.resident import DeviceReads
from tests.abi_text import _header_decls

NAMES = ("sarlacc_barcode_panel", "sarlacc_dev_barcode_panel")


def test_declared_and_bound():
    decls = _header_decls()
    for name in NAMES:
        assert name in decls, name + " is not declared in the header"
        assert name in _lib.PROTOTYPES, name + " is not in the prototype table"
        assert decls[name][0] == "int" and _lib.PROTOTYPES[name][0] is C.c_int
    dev = decls["sarlacc_dev_barcode_panel"][1]
    assert dev[3:5] == [("int64_t", "n"), ("int32_t", "max_len")] and dev[-1] == ("void*", "stream")
    assert [p for p in dev if p[1] in ("barcodes", "barcode_off", "nbarcodes")] == \
        [("const char*", "barcodes"), ("const int64_t*", "barcode_off"), ("int", "nbarcodes")]
    host = decls["sarlacc_barcode_panel"][1]
    assert [p[1] for p in host[-4:]] == ["best", "score", "next", "all_scores"]


def test_python_entry_points():
    assert callable(calls.barcode_panel) and callable(DeviceReads.barcode_panel)
    chars, off, nb = calls._panel_args(["ACGT", "", b"TT"])
    assert nb == 3 and off.tolist() == [0, 4, 4, 6] and chars[:6].tobytes() == b"ACGTTT"
    chars, off, nb = calls._panel_args([])
    assert nb == 0 and off.tolist() == [0] and chars.size >= 1
