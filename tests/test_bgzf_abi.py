"""The BGZF entry points exist at every layer that needs no device: declared in include/sarlacc_amd.h, bound in
sarlacc_amd._lib.PROTOTYPES (tests/test_abi_table.py holds the two together type by type), exported by the library when
it has been built, and reachable from the package."""
import ctypes as C
import os

import pytest

from sarlacc_amd import _lib, bgzf
from sarlacc_amd.resident import DeviceReads
from tests.abi_text import _header_decls

NAMES = ("sarlacc_bgzf_scan", "sarlacc_dev_bgzf_inflate", "sarlacc_dev_copy", "sarlacc_dev_rfind_byte")


def test_declared_and_bound():
    decls = _header_decls()
    for name in NAMES:
        assert name in decls, name + " is not declared in the header"
        assert name in _lib.PROTOTYPES, name + " is not in the prototype table"
        assert decls[name][0] == "int" and _lib.PROTOTYPES[name][0] is C.c_int
    assert decls["sarlacc_dev_bgzf_inflate"][1] == [
        ("const uint8_t*", "d_comp"), ("const int64_t*", "d_comp_off"), ("const int64_t*", "d_text_off"), ("int64_t", "n_blocks"),
        ("int64_t", "first_block"), ("uint8_t*", "d_text"), ("int", "check_crc"), ("void*", "stream")]
    scan = decls["sarlacc_bgzf_scan"][1]
    assert scan[:4] == [("const uint8_t*", "buf"), ("int64_t", "nbytes"), ("int64_t", "max_blocks"), ("int64_t", "first_block")]
    assert [p[1] for p in scan[4:]] == ["comp_off", "text_off", "n_blocks", "used_bytes", "last_is_eof"]
    assert all("stream" != p[1] for p in scan), "the scan needs no device"


def test_exported_by_the_library():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libsarlacc_amd.so has not been built")
    so = _lib.lib()
    assert [n for n in NAMES if not hasattr(so, n)] == []


def test_python_entry_points():
    assert callable(bgzf.sniff) and callable(bgzf.scan) and callable(bgzf.DeviceTextStream)
    assert callable(DeviceReads._stream_bgzf)
    assert bgzf.sniff_bytes(b"@r\n") == bgzf.TEXT and bgzf.sniff_bytes(b"\x1f\x8b\x08\x08") == bgzf.GZIP
