"""The ctypes prototypes of the Python binding (sarlacc_amd._lib.PROTOTYPES) are written by hand, so they are held
to include/sarlacc_amd.h as text: the same functions, and for each the declared return type and the declared type of
every parameter.  Needs neither the library nor a device."""
import ctypes as C
import os
import re

import pytest

from sarlacc_amd import _lib
from tests.abi_text import ROOT, _header_decls

SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "double": C.c_double}
# the `const char*` parameters that are NUL-terminated names; every other pointer is data of a stated length
NAMES = {("sarlacc_set_option", "name"), ("sarlacc_stage_ms", "name"), ("sarlacc_stage_count", "name")}


def _ctype(func, ctext, pname):
    if "*" in ctext:
        return C.c_char_p if (func, pname) in NAMES else _lib.Pointer
    return SCALARS[ctext]


def _restype(ctext):
    return dict(SCALARS, **{"void": None, "const char*": C.c_char_p})[ctext]   # (sarlacc_last_error returns a C string)


def mismatches(table):
    """Everything in which `table` departs from the header, as readable lines."""
    decls = _header_decls()
    bad = ["%s: in the table, not in the header" % n for n in sorted(set(table) - set(decls))]
    bad += ["%s: declared in the header, not in the table" % n for n in sorted(set(decls) - set(table))]
    for name in sorted(set(table) & set(decls)):
        ret, params = decls[name]
        restype, argtypes = table[name]
        if restype is not _restype(ret):
            bad.append("%s: returns %s, the table says %s" % (name, ret, restype))
        if len(argtypes) != len(params):
            bad.append("%s: %d parameters declared, %d in the table" % (name, len(params), len(argtypes)))
            continue
        bad += ["%s: parameter %d (%s %s) is %s in the table" % (name, k + 1, ctext, pname, got.__name__)
                for k, ((ctext, pname), got) in enumerate(zip(params, argtypes)) if got is not _ctype(name, ctext, pname)]
    return bad


def test_the_header_is_read_in_full():
    decls = _header_decls()
    assert len(decls) >= 58
    assert decls["sarlacc_version"] == ("int", []) and decls["sarlacc_release_workspace"] == ("void", [])
    assert decls["sarlacc_last_error"] == ("const char*", [])
    assert decls["sarlacc_dev_malloc"] == ("int", [("void**", "p"), ("int64_t", "bytes")])
    assert decls["sarlacc_dev_scramble"][1][3:5] == [("int64_t", "n"), ("uint64_t", "seed")]
    assert decls["sarlacc_dev_align"][1][3:5] == [("int64_t", "n"), ("int32_t", "max_len")]
    assert decls["sarlacc_dev_align"][1][-1] == ("void*", "stream")


def test_table_matches_the_header():
    assert mismatches(_lib.PROTOTYPES) == []


def test_the_comparison_bites():
    narrowed = dict(_lib.PROTOTYPES)
    restype, argtypes = narrowed["sarlacc_dev_fastq_format"]
    k = argtypes.index(C.c_int64)
    narrowed["sarlacc_dev_fastq_format"] = (restype, argtypes[:k] + [C.c_int] + argtypes[k + 1:])
    assert mismatches(narrowed) == ["sarlacc_dev_fastq_format: parameter %d (int64_t first_index) is c_int in the table" % (k + 1)]
    missing = dict(_lib.PROTOTYPES)
    del missing["sarlacc_dev_sam_extract"]
    assert mismatches(missing) == ["sarlacc_dev_sam_extract: declared in the header, not in the table"]
    extra = dict(_lib.PROTOTYPES, sarlacc_no_such_call=(C.c_int, []))
    assert mismatches(extra) == ["sarlacc_no_such_call: in the table, not in the header"]
    wrong_ret = dict(_lib.PROTOTYPES, sarlacc_release_umi_workspace=(C.c_int, []))
    assert len(mismatches(wrong_ret)) == 1
    short = dict(_lib.PROTOTYPES, sarlacc_set_device=(C.c_int, []))
    assert len(mismatches(short)) == 1


def test_every_call_of_the_package_is_in_the_table():
    pkg = os.path.join(ROOT, "sarlacc_amd")
    used = set()
    for f in sorted(os.listdir(pkg)):
        if f.endswith(".py"):
            used |= set(re.findall(r"\blib(?:\(\))?\.(sarlacc_\w+)", open(os.path.join(pkg, f)).read()))
    assert len(used) >= 50, "the scan no longer finds the package's calls"
    assert used <= set(_lib.PROTOTYPES), sorted(used - set(_lib.PROTOTYPES))


def test_every_table_name_resolves_in_the_library():
    """Loading the library initialises no device, so this runs wherever the library has been built."""
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libsarlacc_amd.so has not been built")
    so = _lib.lib()
    assert [n for n in _lib.PROTOTYPES if not hasattr(so, n)] == []
