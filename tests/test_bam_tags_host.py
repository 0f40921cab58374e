"""tests/bam_tags_cases.py, the plain-Python restatement the GPU tests of the BAM tags compare with, pinned on ground it
does not hold itself: bytes written out by hand from the SAM specification (section 4.2.4), the independent decoder
tests.bam_cases._tags_text over random tag lists, and the argument checks of DeviceReads.tag / set_tag / drop_tags that
need no device."""
import struct

import numpy as np
import pytest

from tests import bam_cases as B
from tests import bam_tags_cases as T


# ---- bytes by hand -------------------------------------------------------------------------------------------------------

def test_literal_entries():
    assert B.encode_tag("NM:i:1") == b"NMC\x01"
    assert T.walk(b"NMC\x01") == [(b"NM", "C", 0, 3, 1, 4)]
    z = b"RGZrun1\0"
    assert B.encode_tag("RG:Z:run1") == z and T.walk(z) == [(b"RG", "Z", 0, 3, 4, 8)]
    h = b"xhH1AE301\0"
    assert B.encode_tag("xh:H:1AE301") == h and T.walk(h) == [(b"xh", "H", 0, 3, 6, 10)]
    a = b"tpAP"
    assert B.encode_tag("tp:A:P") == a and T.walk(a) == [(b"tp", "A", 0, 3, 1, 4)]
    bs = b"mvBs\x02\x00\x00\x00\x05\x00\xff\xff"       # B:s with the two entries 5 and -1
    assert B.encode_tag("mv:B:s,5,-1") == bs and T.walk(bs) == [(b"mv", "B", 0, 3, 9, 12)]
    empty = b"MLBC\x00\x00\x00\x00"
    assert B.encode_tag("ML:B:C") == empty and T.walk(empty) == [(b"ML", "B", 0, 3, 5, 8)]
    assert T.walk(b"") == []
    every = b"".join([b"NMC\x01", z, h, a, bs, empty, b"qsf\x00\x00\x80\x3f", b"nsi\xfe\xff\xff\xff", b"e0Z\0"])
    assert [e[:2] for e in T.walk(every)] == [(b"NM", "C"), (b"RG", "Z"), (b"xh", "H"), (b"tp", "A"), (b"mv", "B"), (b"ML", "B"),
                                             (b"qs", "f"), (b"ns", "i"), (b"e0", "Z")]
    assert T.find(every, b"mv") == (ord("B"), 4 + 8 + 10 + 4 + 3, 9, 26, 12)
    assert T.find(every, b"e0") == (ord("Z"), len(every) - 1, 0, len(every) - 4, 4)
    assert T.find(every, b"zz") == (0, 0, 0, 0, 0)
    assert T.int_values([every, b""], b"ns")[0].tolist() == [-2, 0]
    assert T.string_values([every, b""], b"tp")[0] == [b"P", b""]


def test_first_occurrence_wins():
    aux = b"RXZAAA\0" + b"NMC\x07" + b"RXZCC\0"
    assert T.find(aux, b"RX") == (ord("Z"), 3, 3, 0, 7)
    assert T.tags_refusal(aux) == "tag RX appears twice"
    assert T.drop_tag([aux], b"RX") == [b"NMC\x07"]
    assert T.set_tag([aux], b"RX", "Z", [b"G"]) == [b"NMC\x07" + b"RXZCC\0" + b"RXZG\0"]


@pytest.mark.parametrize("aux", [
    b"N", b"NM", b"NMC\x01X", b"NMC\x01XY",                      # fewer than 3 bytes left
    b"NMz\x01", b"NMa\x01\x02\x03\x04", b"NM\0\x01",              # a type letter outside AcCsSiIfZHB
    b"NMi\x01\x02\x03", b"NMs\x01", b"NMC", b"qsf\0\0\0",         # a fixed value past the end
    b"mvBc\x01\0\0", b"mvB", b"mvBc",                            # a B header past the end
    b"mvBc\x02\0\0\0\x01", b"mvBi\x01\0\0\0\x01\x02\x03", b"mvBc\xff\xff\xff\xff\x01",   # a B payload past the end
    b"mvBA\x01\0\0\0A", b"mvBZ\0\0\0\0", b"mvBd\0\0\0\0",          # a B subtype outside cCsSiIf
    b"RGZabc", b"RGZ", b"xhH12",                                 # no NUL in front of the end
])
def test_malformed(aux):
    with pytest.raises(T.Malformed):
        T.walk(aux)
    assert T.tags_refusal(aux) == T.MALFORMED and T.first_malformed([b"", b"NMC\x01", aux, aux]) == 3
    with pytest.raises(T.Malformed):
        T.walk(b"NMC\x01" + aux)


def test_splice_by_hand():
    areas = [b"NMC\x01RXZAC\0", b"", b"tpAP"]
    assert T.splice(areas, src=[2, 0, 0, 1]) == [b"tpAP", areas[0], areas[0], b""]
    assert T.splice(areas, cuts=[(4, 6), (0, 0), (0, 4)]) == [b"NMC\x01", b"", b""]
    assert T.splice(areas, tag=b"BC", kind="i", column=[-2, 0, 2 ** 31 - 1], mask=[True, False, True]) == \
        [areas[0] + b"BCi\xfe\xff\xff\xff", b"", b"tpAPBCi\xff\xff\xff\x7f"]
    assert T.set_tag(areas, b"RX", "Z", [b"GGGG", b"", b"T"]) == [b"NMC\x01RXZGGGG\0", b"RXZ\0", b"tpAPRXZT\0"]


def test_record_with_tags_by_hand():
    rec = T.record(b"r1", b"ACG", b"!+5", b"NMC\x01")
    assert rec == struct.pack("<i", 32 + 3 + 2 + 3 + 4) + struct.pack("<iiBBHHHiiii", -1, -1, 3, 0, 4680, 0, 4, 3, -1, -1, 0) + \
        b"r1\0" + b"\x12\x40" + b"\x00\x0a\x14" + b"NMC\x01"
    off, cuts = T.layout([b"r1", b"r2 comment"], [b"ACG", b""], [b"!+5", b""], [b"NMC\x01", b""])
    assert off.tolist() == [0, 48, 48 + 39] and cuts.tolist() == [39, 41, 44, 87, 87, 87]
    assert T.first_refusal([b"a", b"b"], [b"A", b"A"], [b" ", b"I"], [b"N", b"N"]) == (1, "quality byte outside Phred+33")
    assert T.first_refusal([b"a", b"b"], [b"A", b"A"], [b"I", b"I"], [b"", b"N"]) == (2, T.MALFORMED)


# ---- the independent decoder ---------------------------------------------------------------------------------------------

def test_agrees_with_the_decoder_over_random_tag_lists():
    rng = np.random.default_rng(5)
    seen = set()
    for _ in range(400):
        fields = T.random_fields(rng)
        aux = T.encode(fields)
        text, cg = B._tags_text(aux)
        assert cg is None and len(text) == len(fields)
        entries = T.walk(aux)
        assert [e[0].decode() for e in entries] == [f[:2] for f in fields] == [t[:2] for t in text]
        assert entries == [] or (entries[0][2] == 0 and entries[-1][5] == len(aux))
        assert all(a[5] == b[2] for a, b in zip(entries, entries[1:]))
        for (tag, ty, at, v, vlen, nxt), t in zip(entries, text):
            seen.add(ty)
            assert T.find(aux, tag) == (ord(ty), v, vlen, at, nxt - at)      # the tags of a list are distinct
            if ty in "ZH":
                assert aux[v:v + vlen].decode() == t[5:] and aux[v + vlen] == 0
            elif ty == "A":
                assert chr(aux[v]) == t[5:]
            elif ty in "cCsSiI":
                assert T.int_values([aux], tag)[0][0] == int(t[5:])
            elif ty == "B":
                assert struct.unpack_from("<I", aux, v + 1)[0] == len(t[5:].split(",")) - 1 and chr(aux[v]) == t[5]
        # every entry once more through the decoder, alone: the spans are those of whole entries
        assert [B._tags_text(aux[e[2]:e[5]])[0][0] for e in entries] == text
    assert seen == set("AcCsSiIfZHB")


def test_basecaller_like_tags_decode():
    aux = T.basecaller_aux(np.random.default_rng(6), 600, 3)
    text, _ = B._tags_text(aux)
    assert [t[:4] for t in text][-4:] == ["RG:Z", "mv:B", "MM:Z", "ML:B"] and T.tags_refusal(aux) is None
    assert T.find(aux, b"mv")[2] == 5 + 1 + 100


# ---- argument checks that need no device ----------------------------------------------------------------------------------

def _batch(n):
    from sarlacc_amd.resident import DeviceReads
    return DeviceReads(None, None, None, np.zeros(n + 1, np.int64), None)


@pytest.mark.parametrize("name", ["", "R", "RXX", "1X", "R_", "R ", b"R\0", None, 7, "é1"])
def test_tag_names(name):
    dev = _batch(2)
    for call in (lambda: dev.tag(name), lambda: dev.set_tag(name, ["a", "b"]), lambda: dev.drop_tags([name]), lambda: dev.drop_tags(["RX", name])):
        with pytest.raises(ValueError, match="tag name"):
            call()
    assert dev.tags is None


def test_tag_names_that_pass():
    from sarlacc_amd.tags import tag_name
    assert [tag_name(n) for n in ("RX", "a9", "Z0", b"mv")] == [b"RX", b"a9", b"Z0", b"mv"]
    dev = _batch(2)
    dev.drop_tags("MM")             # nothing to drop, nothing to launch
    dev.drop_tags(["MM", "ML"])
    assert dev.tags is None


def test_set_tag_values():
    from sarlacc_amd.strset import StringSet, StrList
    from sarlacc_amd.tags import tag_column
    dev = _batch(3)
    for values, what in ((["a", "b"], "2 tag values for 3 reads"), (["a", "b\x7f", "c"], "' '..'~'"), (["a", "\tb", "c"], "' '..'~'"),
                         (["a", "b", "\x1f"], "' '..'~'"), ([1, 2, 2 ** 31], "2\\^31"), ([-2 ** 31 - 1, 0, 0], "2\\^31"), ([1, 2], "2 tag values"),
                         ([1.5, 2.0, 3.0], "strings .* or integers"), ([True, False, True], "strings .* or integers"),
                         (["a", 1, "b"], "strings .* or integers"), (np.zeros((3, 1), np.int32), "strings .* or integers")):
        with pytest.raises(ValueError, match=what):
            dev.set_tag("RX", values)
    for present in ([True, False], [1, 0, 1], np.zeros((3, 1), bool)):
        with pytest.raises(ValueError, match="present"):
            dev.set_tag("RX", ["a", "b", "c"], present)
    assert dev.tags is None
    kind, data = tag_column(["a c", "", "~"], 3)
    assert kind == "Z" and data.to_strings() == ["a c", "", "~"]
    assert tag_column(StrList(["x", "y", "z"]), 3)[0] == "Z" and tag_column(StringSet.from_strings(["x", "y", "z"]), 3)[0] == "Z"
    kind, data = tag_column([-2 ** 31, 0, 2 ** 31 - 1], 3)
    assert kind == "i" and data.dtype == np.int32 and data.tolist() == [-2 ** 31, 0, 2 ** 31 - 1]
    assert tag_column(np.array([1, 2, 3], np.uint8), 3)[1].tolist() == [1, 2, 3]


def test_write_bam_tags_go_with_host_reads():
    from sarlacc_amd import generics as G
    with pytest.raises(ValueError, match="host Reads"):
        G.write_bam("/nonexistent/x.bam", _batch(1), tags={"RX": ["A"]})
