"""The CPU restatement of BAM records -> reads (tests/bam_reads_cases.py) held against hand-written literals: the GPU
tests compare the device with the restatement, these compare the restatement with the SAM specification."""
import struct

import numpy as np

from tests import bam_cases as B
from tests import bam_reads_cases as RC

HEAD = B.header_bytes(b"@HD\tVN:1.6\tSO:unknown\n", [])


def rec(name, flag, text, quals, **kw):
    return RC.read_record(name, flag, RC.seq_codes(text), quals, **kw)


def test_packing_literal():
    assert RC.pack_seq(RC.seq_codes("ACGTN")) == bytes.fromhex("1248f0")
    r = rec(b"q", 4, "ACGTN", [0, 1, 2, 3, 93])
    assert r[-8:] == bytes.fromhex("1248f0") + bytes([0, 1, 2, 3, 93])
    assert RC.reads(HEAD + r) == ([b"q"], [b"ACGTN"], [b"!\"#$~"])


def test_reverse_literal():
    r = rec(b"rev", 16, "AACGN", [0, 1, 2, 3, 93])
    assert RC.reads(HEAD + r) == ([b"rev"], [b"NCGTT"], [b"~$#\"!"])
    even = rec(b"rev", 16, "AACGNT", [0, 1, 2, 3, 93, 40])
    assert RC.reads(HEAD + even) == ([b"rev"], [b"ANCGTT"], [b"I~$#\"!"])


def test_every_code_in_both_nibbles():
    assert [RC.LETTERS[RC.complement(c)] for c in range(16)] == list("=TGKCYSBAWRDMHVN")
    assert all(RC.complement(RC.complement(c)) == c for c in range(16))
    codes = list(range(1, 16)) * 2            # the second run starts at an odd base: every code in the low nibble too
    packed = RC.pack_seq(codes)
    assert {b >> 4 for b in packed} == set(range(1, 16)) and {b & 15 for b in packed[:15]} == set(range(1, 16))
    q = list(range(30))
    fwd = RC.read_record(b"f", 0, codes, q)
    rev = RC.read_record(b"r", 16, codes, q)
    assert RC.reads(HEAD + fwd + rev) == ([b"f", b"r"], [b"ACMGRSVTWYHKDBN" * 2, b"NVHMDRWABSYCKGT" * 2],
                                          [bytes(range(33, 63)), bytes(range(62, 32, -1))])


def test_missing_quality_marker():
    for flag in (0, 16):
        r = RC.read_record(b"m", flag, RC.seq_codes("ACG"), None)
        assert r[-3:] == b"\xff\xff\xff"
        assert RC.reads(HEAD + r)[2] == [b'"""']
        assert RC.reads(HEAD + r, missing_qual=40)[2] == [b"III"]
    # only the first byte is the marker: the rest is not looked at; 0xff anywhere else is a quality above 93
    assert RC.reads(HEAD + rec(b"m", 0, "ACG", [255, 0, 94]))[2] == [b'"""']
    assert RC.reads(HEAD + rec(b"m", 0, "ACG", [0, 255, 0])) == (1, RC.QUAL_HIGH)


def test_flags_names_and_empty_reads():
    recs = [rec(b"a", 0, "AC", [1, 2]), rec(b"b", 0x100, "ACG", [1, 2, 3]), rec(b"c", 0x800, "A", [1]), rec(b"d", 4, "", []),
            rec(b"e/1", 77, "T", [9]), rec(b"f", 0x910, "G", [9])]
    raw = HEAD + b"".join(recs)
    assert RC.reads(raw) == ([b"a", b"d", b"e/1"], [b"AC", b"", b"T"], [b"\"#", b"", b"*"])
    assert RC.reads(raw, exclude_flags=0)[0] == [b"a", b"b", b"c", b"d", b"e/1", b"f"]
    assert RC.reads(raw, exclude_flags=0)[1][5] == b"C"          # 0x910 holds 0x10
    assert RC.reads(raw, exclude_flags=4)[0] == [b"a", b"b", b"c", b"f"]


def test_each_error():
    good = rec(b"g", 0, "ACGT", [1, 2, 3, 4])
    eq = RC.read_record(b"x", 0, list(range(16)), [5] * 16)
    q94 = rec(b"x", 0, "ACGT", [1, 2, 94, 4])
    layout = B.raw_record(-1, -1, b"x!", 0, 0x900, [], 0)          # a name without its NUL, on a dropped record
    both = RC.read_record(b"x", 0, [1, 0], [1, 94])
    assert RC.reads(HEAD + good + eq + good) == (2, RC.SEQ_EQ)
    assert RC.reads(HEAD + good + good + q94) == (3, RC.QUAL_HIGH)
    assert RC.reads(HEAD + layout + q94) == (1, RC.LAYOUT)
    assert RC.reads(HEAD + both) == (1, RC.SEQ_EQ)                 # SEQ before QUAL
    assert RC.reads(HEAD + good + q94 + eq) == (2, RC.QUAL_HIGH)   # the lowest record wins
    # a bad SEQ or QUAL on a dropped record is no error
    dropped = RC.read_record(b"x", 0x100, [0, 0], [94, 94])
    assert RC.reads(HEAD + good + dropped + good)[0] == [b"g", b"g"]
    assert RC.reads(HEAD + good + dropped, exclude_flags=0) == (2, RC.SEQ_EQ)
    # an odd read's padding nibble is no base
    assert RC.reads(HEAD + rec(b"o", 0, "ACG", [1, 2, 3]))[1] == [b"ACG"]
    assert RC.reads(HEAD + good + struct.pack("<i", 31) + b"\0" * 31) == (2, RC.SIZE)
    assert RC.reads(HEAD + good + good[:20]) == (2, RC.CUT)
    assert RC.reads(HEAD + q94 + good[:2]) == (1, RC.QUAL_HIGH)


def test_random_reads_round_trip_through_the_sam_decoder():
    """The restatement against tests/bam_cases.bam_to_sam, the decoder the BAM -> ranges tests already trust."""
    rng = np.random.default_rng(1)
    recs = [RC.random_read(rng, int(n), 0, b"r%d" % i) for i, n in enumerate(rng.integers(0, 40, 30))]
    names, seqs, quals = RC.reads(HEAD + b"".join(recs))
    lines = [ln.split("\t") for ln in B.bam_to_sam(HEAD + b"".join(recs)).decode("latin-1").splitlines() if not ln.startswith("@")]
    assert [ln[0].encode() for ln in lines] == names
    assert [b"" if ln[9] == "*" else ln[9].encode() for ln in lines] == seqs
    assert [b"" if ln[10] == "*" else ln[10].encode("latin-1") for ln in lines] == quals
