"""The CPU restatement of the BAM writer (tests/bam_write_cases.py) held against the CPU restatement of the BAM reader
(tests/bam_reads_cases.reads) and against one record written out by hand.  No device and no library needed."""
import numpy as np
import pytest

from tests import bam_reads_cases as Rd
from tests import bam_write_cases as Bw
from tests import bgzf_write_cases as W

# name "r1" (its comment cut), ACGTN, qualities 0, 10, 20, 40, 93
BY_HAND = bytes.fromhex(
    "2b000000"                  # block_size 43
    "ffffffff" "ffffffff"       # refID -1, pos -1
    "03" "00" "4812"            # l_read_name 3, mapq 0, bin 4680
    "0000" "0400"               # n_cigar_op 0, flag 4
    "05000000"                  # l_seq 5
    "ffffffff" "ffffffff"       # next_refID -1, next_pos -1
    "00000000"                  # tlen 0
    "723100"                    # r1 NUL
    "1248f0"                    # A C | G T | N -
    "000a14285d")


def test_one_record_by_hand():
    assert Bw.expected_records([b"r1 extra"], [b"ACGTN"], [b"!+5I~"]) == BY_HAND
    off, cuts = Bw.layout([b"r1 extra"], [b"ACGTN"], [b"!+5I~"])
    assert off.tolist() == [0, 47] and cuts.tolist() == [39, 42]
    assert Bw.expected_records(None, [b"ACGTN"], [b"!+5I~"], first_index=7)[36:43] == b"READ_7\0"


def test_the_name_rule():
    assert Bw.qname(b"read_1 ch=3") == b"read_1" and Bw.qname(b"a\tb c") == b"a" and Bw.qname(b"whole") == b"whole"
    assert Bw.qname(b"") == b"*" and Bw.qname(b" x") == b"*" and Bw.qname(b"\t") == b"*"


@pytest.mark.parametrize("name", sorted(Bw.BATCHES))
def test_round_trip_through_the_reader(name):
    names, seqs, quals = Bw.BATCHES[name]()
    raw = Bw.header_bytes() + Bw.expected_records(names, seqs, quals)
    got = Rd.reads(raw, exclude_flags=0)
    assert got[0] == [Bw.qname(n) for n in names]
    assert got[1] == seqs and got[2] == quals
    off, cuts = Bw.layout(names, seqs, quals)
    assert off[-1] == len(raw) - len(Bw.header_bytes())
    assert (np.diff(cuts) >= 0).all() and (cuts[1::2] - cuts[0::2] == [(len(s) + 1) // 2 for s in seqs]).all()
    assert (off[1:] - cuts[1::2] == [len(s) for s in seqs]).all()


def test_the_batches_hold_what_the_issue_lists():
    names, seqs, quals = Bw.batch_lengths()
    assert set(Bw.LENGTHS) <= {len(s) for s in seqs}
    assert set(b"".join(seqs)) == set(Bw.BASES) and {33, 126} <= set(b"".join(quals))
    assert {1, 254} <= {len(Bw.kept(n)) for n in names} and b"" in names and any(b" " in n for n in names)
    tiny = Bw.layout(*Bw.batch_tiny())[0]
    assert np.diff(np.searchsorted(tiny, np.arange(0, tiny[-1], 4096))).max() > 64
    span = Bw.layout(*Bw.batch_span())[0]
    assert np.diff(span).max() > 3 * 4096 + 4096
    assert 0 in [len(s) for s in Bw.batch_file()[1]] and len(Bw.batch_file()[1]) == 60


def test_refusals():
    ok = (b"n", b"ACGT", b"IIII")
    assert Bw.refusal(*ok) is None and Bw.refusal(None, b"", b"") is None
    assert Bw.refusal(b"n" * 255, *ok[1:]) == Bw.NAME_LONG and Bw.refusal(b"n" * 254, *ok[1:]) is None
    assert Bw.refusal(b"n" * 10 + b" " + b"c" * 289, *ok[1:]) is None
    assert Bw.refusal(b"a\x01b c", *ok[1:]) == Bw.NAME_BYTE and Bw.refusal(b"ab \x01", *ok[1:]) is None
    assert Bw.refusal(b"a\x7fb", *ok[1:]) == Bw.NAME_BYTE
    for base in (b"=", b"a", b"-", b"\0", b"@", b"Z"):
        assert Bw.refusal(b"n", b"AC" + base + b"T", b"IIII") == Bw.BASE
    assert Bw.refusal(b"n", b"ACGT", b"II I") == Bw.QUAL and Bw.refusal(b"n", b"ACGT", b"II\x7fI") == Bw.QUAL
    assert Bw.refusal(b"a\x01", b"a", b" ") == Bw.NAME_BYTE and Bw.refusal(b"a", b"a", b" ") == Bw.BASE
    assert Bw.first_refusal([b"a", b"b\x01", b"c"], [b"A", b"A", b"x"], [b"I", b"I", b"I"]) == (2, Bw.NAME_BYTE)
    assert Bw.first_refusal(None, [b"A", b"A"], [b"I", b"I"]) is None


def test_header_bytes():
    assert Bw.header_bytes() == b"BAM\1" + (23).to_bytes(4, "little") + b"@HD\tVN:1.6\tSO:unsorted\n" + bytes(4)
    assert Bw.header_bytes(b"") == b"BAM\1" + bytes(8)


@pytest.mark.parametrize("L", [100, 2000])
def test_the_synthetic_stream_is_what_the_helper_writes(L):
    raw, cuts = Bw.synth_records(20000, L, 5)
    names, seqs, quals = Rd.reads(Bw.header_bytes() + raw, exclude_flags=0)
    assert names[:2] == [b"read_0000000", b"read_0000001"] and {len(s) for s in seqs} == {L}
    assert set(b"".join(seqs)) == set(b"ACGT")
    assert Bw.expected_records(names, seqs, quals) == raw
    assert np.array_equal(Bw.layout(names, seqs, quals)[1], cuts)


def test_piece_ends():
    assert Bw.piece_ends([0, 10, 64, 70, 127, 128, 500, 510, 1000, 1200], 1000) == [64, 128, 500, 1000]
    assert Bw.piece_ends([1100, 1200, 2500], 1000, origin=1000) == [100, 200, 1000]
    assert Bw.piece_ends([], 77) == [77]


def test_yardsticks_of_the_record_stream():
    """zlib on the host, the figures the bounds of the device tests rest on: a Huffman table per field pays at 2 000
    bases (it beats level 6) and does not at 100."""
    long_, short = Bw.yardsticks(2000), Bw.yardsticks(100)
    print("2 000 bases: level 6 %d, Huffman-only %d, per field %d (%.3f of level 6)"
          % (long_["level6"], long_["huffman"], long_["per_field"], long_["per_field"] / long_["level6"]))
    print("100 bases: level 6 %d, Huffman-only %d, per field %d (%.3f of level 6)"
          % (short["level6"], short["huffman"], short["per_field"], short["per_field"] / short["level6"]))
    assert long_["per_field"] * 1.004 < long_["level6"]
    assert short["per_field"] > short["huffman"] + 8 * Bw.TABLE_ROOM
    assert len(Bw.seeded_records(100)[0]) == 8 * W.BLOCK
