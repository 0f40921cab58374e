"""The host side of the BAM reader (sarlacc_amd/sam.py: read_bam_header, is_bam) and the self-check of the test
encoder (tests/bam_cases.py): SAM text -> BAM -> SAM text must mean the same to the restatement of R/sam2ranges.R.
Needs the library (the BGZF header walk), no device."""
import gzip
import json
import os
import struct

import numpy as np
import pytest

from tests import bam_cases as B
from tests import sam_restated as R
from tests.bgzf_cases import bgzf_compress

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = json.load(open(os.path.join(HERE, "golden", "sam2ranges_cases.json")))["cases"]


def outcome(text, minq, restricted):
    """What the restatement makes of SAM text: its table, or (record number, code) of its refusal."""
    try:
        return R.as_table(R.sam2ranges(text, minq, restricted))
    except R.SamError as e:
        return B.record_of_line(text, e.line), e.code


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_golden_cases_survive_the_round_trip(case):
    text = case["sam"].encode()
    raw = B.bam_bytes(text)
    if raw is None:
        # what BAM cannot hold: header errors, too few fields, non-numeric FLAG / MAPQ / POS, a CIGAR that is no CIGAR,
        # an op of 2^28 or more -- also on a dropped record (unmapped_any_cigar: POS 'x', CIGAR '?!')
        code = case["error"]["code"] if "error" in case else case["name"]
        assert code in ("sq_sn", "sq_ln", "sq_dup", "fields", "flag", "mapq", "pos", "cigar_syntax", "cigar_range", "unmapped_any_cigar")
        return
    assert outcome(B.bam_to_sam(raw), case["minq"], case["restricted"]) == outcome(text, case["minq"], case["restricted"])


def test_the_encoder_holds_most_golden_cases():
    held = [c["name"] for c in CASES if B.bam_bytes(c["sam"].encode()) is not None]
    assert len(held) >= 14 and {"err_rname", "err_cigar_star", "err_cigar_clips", "err_end", "literal_minq10"} <= set(held)


@pytest.mark.parametrize("minq,restricted", [(None, None), (10, None), (0, ["chr2", "chr5", "*"]), (60, [])])
def test_random_files_survive_the_round_trip(minq, restricted):
    text = B.sam_text(np.random.default_rng(7), 400)
    raw = B.bam_bytes(text)
    back = B.bam_to_sam(raw)
    expect = outcome(text, minq, restricted)
    assert outcome(back, minq, restricted) == expect
    if minq is None:
        assert len(expect["names"]) > 100
    assert B.bam_bytes(back) == B.bam_bytes(B.bam_to_sam(B.bam_bytes(back)))      # a fixed point after one trip


def test_long_cigar_goes_through_a_cg_tag():
    rng = np.random.default_rng(1)
    line = "long\t0\tchr1\t5\t60\t%s\t*\t0\t0\tACGTA\t*\tNM:i:1" % "".join("%d%s" % (a, b) for a, b in
                                                                           zip(rng.integers(1, 9, 70000), rng.choice(list("MID"), 70000)))
    text = (B.header() + line + "\n").encode()
    _, (rec,) = B.sam_to_bam(text)
    n_cig, = struct.unpack_from("<H", rec, 4 + 12)
    assert n_cig == 2 and b"CGBI" + struct.pack("<I", 70000) in rec
    assert outcome(B.bam_to_sam(B.bam_bytes(text)), 10, None) == outcome(text, 10, None)


def test_what_bam_cannot_hold():
    for bad in ("r\tx\tchr1\t1\t60\t5M", "r\t0\tchr1\tx\t60\t5M", "r\t0\tchr1\t1\t256\t5M", "r\t0\tchr1\t1\t60\t5Q",
                "r\t0\tchr1\t1\t60\t268435456M", "r\t0\tchr1\t1\t60", "r\t0\tchr1\t1\t60\t5M\t*\t0\t0\tACGT\t!!"):
        assert B.bam_bytes((B.header() + bad + "\n").encode()) is None, bad


def header_of(data, tmp_path):
    from sarlacc_amd import sam
    p = tmp_path / "h.bam"
    p.write_bytes(data)
    with open(p, "rb") as fh:
        return sam.read_bam_header(fh)


def text_from(data, origin):
    """The inflated bytes of a BGZF file from an origin (file offset, block number, skip) on."""
    return gzip.decompress(data[origin[0]:])[origin[2]:]


@pytest.mark.parametrize("block", [37, 5000, 65280])
def test_header_across_bgzf_blocks(tmp_path, block):
    text = B.sam_text(np.random.default_rng(3), 50)
    head, recs = B.sam_to_bam(text)
    data = bgzf_compress(head + b"".join(recs), block=block)
    names, lengths, origin = header_of(data, tmp_path)
    assert names == B.REFS + ["*"]
    assert lengths.dtype == np.int64 and lengths.tolist() == [1000 * (i + 1) for i in range(len(B.REFS))] + [0]
    assert text_from(data, origin) == b"".join(recs)
    assert origin[1] * block + origin[2] == len(head)
    if block == 37:
        assert origin[1] > 5 and origin[0] > 0


def test_header_seqinfo_is_the_binary_list_not_the_text(tmp_path):
    data = bgzf_compress(B.header_bytes(b"@SQ\tSN:from_text\tLN:5\n", [("from_list", 77), ("second", 0)]))
    names, lengths, origin = header_of(data, tmp_path)
    assert names == ["from_list", "second", "*"] and lengths.tolist() == [77, 0, 0]
    assert text_from(data, origin) == b""


def test_header_ending_on_a_block_edge(tmp_path):
    head = B.header_bytes(b"@HD\tVN:1.6\n", [("chr1", 10)])
    rec = B.raw_record(0, 4, b"r\0", 60, 0, [(5, 0)])
    data = bgzf_compress(head, block=len(head))[:-28] + bgzf_compress(rec)
    names, _, origin = header_of(data, tmp_path)
    assert names == ["chr1", "*"] and text_from(data, origin) == rec


def test_header_without_references(tmp_path):
    names, lengths, origin = header_of(bgzf_compress(B.header_bytes(b"", [])), tmp_path)
    assert names == ["*"] and lengths.tolist() == [0] and origin == (0, 0, 12)


def ref_entry(name_bytes, l_ref, l_name=None):
    return struct.pack("<i", len(name_bytes) if l_name is None else l_name) + name_bytes + struct.pack("<i", l_ref)


GOOD = B.header_bytes(b"@HD\tVN:1.6\n", [("chr1", 10), ("chr2", 20)])
REFUSALS = [
    ("magic", GOOD[:2], "file ends inside"),
    ("l_text", GOOD[:6], "file ends inside"),
    ("text", GOOD[:12], "file ends inside"),
    ("n_ref", GOOD[:21], "file ends inside"),
    ("ref_name", GOOD[:28], "file ends inside reference 1"),
    ("ref_length", GOOD[:-2], "file ends inside reference 2"),
    ("missing_ref", B.MAGIC + struct.pack("<ii", 0, 2) + ref_entry(b"a\0", 5), "file ends inside reference 2"),
    ("neg_l_text", B.MAGIC + struct.pack("<i", -1), "negative text length"),
    ("neg_n_ref", B.MAGIC + struct.pack("<ii", 0, -3), "negative number of references"),
    ("l_name_0", B.MAGIC + struct.pack("<ii", 0, 1) + ref_entry(b"", 5), "reference 1: empty name"),
    ("neg_l_name", B.MAGIC + struct.pack("<ii", 0, 1) + ref_entry(b"", 5, l_name=-4), "reference 1: negative name length"),
    ("no_nul", B.MAGIC + struct.pack("<ii", 0, 2) + ref_entry(b"a\0", 5) + ref_entry(b"bc", 5), "reference 2: name without its NUL"),
    ("neg_l_ref", B.MAGIC + struct.pack("<ii", 0, 1) + ref_entry(b"a\0", -1), "reference 1: negative length"),
    ("duplicate", B.MAGIC + struct.pack("<ii", 0, 3) + ref_entry(b"a\0", 5) + ref_entry(b"b\0", 5) + ref_entry(b"a\0", 6),
     "reference 3: duplicate name 'a'"),
    ("star", B.MAGIC + struct.pack("<ii", 0, 1) + ref_entry(b"*\0", 5), r"reference 1: duplicate name '\*'"),
]


@pytest.mark.parametrize("name,raw,message", REFUSALS, ids=[r[0] for r in REFUSALS])
@pytest.mark.parametrize("block", [5, 5000])
def test_header_refusals(tmp_path, name, raw, message, block):
    from sarlacc_amd import SarlaccError
    with pytest.raises(SarlaccError, match="BAM header: .*" + message):
        header_of(bgzf_compress(raw, block=block), tmp_path)


def test_sniffing(tmp_path):
    from sarlacc_amd import sam
    text = B.sam_text(np.random.default_rng(5), 20)
    files = {"x.bam": (B.bam_file(text), True), "tiny_blocks.bam": (B.bam_file(text, block=1), True),
             "no_eof.bam": (B.bam_file(text, eof=False), True), "x.sam.gz": (bgzf_compress(text), False),
             "x.sam": (text, False), "plain.gz": (gzip.compress(B.bam_bytes(text)), False),
             "magic_as_text.sam": (B.MAGIC + text, False), "short.bam": (bgzf_compress(b"BAM"), False), "empty": (b"", False)}
    for name, (data, expect) in files.items():
        p = tmp_path / name
        p.write_bytes(data)
        assert sam.is_bam(str(p)) is expect, name
