"""sam2ranges on BAM files, the records located and parsed on the device (bam.hip), against the restatement of
R/sam2ranges.R (tests/sam_restated.py) on the equivalent SAM text: every column, name and seqinfo entry must be equal
and every refusal must name the same record.  Integers and names: no tolerance.  Every file is read in one buffer and
again with block_bytes=4096."""
import functools
import json
import os
import struct

import numpy as np
import pytest

from tests import bam_cases as B
from tests import sam_restated as R
from tests.bgzf_cases import bgzf_compress

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = json.load(open(os.path.join(HERE, "golden", "sam2ranges_cases.json")))["cases"]
HELD = [c for c in CASES if B.bam_bytes(c["sam"].encode()) is not None]
INT_MAX = 2 ** 31 - 1
MESSAGES = {"layout": "record fields do not fit its block size", "pos": "POS is not a 32-bit integer",
            "rname": "reference ID outside the header's reference list", "cigar_star": "no CIGAR on a kept record",
            "cigar_op": "CIGAR operation code above 8", "tags": "malformed tags or CG tag", "cigar_range": "CIGAR length above",
            "cigar_clips": "only H and S", "end": "alignment end outside", "size": "block size below 32",
            "cut": "file ends inside the record"}
NAMES = B.REFS + ["*"]
HEAD = B.header_bytes(B.header().encode(), [(r, 1000 * (i + 1)) for i, r in enumerate(B.REFS)])


def run(tmp_path, data, minq=10, restricted=None, **kw):
    from sarlacc_amd import generics
    p = tmp_path / "t.bam"
    p.write_bytes(data)
    return R.as_table(generics.sam2ranges(str(p), minq=minq, restricted=restricted, **kw))


def want(text, minq=10, restricted=None):
    return R.as_table(R.sam2ranges(text, minq, restricted))


def both(tmp_path, data, expect, minq=10, restricted=None):
    assert run(tmp_path, data, minq, restricted) == expect
    assert run(tmp_path, data, minq, restricted, block_bytes=4096) == expect


def refused(tmp_path, data, record, code, minq=10, restricted=None, blocks=(None, 4096)):
    from sarlacc_amd import SarlaccError
    for block in blocks:
        kw = {} if block is None else {"block_bytes": block}
        with pytest.raises(SarlaccError, match="BAM record %d: .*%s" % (record, MESSAGES[code])):
            run(tmp_path, data, minq, restricted, **kw)


def file_of(recs, block=65280, head=HEAD):
    return bgzf_compress(head + b"".join(recs), block=block, level=1)


def encode(lines, names=NAMES):
    recs = [B.encode_record(ln.encode(), names) for ln in lines]
    assert None not in recs
    return recs


def text_of(lines, head=None):
    return ((B.header() if head is None else head) + "\n".join(lines) + "\n").encode()


def test_a_bam_was_a_sam_line_error_before(tmp_path):
    text = B.sam_text(np.random.default_rng(0), 30)
    both(tmp_path, B.bam_file(text), want(text))


@pytest.mark.parametrize("case", [c for c in HELD if "expect" in c], ids=lambda c: c["name"])
def test_golden_cases(tmp_path, case):
    data = B.bam_file(case["sam"].encode())
    e = case["expect"]
    for kw in ({}, {"block_bytes": 4096}):
        got = run(tmp_path, data, case["minq"], case["restricted"], **kw)
        assert got == {k: e[k] for k in got}


@pytest.mark.parametrize("case", [c for c in HELD if "error" in c], ids=lambda c: c["name"])
def test_golden_errors(tmp_path, case):
    text = case["sam"].encode()
    refused(tmp_path, B.bam_file(text), B.record_of_line(text, case["error"]["line"]), case["error"]["code"], case["minq"],
            case["restricted"])


@functools.lru_cache(None)
def random_file():
    text = B.sam_text(np.random.default_rng(7), 3000)
    return text, B.bam_file(text, block=65280)


@pytest.mark.parametrize("minq", [None, 0, 10, 60])
@pytest.mark.parametrize("restricted", [None, "subset", [], ["*"], ["absent_1", "absent_2"]])
def test_random_files_filters(tmp_path, minq, restricted):
    text, data = random_file()
    if restricted == "subset":
        restricted = ["chr2", "chr5", "contig_with_a_long_name_1", "*"]
    expect = want(text, minq, restricted)
    both(tmp_path, data, expect, minq, restricted)
    if restricted is None and minq == 0:
        assert len(expect["names"]) > 1000 and set(expect["strand"]) == {"+", "-"} and max(expect["left.clip"]) > 0


@pytest.mark.parametrize("block", [1, 37, 5000, 65280])
def test_bgzf_block_sizes(tmp_path, block):
    """A BGZF boundary inside a size field, inside the fixed fields, inside a CIGAR: at 1 and 37 bytes, everywhere."""
    text = B.sam_text(np.random.default_rng(block), 150 if block == 1 else 1500)
    both(tmp_path, B.bam_file(text, block=block), want(text, None), None)
    both(tmp_path, B.bam_file(text, block=block, eof=False), want(text, 10), 10)


def padded(lines, names, targets):
    """Records of the SAM lines in which line k + 1 starts at byte targets[k] of the record bytes: the lines before it
    are followed by a dropped record that a Z tag pads (None: no target)."""
    out_lines, recs, at = [], [], 0
    for ln, target in zip(lines, [None] + list(targets)):
        if target is not None:
            empty = "pad\t4\t*\t0\t0\t*\t*\t0\t0\t*\t*\tXP:Z:"
            n = target - at - len(B.encode_record(empty.encode(), names))
            assert n >= 0
            out_lines.append(empty + "p" * n)
            recs += encode(out_lines[-1:], names)
            at += len(recs[-1])
            assert at == target
        out_lines.append(ln)
        recs += encode([ln], names)
        at += len(recs[-1])
    return out_lines, recs


@pytest.mark.parametrize("d", range(-40, 9))
def test_tile_edges(tmp_path, d):
    """A record that starts at T + d and another at 3T + d: size fields across a tile edge, records that end exactly on
    one, an entry at the last byte of a tile, and tiles that lie inside one record."""
    from sarlacc_amd import _lib
    T = _lib.lib().sarlacc_bam_tile_bytes()
    rng = np.random.default_rng(100 + d)
    lines = [B.record(rng, i, mapped=True) for i in range(4)]
    lines, recs = padded(lines, NAMES, [None, T + d, 3 * T + d])
    text = text_of(lines)
    expect = want(text, None)
    assert len(expect["names"]) == 4
    both(tmp_path, file_of(recs), expect, None)


def test_large_records(tmp_path):
    """A record longer than a tile, one longer than four tiles (a 40 000-op CIGAR) and, at block_bytes=4096 and 100 000,
    longer than the buffer, which grows."""
    from sarlacc_amd import _lib
    T = _lib.lib().sarlacc_bam_tile_bytes()
    rng = np.random.default_rng(21)
    lines = [B.record(rng, 0, mapped=True), B.record(rng, 1, mapped=True) + "\tXZ:Z:" + "z" * (T + 100), B.record(rng, 2, mapped=True),
             B.record(rng, 3, mapped=True, nops=40000), B.record(rng, 4, mapped=True), B.record(rng, 5, mapped=True, nops=3000)]
    recs = encode(lines)
    assert len(recs[1]) > T and len(recs[3]) > 4 * T
    expect = want(text_of(lines), None)
    assert len(expect["names"]) == 6
    data = file_of(recs)
    both(tmp_path, data, expect, None)
    assert run(tmp_path, data, None, block_bytes=100000) == expect


def test_small_records_pack_a_tile(tmp_path):
    """37-byte records (l_read_name 1, no CIGAR, no SEQ, flag 4) over more than four tiles between kept ones: the longest
    chain a tile can hold and the most jumping rounds."""
    rng = np.random.default_rng(22)
    tiny = "\t4\t*\t0\t0\t*\t*\t0\t0\t*\t*"
    lines = [B.record(rng, 0, mapped=True)] + [tiny] * 2000 + [B.record(rng, 1, mapped=True)] + [tiny] * 500 + [B.record(rng, 2, mapped=True)]
    recs = encode(lines)
    assert len(recs[1]) == 37 and len(recs[5]) == 37
    expect = want(text_of(lines), None)
    assert len(expect["names"]) == 3
    both(tmp_path, file_of(recs), expect, None)
    both(tmp_path, file_of(recs[1:2001]), R.as_table(R.sam2ranges(text_of([]), None)), None)     # nothing kept at all


def test_decoy_payloads(tmp_path):
    """B,i tags filled with the values 32 ... 60 and quality strings whose bytes read as the size 32 at every fourth
    byte: chains of valid-looking sizes run through every payload.  Only the real records may be found."""
    rng = np.random.default_rng(23)
    lines = []
    for i in range(300):
        ln = B.record(rng, i, mapped=True).split("\t")
        n = 4 * int(rng.integers(20, 400))
        ln[9], ln[10] = "ACGT" * (n // 4), "A!!!" * (n // 4)            # QUAL bytes 20 00 00 00: the int32 32
        ln = ln[:11] + ["XD:B:i," + ",".join(str(v) for v in rng.integers(32, 61, int(rng.integers(10, 3000)))),
                        "XE:B:C," + ",".join(["36", "0", "0", "0"] * int(rng.integers(1, 200)))] + ln[11:]
        lines.append("\t".join(ln))
    recs = encode(lines)
    raw = b"".join(recs)
    assert raw.count(struct.pack("<i", 32)) > 10000 and len(raw) > 1 << 20
    for minq in (None, 10):
        both(tmp_path, file_of(recs), want(text_of(lines), minq), minq)


EVERY_TYPE = ["XA:A:q", "Xc:i:-5", "XC:i:200", "Xs:i:-30000", "XS:i:60000", "Xi:i:-100000", "XI:i:3000000000", "Xf:f:1.5",
              "XZ:Z:some text", "XH:H:1AE301", "Xb:B:c,-1,2,-3", "XB:B:S,1,60000", "Xg:B:f,0.5,2.5,1e10", "XG:B:I,7,8,9", "XE:B:C,1"]


def long_cigar_line(rng, nops=70000):
    ops = "".join("%d%s" % (a, b) for a, b in zip(rng.integers(1, 9, nops), rng.choice(list("MIDN=X"), nops)))
    return "\t".join(["long", "16", "chr2", "100", "60", "3H7S" + ops + "9S2H", "*", "0", "0", "ACGTACG", "*"] + EVERY_TYPE)


def test_cg_tag(tmp_path):
    rng = np.random.default_rng(24)
    long_line = long_cigar_line(rng)
    around = [B.record(rng, i, mapped=True) for i in range(4)]
    lines = around[:2] + [long_line] + around[2:]
    expect = want(text_of(lines), None)
    assert expect["left.clip"][2] == 10 and expect["right.clip"][2] == 11 and expect["width"][2] > 100000
    for cg_at in (0, 7, None):            # the CG tag before, among and behind tags of every type
        rec = B.encode_record(long_line.encode(), NAMES, cg_at=cg_at)
        assert struct.unpack_from("<H", rec, 16)[0] == 2
        recs = encode(around[:2]) + [rec] + encode(around[2:])
        both(tmp_path, file_of(recs), expect, None)
    # the stand-in form without a CG tag: the two ops stand as they are
    plain = "\t".join(["standin", "0", "chr1", "5", "60", "7S100N", "*", "0", "0", "ACGTACG", "*"] + EVERY_TYPE)
    lines = around[:2] + [plain] + around[2:]
    expect = want(text_of(lines), None)
    assert expect["left.clip"][2] == 7 and expect["width"][2] == 100
    both(tmp_path, file_of(encode(lines)), expect, None)


def standin(tags, flag=0):
    return B.raw_record(0, 4, b"bad\0", 60, flag, [(4, 4), (100, 3)], 4, b"\x12\x48", b"\x10" * 4, tags)


def kept(cigar, pos=4, refid=0, flag=0, **kw):
    return B.raw_record(refid, pos, b"bad\0", 60, flag, cigar, **kw)


NREF = len(B.REFS)
CG_I = b"CGBi" + struct.pack("<Ii", 1, 5 << 4)
REFUSALS = [  # (name, code, the bad record, the same value on a dropped record or None where every record is checked)
    ("l_read_name_0", "layout", B.raw_record(0, 4, b"", 60, 4, [(5, 0)]), None),
    ("name_without_nul", "layout", B.raw_record(0, 4, b"bad!", 60, 4, [(5, 0)]), None),
    ("negative_l_seq", "layout", B.raw_record(0, 4, b"bad\0", 60, 4, [(5, 0)], l_seq=-1), None),
    ("fields_beyond_block", "layout", B.raw_record(0, 4, b"bad\0", 60, 4, [(5, 0)], l_seq=9, seq=b"\x11" * 5, qual=b"!" * 8), None),
    ("cigar_beyond_block", "layout", B.raw_record(0, 4, b"bad\0", 60, 4, [(5, 0)], n_cigar_op=40000), None),
    ("pos", "pos", kept([(5, 0)], pos=INT_MAX), kept([(5, 0)], pos=INT_MAX, flag=4)),
    ("rname_n_ref", "rname", kept([(5, 0)], refid=NREF), kept([(5, 0)], refid=NREF, flag=4)),
    ("rname_minus_2", "rname", kept([(5, 0)], refid=-2), kept([(5, 0)], refid=-2, flag=4)),
    ("cigar_star", "cigar_star", kept([]), kept([], flag=4)),
    ("cigar_op_9", "cigar_op", kept([(5, 0), (3, 9)]), kept([(5, 0), (3, 9)], flag=4)),
    ("cigar_op_15", "cigar_op", kept([(1, 15)] + [(5, 0)] * 70), kept([(1, 15)], flag=4)),
    ("cigar_range", "cigar_range", kept([(2 ** 28 - 1, 0)] * 9, pos=-1), kept([(2 ** 28 - 1, 0)] * 9, flag=4)),
    ("cigar_clips_s", "cigar_clips", kept([(10, 4)]), kept([(10, 4)], flag=4)),
    ("cigar_clips_hs", "cigar_clips", kept([(3, 5), (5, 4)]), kept([(3, 5), (5, 4)], flag=4)),
    ("end", "end", kept([(1000, 0)], pos=2147483000 - 1), kept([(1000, 0)], pos=2147483000 - 1, flag=4)),
    ("end_low", "end", kept([(1, 1)], pos=-2 ** 31), kept([(1, 1)], pos=-2 ** 31, flag=4)),
    ("tags_cg_type", "tags", standin(b"NMC\x03" + CG_I), standin(b"NMC\x03" + CG_I, flag=4)),
    ("tags_cg_not_array", "tags", standin(b"CGZ5M\0"), standin(b"CGZ5M\0", flag=4)),
    ("tags_unknown_type", "tags", standin(b"XQq\x03"), standin(b"XQq\x03", flag=4)),
    ("tags_past_record", "tags", standin(b"XZZno end"), standin(b"XZZno end", flag=4)),
    ("tags_array_past_record", "tags", standin(b"CGBI" + struct.pack("<II", 3, 5 << 4)), standin(b"XBBI" + struct.pack("<I", 9), flag=4)),
    ("block_size_31", "size", struct.pack("<i", 31) + b"\0" * 31, None),
    ("block_size_0", "size", struct.pack("<i", 0), None),
    ("block_size_minus_1", "size", struct.pack("<i", -1) + b"\xff" * 40, None),
]


@functools.lru_cache(None)
def good_records():
    rng = np.random.default_rng(3)
    lines = [B.record(rng, i) for i in range(40)]
    return lines, encode(lines)


@pytest.mark.parametrize("name,code,bad,dropped", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(tmp_path, name, code, bad, dropped):
    lines, good = good_records()
    for where, blocks in ((0, (None,)), (25, (None,)), (39, (4096,))):
        recs = good[:where] + [bad] + good[where:] + ([bad] if where == 0 else [])   # the first bad record is named
        refused(tmp_path, file_of(recs), where + 1, code, blocks=blocks)
    if dropped is not None:
        both(tmp_path, file_of(good[:20] + [dropped] + good[20:]), want(text_of(lines)))


@pytest.mark.parametrize("cut", [2, 20, 50], ids=["size_field", "fixed_fields", "payload"])
def test_file_cut_inside_a_record(tmp_path, cut):
    lines, good = good_records()
    assert all(len(r) > 50 for r in good)
    for where, blocks in ((0, (None, 4096)), (25, (None,)), (39, (4096,))):
        raw = HEAD + b"".join(good[:where]) + good[where][:cut]
        for eof in (True, False):      # a missing BGZF end-of-file block changes nothing
            refused(tmp_path, bgzf_compress(raw, block=700, eof=eof), where + 1, "cut", blocks=blocks)


def test_the_lowest_record_wins(tmp_path):
    """A field error in front of a broken size field, and behind one; after an error the library is usable again."""
    lines, good = good_records()
    bad = kept([(10, 4)])
    broken = struct.pack("<i", 7) + b"\0" * 7
    refused(tmp_path, file_of(good[:5] + [bad] + good[5:10] + [broken] + good[10:]), 6, "cigar_clips")
    refused(tmp_path, file_of(good[:5] + [broken] + good[5:10] + [bad] + good[10:]), 6, "size")
    refused(tmp_path, file_of(good[:30] + [bad] + good[30:] + [good[0][:20]]), 31, "cigar_clips")
    both(tmp_path, file_of(good), want(text_of(lines)))


def test_header_only_and_empty_results(tmp_path):
    empty = R.as_table(R.sam2ranges(B.header().encode(), 10))
    both(tmp_path, file_of([]), empty)
    both(tmp_path, bgzf_compress(HEAD, block=len(HEAD)), empty)
    both(tmp_path, bgzf_compress(B.header_bytes(b"", [])), R.as_table(R.sam2ranges(b"", 10)))


def test_many_references(tmp_path):
    rng = np.random.default_rng(5)
    refs = ["ref%05d" % i for i in range(5000)]
    text = B.sam_text(rng, 2000, refs=refs)
    data = bgzf_compress(B.bam_bytes(text), block=65280, level=1)
    both(tmp_path, data, want(text, 0), 0)
    sub = [str(s) for s in rng.choice(refs, 700, replace=False)]
    both(tmp_path, data, want(text, 0, sub), 0, sub)


def test_ont_like_file(tmp_path):
    """5 000 records of 2-kb reads: 36-character names, about one CIGAR op per 6 bases, SEQ, QUAL and tags."""
    rng = np.random.default_rng(2024)
    refs = ["chr%d" % i for i in range(1, 23)]
    n, L = 5000, 2000
    pool = [B.cigar(rng, L // 6) for _ in range(64)]
    seq = "".join(rng.choice(list("ACGT"), L))
    qual = "".join(chr(int(c)) for c in rng.integers(33, 75, L))
    flags = rng.choice([0, 16, 4, 256, 2048, 272], n, p=[0.4, 0.35, 0.1, 0.05, 0.05, 0.05])
    lines = []
    for i in range(n):
        f = int(flags[i])
        lines.append("%08x-%04x-%04x-%04x-%012x\t%d\t%s\t%d\t%d\t%s\t*\t0\t0\t%s\t%s\tNM:i:%d\tms:i:%d\ttp:A:P"
                     % (i, i % 65536, 7, 9, i, f, "*" if f & 4 else refs[i % 22], 1 + (i * 7919) % 10 ** 7,
                        int(rng.integers(0, 61)), "*" if f & 4 else pool[i % 64], seq, qual, i % 50, i))
    text = (B.header(refs) + "\n".join(lines) + "\n").encode()
    expect = want(text, 10)
    assert len(expect["names"]) > 2500
    data = bgzf_compress(B.bam_bytes(text), block=65280, level=1)
    assert run(tmp_path, data, 10) == expect
    assert run(tmp_path, data, 10, block_bytes=4096) == expect      # (a buffer takes whole BGZF blocks: about 340 buffers)
