"""Reads from BAM, SEQ and QUAL unpacked on the device (bam_reads.hip), against the CPU restatement
tests/bam_reads_cases.py over the same raw bytes: names, bases, qualities and offsets must be equal byte for byte and
every refusal must name the same record.  Every file is read whole (from_bam) and again in chunks through buffers of
block_bytes=4096 (stream_bam)."""
import ctypes as C
import functools
import re
import struct

import numpy as np
import pytest

from tests import bam_cases as B
from tests import bam_reads_cases as RC
from tests.bgzf_cases import bgzf_compress

pytestmark = pytest.mark.gpu

HEAD = B.header_bytes(b"@HD\tVN:1.6\tSO:unknown\n@PG\tID:basecaller\n", [("chr1", 1000)])
LENGTHS = [0, 1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 2047, 2048, 2049, 70001]
A1 = "ACGATCAGC" + "N" * 12 + "GTCAGTCAG"
A2 = "CACACTGAGCAGCGACTAGACA"


def file_of(recs, block=3000, head=HEAD, eof=True):
    return bgzf_compress(head + b"".join(recs), block=block, level=1, eof=eof)


def rows(dev):
    """A resident batch as (names, seqs, quals), lists of bytes; the offsets are checked on the way."""
    seq, qual = dev.download()
    off = dev.off.to_numpy(np.int64, len(dev) + 1)
    assert off[0] == 0 and np.array_equal(off, dev.off_host) and np.array_equal(seq.off, qual.off)
    names = dev.names.ss
    assert names.off[0] == 0 and len(names) == len(dev)
    cut = lambda ss: [ss.chars[ss.off[i]:ss.off[i + 1]].tobytes() for i in range(len(ss))]      # noqa: E731
    return cut(names), cut(seq), cut(qual)


def whole(path, **kw):
    from sarlacc_amd.resident import DeviceReads
    return rows(DeviceReads.from_bam(str(path), **kw))


def chunked(path, number=5, block_bytes=4096, **kw):
    from sarlacc_amd.resident import DeviceReads
    out, sizes = ([], [], []), []
    for dev in DeviceReads.stream_bam(str(path), number, block_bytes=block_bytes, **kw):
        sizes.append(len(dev))
        for acc, part in zip(out, rows(dev)):
            acc += part
    assert all(s == number for s in sizes[:-1]) and all(0 < s <= number for s in sizes[-1:])
    return out


def both(tmp_path, data, expect, **kw):
    p = tmp_path / "r.bam"
    p.write_bytes(data)
    expect = tuple(expect)
    assert whole(p, **kw) == expect
    assert chunked(p, **kw) == expect


def refused(tmp_path, data, record, message, **kw):
    from sarlacc_amd import SarlaccError
    p = tmp_path / "bad.bam"
    p.write_bytes(data)
    for read in (whole, chunked):
        with pytest.raises(SarlaccError, match="BAM record %d: %s" % (record, re.escape(message))):
            read(p, **kw)


def test_a_bam_path_was_not_a_read_source_before(tmp_path):
    rng = np.random.default_rng(0)
    recs = [RC.random_read(rng, 50, f, b"r%d" % i) for i, f in enumerate([4, 16, 4])]
    both(tmp_path, file_of(recs), RC.reads(HEAD + b"".join(recs)))


@functools.lru_cache(None)
def length_records():
    rng = np.random.default_rng(1)
    recs = []
    # behind the lengths, sixteen reads of 33 bases: each starts one byte further on mod 16
    for i, (n, flag) in enumerate([(n, f) for n in LENGTHS for f in (4, 20)] + [(33, 4), (33, 20)] * 8):
        name = (b"%d_" % i).ljust(1 + i % 16, b"n")[:1 + i % 16]      # SEQ starts at every alignment mod 16
        recs.append(RC.random_read(rng, n, flag, name))
    raw = HEAD + b"".join(recs)
    return recs, RC.reads(raw)


def test_lengths_forward_and_reversed(tmp_path):
    """Every length class of the unpack pass, forward and reversed, one read above 65 535 bases that is longer than a
    locator tile and several BGZF blocks; the odd lengths put reads of two pieces and more at every destination alignment."""
    recs, expect = length_records()
    names, seqs, quals = expect
    assert [len(s) for s in seqs[:46]] == [n for n in LENGTHS for _ in (0, 1)] and {len(n) for n in names} == set(range(1, 17))
    assert {sum(map(len, seqs[:i])) % 16 for i in range(len(seqs)) if len(seqs[i]) >= 33} == set(range(16))
    both(tmp_path, file_of(recs, block=65280), expect)
    both(tmp_path, file_of(recs, block=3000), expect)


def test_code_and_quality_domain(tmp_path):
    rng = np.random.default_rng(2)
    good = [RC.random_read(rng, int(n), f, b"g%d" % i) for i, (n, f) in enumerate(zip(rng.integers(1, 300, 12), [0, 16] * 6))]
    every = [RC.read_record(b"all", f, list(range(1, 16)) * 5, (list(range(94)) * 2)[:75]) for f in (0, 16)]
    recs = good[:6] + every + good[6:]
    both(tmp_path, file_of(recs), RC.reads(HEAD + b"".join(recs)))
    for flag in (0, 16):
        refused(tmp_path, file_of(good[:6] + [RC.read_record(b"eq", flag, list(range(16)), [7] * 16)] + good[6:]), 7, RC.SEQ_EQ)
        refused(tmp_path, file_of(good[:6] + [RC.read_record(b"q", flag, [1] * 40, [93] * 39 + [94])] + good[6:]), 7, RC.QUAL_HIGH)
    # the missing-quality marker, forward and reversed, short and long; only the first byte is the marker
    missing = [RC.random_read(rng, n, f, b"m%d" % n, missing=True) for n in (1, 2, 17, 100, 2049) for f in (0, 16)]
    missing.append(RC.read_record(b"first_only", 16, [1, 2, 4, 8] * 10, [255] + [0, 94, 12] * 13))
    recs = good[:3] + missing[:5] + good[3:9] + missing[5:] + good[9:]
    for mq in (1, 40):
        expect = RC.reads(HEAD + b"".join(recs), missing_qual=mq)
        assert expect[2][3] == bytes([mq + 33])
        both(tmp_path, file_of(recs), expect, missing_qual=mq)
    refused(tmp_path, file_of(good + [RC.read_record(b"late", 0, [1] * 20, [0] * 19 + [255])]), 13, RC.QUAL_HIGH)


@pytest.mark.parametrize("n", [1, 15, 16, 17, 1025])
def test_domain_scan_at_its_step_edges(tmp_path, n):
    """The size pass scans n bytes 16 per lane and 1 024 per wavefront step, the rest byte by byte: a bad last byte among
    n bytes of SEQ (2 n bases, the code 0 in its low nibble) and of QUAL, and the same records without it are reads."""
    good = RC.read_record(b"g", 0, [1, 2, 4, 8] * 3, [30] * 12)
    seq_ok, qual_ok = RC.read_record(b"s", 0, [15] * (2 * n), [7] * (2 * n)), RC.read_record(b"q", 0, [2] * n, [93] * n)
    both(tmp_path, file_of([good, seq_ok, qual_ok]), RC.reads(HEAD + good + seq_ok + qual_ok))
    refused(tmp_path, file_of([good, RC.read_record(b"s", 0, [15] * (2 * n - 1) + [0], [7] * (2 * n))]), 2, RC.SEQ_EQ)
    refused(tmp_path, file_of([good, RC.read_record(b"q", 0, [2] * n, [93] * (n - 1) + [94])]), 2, RC.QUAL_HIGH)


def test_flags(tmp_path):
    rng = np.random.default_rng(3)
    flags = [0, 4, 16, 0x100, 0x800, 0x910, 77, 141] * 4
    recs = [RC.random_read(rng, int(n), f, b"f%d/%d" % (i, f)) for i, (n, f) in enumerate(zip(rng.integers(0, 200, len(flags)), flags))]
    raw = HEAD + b"".join(recs)
    assert len(RC.reads(raw)[0]) == 20 and len(RC.reads(raw, exclude_flags=0)[0]) == 32 and len(RC.reads(raw, exclude_flags=4)[0]) == 20
    for ex in (0x900, 0, 0x4):
        both(tmp_path, file_of(recs), RC.reads(raw, exclude_flags=ex), exclude_flags=ex)
    # a bad SEQ or QUAL in an excluded record is not an error; a bad layout there is
    bad_seq = RC.read_record(b"sec", 0x100, [0] * 9, [99] * 9)
    with_bad = recs[:10] + [bad_seq] + recs[10:]
    both(tmp_path, file_of(with_bad), RC.reads(HEAD + b"".join(with_bad)))
    refused(tmp_path, file_of(with_bad), 11, RC.SEQ_EQ, exclude_flags=0)
    bad_layout = B.raw_record(-1, -1, b"sec!", 0, 0x100, [], 4, b"\x11\x11", b"\x05" * 4)      # no NUL behind the name
    refused(tmp_path, file_of(recs[:10] + [bad_layout] + recs[10:]), 11, RC.LAYOUT)


def sized(rng, total, flag, name):
    """A record of exactly `total` bytes: random bases and a Z tag that pads."""
    base = 36 + len(name) + 1
    n = max(0, (total - base - 4) * 2 // 3 - 2)
    rest = total - base - (n + 1) // 2 - n
    assert rest >= 4
    codes, quals = rng.integers(1, 16, n).tolist(), rng.integers(0, 94, n).tolist()
    rec = RC.read_record(name, flag, codes, quals, tags=b"XPZ" + b"p" * (rest - 4) + b"\0")
    assert len(rec) == total
    return rec


@pytest.mark.parametrize("d", [-3, -40, -1000])
def test_records_across_tile_edges(tmp_path, d):
    """A kept, a dropped and a kept record that each lie across a multiple of the locator's tile."""
    from sarlacc_amd import _lib
    T = _lib.lib().sarlacc_bam_tile_bytes()
    rng = np.random.default_rng(40 - d)
    recs, at = [], 0
    for k, flag in enumerate((16, 0x100, 4)):
        fill = (k + 1) * T + d - at
        recs += [sized(rng, fill, 4, b"fill%d" % k), sized(rng, 2000, flag, b"edge%d" % k)]
        at += fill + 2000
    recs.append(RC.random_read(rng, 30, 0, b"last"))
    expect = RC.reads(HEAD + b"".join(recs))
    assert expect[0] == [b"fill0", b"edge0", b"fill1", b"fill2", b"edge2", b"last"]
    # without a header in front the offsets in the file are those of the buffer
    p = tmp_path / "edge.bam"
    p.write_bytes(bgzf_compress(B.header_bytes(b"", []), block=100, eof=False) + bgzf_compress(b"".join(recs), block=65280, level=1))
    assert whole(p) == tuple(expect) and chunked(p, number=2) == tuple(expect)


@functools.lru_cache(None)
def chunk_file():
    rng = np.random.default_rng(5)
    lens = [40, 0, 700, 9000, 3, 1500, 64, 5000, 17, 300, 1, 2500, 800]
    flags = [4, 16, 0x100, 4, 16, 4, 0x800, 16, 4, 0x110, 16, 4, 4]
    recs = [RC.random_read(rng, n, f, b"c%d" % i) for i, (n, f) in enumerate(zip(lens, flags))]
    return file_of(recs, block=2000), RC.reads(HEAD + b"".join(recs))


@pytest.mark.parametrize("number", ["1", "3", "n-1", "n", "n+1"])
def test_chunks_are_slices_of_the_whole(tmp_path, number):
    """Exactly `number` reads per chunk wherever the 4 096-byte buffers end (the 9 000-base read is larger than one: the
    buffer grows), dropped records between and behind the chunks."""
    from sarlacc_amd.resident import DeviceReads
    data, expect = chunk_file()
    n = len(expect[0])
    assert n == 10
    number = {"1": 1, "3": 3, "n-1": n - 1, "n": n, "n+1": n + 1}[number]
    p = tmp_path / "c.bam"
    p.write_bytes(data)
    at = 0
    for dev in DeviceReads.stream_bam(str(p), number, block_bytes=4096):
        assert len(dev) == min(number, n - at)
        assert rows(dev) == tuple(col[at:at + len(dev)] for col in expect)
        at += len(dev)
    assert at == n
    with pytest.raises(ValueError):
        next(DeviceReads.stream_bam(str(p), 0))


@functools.lru_cache(None)
def good_records():
    rng = np.random.default_rng(6)
    return [RC.random_read(rng, int(n), f, b"ok%d" % i) for i, (n, f) in enumerate(zip(rng.integers(20, 400, 24), [4, 16, 0x100] * 8))]      # (every record above 50 bytes)


BAD = {
    "layout": (RC.LAYOUT, B.raw_record(-1, -1, b"x\0", 0, 0x100, [], l_seq=9, seq=b"\x11" * 5, qual=b"!" * 8)),
    "seq": (RC.SEQ_EQ, RC.read_record(b"x", 4, [1, 2, 0, 4, 8], [1] * 5)),
    "seq_odd_end": (RC.SEQ_EQ, RC.read_record(b"x", 16, [1] * 64 + [0], [1] * 65)),
    "qual": (RC.QUAL_HIGH, RC.read_record(b"x", 16, [1] * 33, [93] * 32 + [200])),
    "size": (RC.SIZE, struct.pack("<i", 31) + b"\0" * 31),
}


@pytest.mark.parametrize("kind", sorted(BAD))
def test_refusals(tmp_path, kind):
    message, bad = BAD[kind]
    good = good_records()
    for where in (0, 11, 24):
        refused(tmp_path, file_of(good[:where] + [bad] + good[where:]), where + 1, message)


@pytest.mark.parametrize("cut", [2, 20, 50])
def test_file_cut_inside_a_record(tmp_path, cut):
    good = good_records()
    for where in (0, 11, 23):
        raw = HEAD + b"".join(good[:where]) + good[where][:cut]
        refused(tmp_path, bgzf_compress(raw, block=700), where + 1, RC.CUT)


def test_the_lowest_record_wins(tmp_path):
    good = good_records()
    seq, qual, size = BAD["seq"][1], BAD["qual"][1], BAD["size"][1]
    refused(tmp_path, file_of(good[:5] + [qual] + good[5:9] + [seq] + good[9:]), 6, RC.QUAL_HIGH)
    refused(tmp_path, file_of(good[:5] + [seq] + good[5:9] + [size] + good[9:]), 6, RC.SEQ_EQ)
    refused(tmp_path, file_of(good[:5] + [size] + good[5:9] + [seq] + good[9:]), 6, RC.SIZE)
    refused(tmp_path, file_of(good[:20] + [qual] + good[20:] + [good[0][:20]]), 21, RC.QUAL_HIGH)
    refused(tmp_path, file_of([RC.read_record(b"x", 0, [0, 1], [94, 1])] + good), 1, RC.SEQ_EQ)      # SEQ before QUAL
    both(tmp_path, file_of(good), RC.reads(HEAD + b"".join(good)))                                # usable after an error


@pytest.mark.parametrize("shift", [0, 5])
def test_a_middle_range_writes_its_own_bytes_only(shift):
    """The C ABI on a middle range: 64 pattern bytes in front of and behind every output array stay as they are (also
    where no output is 16-byte aligned), the offsets start at 0, NULL names are accepted."""
    from sarlacc_amd import _lib
    from sarlacc_amd._lib import check
    from sarlacc_amd.resident import DevBuffer
    lib = _lib.lib()
    recs, expect = length_records()
    raw = b"".join(recs[:30])
    names, seqs, quals = (col[:30] for col in expect)
    d_bam = DevBuffer.from_numpy(np.frombuffer(raw, np.uint8))
    nrec, used, nreads = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    check(lib.sarlacc_dev_bam_reads_index(d_bam, len(raw), 1, 1, 0x900, C.byref(nrec), C.byref(used), C.byref(nreads), None))
    assert (nrec.value, used.value, nreads.value) == (30, len(raw), 30)
    first, count = 7, 19
    tb, tn, nxt = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    check(lib.sarlacc_dev_bam_reads_range(first, count, C.byref(tb), C.byref(tn), C.byref(nxt)))
    want_seq, want_qual, want_names = (b"".join(col[first:first + count]) for col in (seqs, quals, names))
    assert (tb.value, tn.value, nxt.value) == (len(want_seq), len(want_names), len(b"".join(recs[:first + count])))
    taken = C.c_int64(0)
    check(lib.sarlacc_dev_bam_reads_records(first + count, C.byref(taken)))
    assert taken.value == first + count
    check(lib.sarlacc_dev_bam_reads_range(first, 30 - first, C.byref(tb), C.byref(tn), C.byref(nxt)))
    assert nxt.value == used.value
    check(lib.sarlacc_dev_bam_reads_range(first, count, C.byref(tb), C.byref(tn), C.byref(nxt)))
    pattern = np.arange(64, dtype=np.uint8) ^ 0xa5

    def guarded(nbytes):
        host = np.concatenate([np.zeros(shift, np.uint8), pattern, np.full(nbytes, 0xee, np.uint8), pattern])
        return DevBuffer.from_numpy(host), host.size

    def payload(buf, size, nbytes, dtype=np.uint8):
        host = buf.to_numpy(np.uint8, size)
        assert np.array_equal(host[shift:shift + 64], pattern) and np.array_equal(host[shift + 64 + nbytes:], pattern)
        return host[shift + 64:shift + 64 + nbytes].copy().view(dtype)

    sizes = {"seq": tb.value, "qual": tb.value, "off": 8 * (count + 1), "names": tn.value, "noff": 8 * (count + 1)}
    for with_names in (True, False):
        bufs = {k: guarded(v) for k, v in sizes.items()}
        at = {k: bufs[k][0].ptr.value + shift + 64 for k in bufs}
        check(lib.sarlacc_dev_bam_reads_extract(d_bam, first, count, 1, at["seq"], at["qual"], at["off"],
                                                at["names"] if with_names else None, at["noff"] if with_names else None, None))
        got = {k: payload(bufs[k][0], bufs[k][1], sizes[k], np.int64 if k in ("off", "noff") else np.uint8) for k in bufs}
        assert got["seq"].tobytes() == want_seq and got["qual"].tobytes() == want_qual
        assert np.array_equal(got["off"], RC.flat(seqs[first:first + count])[1])
        if with_names:
            assert got["names"].tobytes() == want_names and np.array_equal(got["noff"], RC.flat(names[first:first + count])[1])
        else:
            assert (got["names"] == 0xee).all() and (got["noff"].view(np.uint8) == 0xee).all()
    # an empty range and an empty buffer succeed
    check(lib.sarlacc_dev_bam_reads_range(30, 0, C.byref(tb), C.byref(tn), C.byref(nxt)))
    assert (tb.value, tn.value, nxt.value) == (0, 0, used.value)
    check(lib.sarlacc_dev_bam_reads_index(d_bam, 0, 1, 1, 0x900, C.byref(nrec), C.byref(used), C.byref(nreads), None))
    assert (nrec.value, used.value, nreads.value) == (0, 0, 0)


@functools.lru_cache(None)
def mock_pair():
    """The same 200 reads as FASTQ text and as BAM records (half of them stored reverse-complemented with flag 0x10)."""
    from sarlacc_amd.mock import mock_reads
    sim = mock_reads(A1, A2, nmolecules=40, nreads=5, seqlen=400, seed=2024)
    names = ["READ_%d" % (i + 1) for i in range(len(sim["reads"]))]
    assert len(names) == 200
    text, recs = [], []
    for i, (nm, s, q) in enumerate(zip(names, sim["reads"], sim["quals"])):
        text.append("@%s\n%s\n+\n%s\n" % (nm, s, q))
        codes, vals = RC.seq_codes(s), [ord(c) - 33 for c in q]
        if i % 2:
            codes, vals = [RC.complement(c) for c in reversed(codes)], vals[::-1]
        recs.append(RC.read_record(nm.encode(), 16 if i % 2 else 4, codes, vals))
        if i % 7 == 0:      # the same read again as a supplementary piece: dropped
            recs.append(RC.read_record(nm.encode(), 0x800, codes[:50], vals[:50]))
    return "".join(text).encode(), file_of(recs, block=65280)


def test_round_trip_with_the_fastq_route(tmp_path):
    from sarlacc_amd import generics as G
    from sarlacc_amd.resident import DeviceReads
    text, data = mock_pair()
    fq, bam = tmp_path / "r.fastq", tmp_path / "r.bam"
    fq.write_bytes(text)
    bam.write_bytes(data)
    a, b = DeviceReads.from_fastq(str(fq)), DeviceReads.from_bam(str(bam))
    assert rows(a) == rows(b) and np.array_equal(a.off_host, b.off_host)
    assert b.fastq_text() == text
    out = tmp_path / "back.fastq"
    assert b.to_fastq(str(out)) == len(text) and out.read_bytes() == text
    host = G.read_bam(str(bam))
    assert host.names == list(a.names) and host.seq.to_strings() == a.download()[0].to_strings()
    assert host.qual.to_strings() == a.download()[1].to_strings()

    def same(x, y):
        assert x["names"] == y["names"] and np.array_equal(x["read.width"], y["read.width"]) and np.array_equal(x["reversed"], y["reversed"])
        for key in ("adaptor1", "adaptor2"):
            assert np.array_equal(x[key]["score"].view(np.int64), y[key]["score"].view(np.int64))
            assert np.array_equal(x[key]["start"], y[key]["start"]) and np.array_equal(x[key]["end"], y[key]["end"])
            assert x[key]["subseq"] == y[key]["subseq"] and x[key]["metadata"] == y[key]["metadata"]
        assert {k: v for k, v in x["metadata"].items() if k != "filepath"} == {k: v for k, v in y["metadata"].items() if k != "filepath"}

    aln_fq = G.adaptorAlign(A1, A2, str(fq), tolerance=120)
    for number in (1e5, 37):
        aln_bam = G.adaptorAlign(A1, A2, str(bam), tolerance=120, number=number)
        same(aln_fq, aln_bam)
        assert aln_bam["metadata"]["filepath"] == str(bam)
    filt_fq, filt_bam = G.filterReads(aln_fq, 6, 6), G.filterReads(aln_bam, 6, 6)
    assert len(filt_fq["names"]) > 0
    same(filt_fq, filt_bam)
    assert np.array_equal(filt_fq["trim.start"], filt_bam["trim.start"]) and np.array_equal(filt_fq["trim.end"], filt_bam["trim.end"])
    want = G.realizeReads(filt_fq)
    for number in (1e5, 37):
        got = G.realizeReads(filt_bam, number=number)
        assert got.names == want.names and got.seq.to_strings() == want.seq.to_strings()
        assert got.qual.to_strings() == want.qual.to_strings()
    with pytest.raises(ValueError, match="qual_type"):
        G.adaptorAlign(A1, A2, str(bam), qual_type="solexa")


def test_header_only_files(tmp_path):
    from sarlacc_amd import generics as G
    from sarlacc_amd.resident import DeviceReads
    fq, bam = tmp_path / "e.fastq", tmp_path / "e.bam"
    fq.write_bytes(b"")
    for data in (file_of([]), bgzf_compress(HEAD, block=len(HEAD)), file_of([RC.random_read(np.random.default_rng(0), 9, 0x100)])):
        bam.write_bytes(data)
        dev = DeviceReads.from_bam(str(bam))
        assert len(dev) == 0 and dev.names == [] and rows(dev) == ([], [], [])
        assert list(DeviceReads.stream_bam(str(bam), 3)) == []
        a, b = G.adaptorAlign(A1, A2, str(fq)), G.adaptorAlign(A1, A2, str(bam))
        assert len(b["read.width"]) == 0 and len(b["names"]) == 0 and b["reversed"].dtype == a["reversed"].dtype
        for key in ("adaptor1", "adaptor2"):
            assert sorted(a[key]) == sorted(b[key]) and len(b[key]["score"]) == 0 and sorted(a[key]["subseq"]) == sorted(b[key]["subseq"])
