"""Unaligned BAM written from resident reads (sarlacc_dev_bam_format_size / _format, sarlacc_dev_bgzf_deflate_cuts,
DeviceReads.to_bam, generics.write_bam).  Every byte is held against tests/bam_write_cases.py, which restates the writer
in plain Python, and files are decoded by decoders that are not the code under test first: gzip.decompress (zlib checks
every member's CRC-32 and ISIZE) and the Python inflate of tests.bgzf_cases; then by the package's own readers."""
import ctypes as C
import functools
import gzip
import zlib

import numpy as np
import pytest

from tests import bam_reads_cases as Rd
from tests import bam_write_cases as Bw
from tests import bgzf_write_cases as W
from tests.bgzf_cases import EOF_BLOCK, bgzf_compress, ref_inflate

pytestmark = pytest.mark.gpu

GUARD = 48            # bytes of 0xEE either side of an output
TABLE_ROOM = 8 * Bw.TABLE_ROOM      # 300 bytes for each of the 8 blocks


def _buf(data):
    from sarlacc_amd.resident import DevBuffer
    return DevBuffer.from_numpy(np.frombuffer(data or b"\0", np.uint8))


def device_batch(names, seqs, quals, encoding=None):
    """The reads as a resident batch, their names (None: default names) as the StrList from_fastq would leave."""
    from sarlacc_amd.encoding import phred_encoding
    from sarlacc_amd.resident import DevBuffer, DeviceReads
    from sarlacc_amd.strset import StrList
    s, off = Rd.flat(seqs)
    q, _ = Rd.flat(quals)
    dev = DeviceReads(_buf(s), _buf(q), DevBuffer.from_numpy(off), off, encoding if encoding is not None else phred_encoding())
    if names is not None:
        dev.names = StrList(list(names))
    return dev


class Sized:
    """Step 1 through the C ABI: the record offsets and cuts on the device and on the host."""

    def __init__(self, dev, names, first_index=1, with_cuts=True):
        from sarlacc_amd import _lib
        from sarlacc_amd.resident import DevBuffer
        n = len(dev)
        self.dev, self.n, self.first_index = dev, n, first_index
        self.names = self.noff = None
        if names is not None:
            nb, noff = Rd.flat(names)
            self.names, self.noff = _buf(nb), DevBuffer.from_numpy(noff)
        self.rec_off = DevBuffer.from_numpy(np.full(n + 2, -7, np.int64))
        self.cuts = DevBuffer.from_numpy(np.full(2 * n + 1, -7, np.int64)) if with_cuts else None
        total = C.c_int64(-1)
        _lib.check(_lib.lib().sarlacc_dev_bam_format_size(dev.seq, dev.qual, dev.off, n, self.names, self.noff, first_index,
                                                          self.rec_off, self.cuts, C.byref(total), None))
        ro = self.rec_off.to_numpy(np.int64, n + 2)
        assert ro[-1] == -7, "offsets written past n + 1 entries"
        self.ro, self.total = ro[:-1].copy(), total.value
        assert self.total == self.ro[-1]
        if with_cuts:
            cu = self.cuts.to_numpy(np.int64, 2 * n + 1)
            assert cu[-1] == -7, "cuts written past 2 n entries"
            self.cu = cu[:-1].copy()

    def format(self, first=0, count=None, shift=0):
        """Step 2: the records [first, first + count) written `shift` bytes into a guarded buffer."""
        from sarlacc_amd import _lib
        from sarlacc_amd.resident import DevBuffer
        count = self.n - first if count is None else count
        nbytes = int(self.ro[first + count] - self.ro[first])
        assert GUARD % 16 == 0
        d_out = DevBuffer.from_numpy(np.full(2 * GUARD + shift + nbytes, 0xEE, np.uint8))
        dev = self.dev
        _lib.check(_lib.lib().sarlacc_dev_bam_format(dev.seq, dev.qual, dev.off, self.names, self.noff, self.first_index,
                                                     self.rec_off, first, count, C.c_void_p(d_out.ptr.value + GUARD + shift), None))
        got = d_out.to_numpy(np.uint8, 2 * GUARD + shift + nbytes)
        assert (got[:GUARD + shift] == 0xEE).all() and (got[GUARD + shift + nbytes:] == 0xEE).all(), "bytes written outside the range"
        return got[GUARD + shift:GUARD + shift + nbytes].tobytes()


def sized(batch, first_index=1, default_names=False, with_cuts=True):
    names, seqs, quals = batch
    return Sized(device_batch(None, seqs, quals), None if default_names else names, first_index, with_cuts)


def first_difference(got, want):
    a, b = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
    if a.size != b.size:
        return "%d bytes, %d expected" % (a.size, b.size)
    d = np.flatnonzero(a != b)
    return None if d.size == 0 else "byte %d is %d, not %d (%d bytes differ)" % (d[0], a[d[0]], b[d[0]], d.size)


# ---- 1. bytes, record by record ---------------------------------------------------------------------------------------

def test_bytes_of_every_length_and_name():
    batch = Bw.batch_lengths()
    S = sized(batch)
    off, cuts = Bw.layout(*batch)
    assert np.array_equal(S.ro, off) and np.array_equal(S.cu, cuts)
    got, want = S.format(), Bw.expected_records(*batch)
    assert first_difference(got, want) is None
    recs = Bw.record_list(*batch)
    for k in range(len(recs)):     # record by record: the message names the record
        assert got[off[k]:off[k + 1]] == recs[k], "record %d of %d bases" % (k + 1, len(batch[1][k]))


@pytest.mark.parametrize("first_index", [1, 999999])
def test_default_names(first_index):
    batch = Bw.batch_forty()
    S = sized(batch, first_index, default_names=True, with_cuts=False)      # d_cuts NULL
    off, _ = Bw.layout(None, batch[1], batch[2], first_index)
    assert np.array_equal(S.ro, off)
    got = S.format()
    assert first_difference(got, Bw.expected_records(None, batch[1], batch[2], first_index)) is None
    assert got[36:36 + 6 + len(str(first_index))] == b"READ_%d\0" % first_index
    if first_index == 999999:      # the width of the number grows inside the batch
        assert got[off[1] + 36:off[1] + 36 + 13] == b"READ_1000000\0"


def test_empty_batch_and_empty_range():
    S = sized(([], [], []))
    assert S.total == 0 and S.ro.tolist() == [0] and S.format() == b""
    S = sized(Bw.batch_forty())
    assert S.format(first=40, count=0) == b"" and S.format(first=3, count=0) == b""


# ---- 2. tiles and ranges ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["tiny", "span", "file"])
def test_tiles(name):
    batch = Bw.BATCHES[name]()
    S = sized(batch)
    off, cuts = Bw.layout(*batch)
    assert np.array_equal(S.ro, off) and np.array_equal(S.cu, cuts)
    assert first_difference(S.format(shift=5), Bw.expected_records(*batch)) is None


def test_ranges_at_every_record_boundary_and_misalignment():
    batch = Bw.batch_forty()
    S, want = sized(batch), Bw.expected_records(*Bw.batch_forty())
    for shift in range(16):
        assert first_difference(S.format(shift=shift), want) is None, "misaligned by %d" % shift
    for k in range(1, 40):
        got = S.format(0, k, shift=k % 16) + S.format(k, 40 - k, shift=(3 * k) % 16)
        assert first_difference(got, want) is None, "split at record %d" % k
    got = b"".join(S.format(k, 1, shift=(5 * k) % 16) for k in range(40))
    assert first_difference(got, want) is None
    span = Bw.batch_span()
    S, want = sized(span), Bw.expected_records(*span)
    got = S.format(0, 4, shift=9) + S.format(4, 1, shift=7) + S.format(5, 4, shift=1)      # the long read alone
    assert first_difference(got, want) is None


# ---- 3. refusals ------------------------------------------------------------------------------------------------------

GOOD = (b"name", b"ACGTN", b"!I5~+")


def _refused(reads):
    """The error of the size pass for [(name, seq, qual)], after the helper has said the same."""
    from sarlacc_amd._lib import SarlaccError
    names, seqs, quals = ([r[k] for r in reads] for k in range(3))
    k, why = Bw.first_refusal(names, seqs, quals)
    with pytest.raises(SarlaccError) as e:
        sized((names, seqs, quals))
    assert str(e.value) == "record %d: %s" % (k, why)
    return k, why


def test_each_message_on_its_own():
    assert _refused([GOOD, (b"n" * 255, b"AC", b"II")]) == (2, Bw.NAME_LONG)
    assert _refused([(b"a\x01b", b"AC", b"II"), GOOD]) == (1, Bw.NAME_BYTE)
    assert _refused([GOOD, GOOD, (b"n", b"ACXT", b"IIII")]) == (3, Bw.BASE)
    assert _refused([GOOD, (b"n", b"ACGT", b"II I")]) == (2, Bw.QUAL)


def test_the_lower_record_wins_and_the_order_inside_a_record():
    assert _refused([GOOD, (b"n", b"ACGT", b"II\x7fI"), (b"n" * 300, b"A", b"I"), GOOD])[0] == 2
    assert _refused([GOOD] * 70 + [(b"n", b"AC-T", b"IIII")] + [GOOD] * 70 + [(b"\x7f", b"A", b"I")])[0] == 71
    assert _refused([(b"n" * 255 + b"\x01", b"a", b" ")]) == (1, Bw.NAME_LONG)
    assert _refused([(b"n\x01", b"a", b" ")]) == (1, Bw.NAME_BYTE)
    assert _refused([(b"n", b"a", b" ")]) == (1, Bw.BASE)
    assert _refused([(b"n", b"A" * 5000 + b"a", b" " * 5001)]) == (1, Bw.BASE)


@pytest.mark.parametrize("base", [b"=", b"a", b"-", b"\0", b"@", b"Z", b"[", b"n"])
@pytest.mark.parametrize("length", [1, 16, 40, 2000])
def test_bases_that_bam_cannot_hold(base, length):
    for at in {0, length // 2, length - 1}:
        seq = b"A" * at + base + b"C" * (length - at - 1)
        assert _refused([GOOD, (b"n", seq, b"I" * length)]) == (2, Bw.BASE)


@pytest.mark.parametrize("q", [0, 32, 127, 128, 255])
def test_quality_bytes_outside_phred33(q):
    for length, at in ((1, 0), (17, 16), (2000, 1999), (2000, 7)):
        qual = b"!" * at + bytes([q]) + b"~" * (length - at - 1)
        assert _refused([(b"n", b"G" * length, qual)]) == (1, Bw.QUAL)


@pytest.mark.parametrize("length", [15, 16, 17, 1025])
def test_domain_scan_at_its_step_edges(length):
    """The lengths around the 16 bytes of a lane and one past the 1 024 of a wavefront step that the two tests above
    leave out between them: a bad last base, a bad last quality, and the record without them."""
    seq, qual = b"ACGT" * (length // 4) + b"N" * (length % 4), b"!" + b"~" * (length - 1)
    assert _refused([GOOD, (b"n", seq[:-1] + b"=", qual)]) == (2, Bw.BASE)
    assert _refused([GOOD, (b"n", seq, qual[:-1] + b"\x7f")]) == (2, Bw.QUAL)
    batch = ([b"n"], [seq], [qual])
    assert first_difference(sized(batch).format(), Bw.expected_records(*batch)) is None


def test_names_at_the_limits():
    assert _refused([(b"n" * 255, b"A", b"I")]) == (1, Bw.NAME_LONG)
    assert _refused([(b"n" * 254 + b"x comment", b"A", b"I")]) == (1, Bw.NAME_LONG)
    assert _refused([(b"ab\x1fcd efg", b"A", b"I")]) == (1, Bw.NAME_BYTE)
    assert _refused([(b"n" * 40 + b"\x80", b"A", b"I")]) == (1, Bw.NAME_BYTE)
    ok = [(b"n" * 254, b"A", b"I"), (b"0123456789 " + b"c" * 289, b"A", b"I"), (b"ab cd\x01\x7f", b"A", b"I"),
          (b"k" * 254 + b"\tcomment", b"A", b"I")]
    batch = tuple([r[k] for r in ok] for k in range(3))
    assert len(ok[1][0]) == 300 and Bw.qname(ok[1][0]) == b"0123456789"
    assert first_difference(sized(batch).format(), Bw.expected_records(*batch)) is None


def test_a_refused_to_bam_leaves_the_file(tmp_path):
    from sarlacc_amd._lib import SarlaccError
    path = tmp_path / "kept.bam"
    path.write_bytes(b"what it held")
    dev = device_batch([b"a", b"b"], [b"ACGT", b"AC=T"], [b"IIII", b"IIII"])
    with pytest.raises(SarlaccError, match="record 2: base cannot be stored in BAM"):
        dev.to_bam(str(path))
    assert path.read_bytes() == b"what it held"


# ---- 4. deflate with cuts ---------------------------------------------------------------------------------------------

def deflate_abi(text, mode, cuts=None, origin=0):
    """sarlacc_dev_bgzf_deflate_cuts (cuts None: sarlacc_dev_bgzf_deflate) through the C ABI, the output between guards
    of 0xEE: (compressed bytes, block offsets)."""
    from sarlacc_amd import _lib, bgzf
    from sarlacc_amd.resident import DevBuffer
    lib = _lib.lib()
    n_blocks, cap = bgzf.deflate_bound(len(text))
    d_src = _buf(text)
    d_out = DevBuffer.from_numpy(np.full(cap + 2 * GUARD, 0xEE, np.uint8))
    d_off = DevBuffer.from_numpy(np.full(n_blocks + 2, -7, np.int64))
    total, out_ptr = C.c_int64(-1), C.c_void_p(d_out.ptr.value + GUARD)
    if cuts is None:
        _lib.check(lib.sarlacc_dev_bgzf_deflate(d_src, len(text), mode, out_ptr, cap, d_off, C.byref(total), None))
    else:
        host = np.ascontiguousarray(cuts, dtype=np.int64)
        d_cuts = DevBuffer.from_numpy(host) if host.size else None
        _lib.check(lib.sarlacc_dev_bgzf_deflate_cuts(d_src, len(text), d_cuts, host.size, origin, mode, out_ptr, cap, d_off,
                                                     C.byref(total), None))
    out = d_out.to_numpy(np.uint8, cap + 2 * GUARD)
    assert 0 <= total.value <= cap
    assert (out[:GUARD] == 0xEE).all() and (out[GUARD + total.value:] == 0xEE).all(), "bytes written outside the output"
    off = d_off.to_numpy(np.int64, n_blocks + 2)
    assert off[-1] == -7 and off[-2] == total.value
    return out[GUARD:GUARD + total.value].tobytes(), off[:-1].copy()


@functools.lru_cache(maxsize=None)
def seeded(L, how):
    """The 8 blocks of Bw.seeded_records(L): how = "cuts" (mode 0 with the records' cuts) or "one" (mode 1)."""
    raw, cuts = Bw.seeded_records(L)
    return deflate_abi(raw, 0, cuts) if how == "cuts" else deflate_abi(raw, 1)


@pytest.mark.parametrize("L", [100, 2000])
def test_blocks_with_cuts_inflate_and_only_shrink(L):
    raw, _ = Bw.seeded_records(L)
    (comp, off), (one, off1) = seeded(L, "cuts"), seeded(L, "one")
    assert len(off) == 9 and len(off1) == 9
    for k, text in enumerate(W.pieces(raw)):
        payload, crc, isize = Bw.block_parts(comp[off[k]:off[k + 1]])
        assert len(text) == W.BLOCK and isize == W.BLOCK and crc == zlib.crc32(text)
        assert zlib.decompress(payload, -15) == text, "block %d" % k
        assert off[k + 1] - off[k] <= W.BLOCK + W.STORED + W.FRAMING
    assert gzip.decompress(comp + EOF_BLOCK) == raw and gzip.decompress(one + EOF_BLOCK) == raw
    assert (np.diff(off) <= np.diff(off1)).all()


def test_long_reads_take_a_table_per_field():
    y = Bw.yardsticks(2000)
    got, one = len(seeded(2000, "cuts")[0]), len(seeded(2000, "one")[0])
    print("2 000-base records with cuts: %d bytes; zlib level 6 %d (ratio %.4f), zlib Huffman-only per field %d (ratio %.4f); "
          "mode 1 %d (ratio %.4f)" % (got, y["level6"], got / y["level6"], y["per_field"], got / y["per_field"], one, got / one))
    assert got <= y["level6"]
    assert got < one


def test_short_reads_take_one_table():
    y = Bw.yardsticks(100)
    got, one = len(seeded(100, "cuts")[0]), len(seeded(100, "one")[0])
    print("100-base records with cuts: %d bytes; zlib Huffman-only %d (ratio %.4f), per field %d; mode 1 %d"
          % (got, y["huffman"], got / y["huffman"], y["per_field"], one))
    assert got <= y["huffman"] + TABLE_ROOM


def _two_fields():
    """1 000 bytes over 4 values, then 2 000 over 40: a table for each is smaller than one for both."""
    rng = np.random.default_rng(21)
    return rng.integers(1, 5, 1000).astype(np.uint8).tobytes() + rng.integers(40, 80, 2000).astype(np.uint8).tobytes()


def _deflate_blocks(comp):
    """The number of deflate blocks in the one BGZF block of `comp`, after the text came out right."""
    text, stats = ref_inflate(comp[18:-8])
    return text, len(stats)


def test_no_cuts_is_mode_1():
    for text in (_two_fields(), Bw.seeded_records(2000)[0][:W.BLOCK + 777]):
        assert deflate_abi(text, 0, [])[0] == deflate_abi(text, 1)[0]
        assert deflate_abi(text, 1, [1000])[0] == deflate_abi(text, 1)[0]
        assert deflate_abi(text, 2, [1000])[0] == deflate_abi(text, 2)[0]


def test_cuts_outside_the_text_are_ignored():
    text, origin = _two_fields(), 5000
    want, _ = deflate_abi(text, 0, [origin + 1000], origin)
    assert _deflate_blocks(want) == (text, 2) and len(want) < len(deflate_abi(text, 1)[0])
    assert deflate_abi(text, 0, [1000])[0] == want                                    # the origin is only an offset
    outside = [0, 40, origin - 1, origin, origin + 1000, origin + len(text), origin + len(text) + 1, origin + 10 ** 9]
    assert deflate_abi(text, 0, outside, origin)[0] == want
    assert deflate_abi(text, 0, [origin + len(text)], origin)[0] == deflate_abi(text, 1)[0]
    # the newlines of a text play no part once cuts are given
    lines = W.synth_fastq(9000, 2000, 4)
    assert deflate_abi(lines, 0, [])[0] == deflate_abi(lines, 1)[0] != deflate_abi(lines, 0)[0]


def test_a_cut_closes_a_piece_only_64_bytes_into_it():
    text = _two_fields()
    want = deflate_abi(text, 0, [1000])[0]
    assert deflate_abi(text, 0, [1000, 1010])[0] == want
    assert deflate_abi(text, 0, [10, 63, 1000, 1063])[0] == want
    three = deflate_abi(text, 0, [1000, 1064])[0]
    assert three != want and gzip.decompress(three + EOF_BLOCK) == text
    # 64 is the first position that closes a piece: where it does, three tables were smaller than two
    rng = np.random.default_rng(22)
    text = bytes(64) + rng.integers(1, 5, 1000).astype(np.uint8).tobytes() + rng.integers(40, 80, 2000).astype(np.uint8).tobytes()
    assert _deflate_blocks(deflate_abi(text, 0, [64, 1064])[0]) == (text, 3)
    assert _deflate_blocks(deflate_abi(text, 0, [63, 1064])[0]) == (text, 2)


def test_cuts_in_later_blocks_use_the_block_s_own_positions():
    """Block 1 of a two-block text gets the pieces its cuts give it, wherever block 0's lie."""
    fields = _two_fields()
    text = Bw.seeded_records(2000)[0][:W.BLOCK] + fields
    comp, off = deflate_abi(text, 0, [W.BLOCK + 1000], 0)
    assert gzip.decompress(comp + EOF_BLOCK) == text
    assert comp[off[1]:] == deflate_abi(fields, 0, [1000])[0]
    assert comp[:off[1]] == deflate_abi(text[:W.BLOCK], 1)[0]


def test_deflate_device_routes_cuts():
    from sarlacc_amd import bgzf
    text = _two_fields()
    want = deflate_abi(text, 0, [1000])[0]
    d_text = _buf(text)
    for cuts, origin in (([1000], 0), (np.array([1700]), 700), ((_buf(np.array([1000], np.int64).tobytes()), 1), 0)):
        d_comp, nbytes = bgzf.deflate_device(d_text, len(text), cuts=cuts, cut_origin=origin)
        assert d_comp.to_numpy(np.uint8, nbytes).tobytes() == want
    d_comp, nbytes = bgzf.deflate_device(d_text, len(text))
    assert d_comp.to_numpy(np.uint8, nbytes).tobytes() == deflate_abi(text, 0)[0]


# ---- 5. files ---------------------------------------------------------------------------------------------------------

def _blocks_of(data):
    """The BGZF blocks of a file, split at their BSIZE fields."""
    out, p = [], 0
    while p < len(data):
        size = int.from_bytes(data[p + 16:p + 18], "little") + 1
        out.append(data[p:p + size])
        p += size
    assert p == len(data)
    return out


def test_file(tmp_path):
    from sarlacc_amd import bgzf, generics as G, sam
    from sarlacc_amd.resident import DeviceReads
    batch = Bw.batch_file()
    names, seqs, quals = batch
    want = Bw.header_bytes() + Bw.expected_records(*batch)
    path = tmp_path / "reads.bam"
    dev = device_batch(*batch)
    assert dev.to_bam(str(path)) == path.stat().st_size
    data = path.read_bytes()
    assert first_difference(gzip.decompress(data), want) is None
    assert data.endswith(EOF_BLOCK)
    blocks = _blocks_of(data)
    assert gzip.decompress(blocks[0]) == Bw.header_bytes()           # the header has blocks of its own
    n, used, _, text_off, eof = bgzf.scan(data)
    assert n == len(blocks) and used == len(data) and eof and text_off[-1] == len(want)
    assert sam.is_bam(str(path))
    with open(path, "rb") as fh:
        ref_names, ref_lengths, origin = sam.read_bam_header(fh)
    assert ref_names == ["*"] and ref_lengths.tolist() == [0]
    back = DeviceReads.from_bam(str(path))
    s, q = back.download()
    assert [x.encode() for x in s.to_strings()] == seqs and [x.encode() for x in q.to_strings()] == quals
    assert list(back.names) == [Bw.qname(n).decode() for n in names]
    ranges = G.sam2ranges(str(path))
    assert len(ranges["start"]) == 0 and ranges["seqinfo"]["seqnames"] == ["*"]
    # many ranges: other blocks, the same bytes
    small = tmp_path / "small.bam"
    assert dev.to_bam(str(small), block_bytes=1000) == small.stat().st_size
    assert gzip.decompress(small.read_bytes()) == want and len(_blocks_of(small.read_bytes())) > len(blocks)
    again = DeviceReads.from_bam(str(small)).download()
    assert again[0].to_strings() == s.to_strings() and again[1].to_strings() == q.to_strings()


def test_ranges_start_new_blocks_and_records_straddle_them(tmp_path):
    """Three reads of 50 000 bases in ranges of two and one: five blocks of records, the second range in its own."""
    batch = Bw.draw(np.random.default_rng(31), [50000, 50000, 50000], Bw.BASES)
    recs = Bw.record_list(*batch)
    path = tmp_path / "straddle.bam"
    device_batch(*batch).to_bam(str(path), block_bytes=len(recs[0]) + len(recs[1]))
    blocks = _blocks_of(path.read_bytes())
    sizes = [len(gzip.decompress(b)) for b in blocks]
    two = len(recs[0]) + len(recs[1])
    assert sizes == [len(Bw.header_bytes()), W.BLOCK, W.BLOCK, two - 2 * W.BLOCK, W.BLOCK, len(recs[2]) - W.BLOCK, 0]
    assert gzip.decompress(path.read_bytes()) == Bw.header_bytes() + b"".join(recs)


def test_headers(tmp_path):
    from sarlacc_amd._lib import SarlaccError
    batch = Bw.batch_forty()
    dev, path = device_batch(*batch), tmp_path / "h.bam"
    text = "@HD\tVN:1.6\tSO:unsorted\n@RG\tID:run1\tPL:ONT\n@CO\tmade here\n"
    dev.to_bam(str(path), header=text)
    assert gzip.decompress(path.read_bytes()) == Bw.header_bytes(text.encode()) + Bw.expected_records(*batch)
    dev.to_bam(str(path), header=b"")
    assert gzip.decompress(path.read_bytes()) == Bw.header_bytes(b"") + Bw.expected_records(*batch)
    before = path.read_bytes()
    with pytest.raises(SarlaccError, match="@SQ"):
        dev.to_bam(str(path), header="@HD\tVN:1.6\n@SQ\tSN:chr1\tLN:1000\n")
    assert path.read_bytes() == before


def test_empty_batch(tmp_path):
    from sarlacc_amd import sam
    from sarlacc_amd.resident import DeviceReads
    path = tmp_path / "empty.bam"
    assert device_batch([], [], []).to_bam(str(path)) == path.stat().st_size
    data = path.read_bytes()
    assert len(_blocks_of(data)) == 2 and data.endswith(EOF_BLOCK) and gzip.decompress(data) == Bw.header_bytes()
    assert sam.is_bam(str(path)) and len(DeviceReads.from_bam(str(path))) == 0


def test_default_names_in_a_file(tmp_path):
    _, seqs, quals = Bw.batch_forty()
    path = tmp_path / "d.bam"
    device_batch(None, seqs, quals).to_bam(str(path))
    assert gzip.decompress(path.read_bytes()) == Bw.header_bytes() + Bw.expected_records(None, seqs, quals)


# ---- 6. round trip from BAM -------------------------------------------------------------------------------------------

def test_round_trip_from_bam(tmp_path):
    """Reverse-strand, secondary and missing-quality records -> from_bam -> to_bam -> from_bam: the same reads."""
    from sarlacc_amd.resident import DeviceReads
    rng = np.random.default_rng(41)
    recs = [Rd.random_read(rng, 300, 0, b"fwd"), Rd.random_read(rng, 4097, 16, b"rev"), Rd.random_read(rng, 50, 0x100, b"secondary"),
            Rd.random_read(rng, 33, 4, b"noqual", missing=True), Rd.random_read(rng, 0, 4, b"empty"),
            Rd.random_read(rng, 2001, 0x14, b"rev_unmapped")]
    raw = Rd.B.header_bytes(b"@HD\tVN:1.6\n", []) + b"".join(recs)
    names, seqs, quals = Rd.reads(raw)
    assert names == [b"fwd", b"rev", b"noqual", b"empty", b"rev_unmapped"]
    src, out = tmp_path / "in.bam", tmp_path / "out.bam"
    src.write_bytes(bgzf_compress(raw, block=5000))
    first = DeviceReads.from_bam(str(src))
    first.to_bam(str(out))
    assert gzip.decompress(out.read_bytes()) == Bw.header_bytes() + Bw.expected_records(names, seqs, quals)
    second = DeviceReads.from_bam(str(out))
    a, b = first.download(), second.download()
    assert b[0].to_strings() == a[0].to_strings() == [s.decode() for s in seqs]
    assert b[1].to_strings() == a[1].to_strings() == [q.decode() for q in quals]
    assert list(second.names) == list(first.names) == [n.decode() for n in names]


# ---- 7. generics.write_bam --------------------------------------------------------------------------------------------

def test_write_bam_of_host_reads(tmp_path):
    from sarlacc_amd import generics as G
    from sarlacc_amd.resident import DeviceReads
    names, seqs, quals = Bw.batch_forty()
    reads = G.Reads(seqs, quals, [n.decode() for n in names])
    host, dev = tmp_path / "host.bam", tmp_path / "dev.bam"
    assert G.write_bam(str(host), reads) == host.stat().st_size
    uploaded = DeviceReads.upload(reads)
    uploaded.names = reads.names
    assert uploaded.to_bam(str(dev)) == dev.stat().st_size
    assert host.read_bytes() == dev.read_bytes()
    assert gzip.decompress(host.read_bytes()) == Bw.header_bytes() + Bw.expected_records(names, seqs, quals)
    assert G.write_bam(str(dev), uploaded, header="@CO\tx\n") == dev.stat().st_size
    assert gzip.decompress(dev.read_bytes()) == Bw.header_bytes(b"@CO\tx\n") + Bw.expected_records(names, seqs, quals)
    unnamed = tmp_path / "unnamed.bam"
    G.write_bam(str(unnamed), G.Reads(seqs, quals))
    assert gzip.decompress(unnamed.read_bytes()) == Bw.header_bytes() + Bw.expected_records(None, seqs, quals)


def test_another_encoding_is_refused(tmp_path):
    from sarlacc_amd import generics as G
    from sarlacc_amd._lib import SarlaccError
    from sarlacc_amd.encoding import illumina_encoding
    path = tmp_path / "illumina.bam"
    path.write_bytes(b"what it held")
    reads = G.Reads([b"ACGT"], [b"hhhh"], ["r"], illumina_encoding())
    with pytest.raises(SarlaccError, match="illumina"):
        G.write_bam(str(path), reads)
    with pytest.raises(SarlaccError, match="illumina"):
        device_batch([b"r"], [b"ACGT"], [b"hhhh"], illumina_encoding()).to_bam(str(path))
    assert path.read_bytes() == b"what it held"
