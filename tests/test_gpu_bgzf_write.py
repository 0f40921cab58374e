"""BGZF output deflated on the device (sarlacc_dev_bgzf_deflate, DeviceReads.to_fastq(compress=True),
generics.write_fastq(compress=True)).  Every decoded text is held byte for byte against text that does not come from the
code under test (a literal, a generator here, the host loop of generics.write_fastq), and is decoded by decoders that are
not the code under test: gzip.decompress (zlib: it also checks every member's CRC-32 and ISIZE), the Python inflate of
tests.bgzf_cases on the small texts, and the device inflate of the reader."""
import ctypes as C
import functools
import gzip
import heapq
import zlib

import numpy as np
import pytest

from tests import bgzf_write_cases as W
from tests.bgzf_cases import EOF_BLOCK, ref_inflate
from tests.test_gpu_fastq_write import draw, host_text, resident

pytestmark = pytest.mark.gpu

BLOCK, SLOT = W.BLOCK, 65536
MODES = (0, 1, 2)
GUARD = 37            # bytes of 0xEE either side of the output (odd: the output is not 16-byte aligned)
SHIFT = 3             # the text starts this far into its buffer


def _fastq(nbytes, L=150, seed=7):
    return W.synth_fastq(nbytes + 2 * L + 100, L, seed)[:nbytes]


def _long_read():
    """One record of 100 000 bases: the sequence line crosses the first block boundary, the quality line two more, and
    the third block (bytes 130 560 .. 195 840) holds no newline at all."""
    rng = np.random.default_rng(3)
    seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 100000)].tobytes()
    qual = rng.integers(40, 75, 100000).astype(np.uint8).tobytes()
    text = b"@r\n" + seq + b"\n+\n" + qual + b"\n"
    assert 10 not in text[2 * BLOCK:3 * BLOCK]
    return text


def _newline_edges():
    """Block 0 ends with a newline and block 1 begins with one."""
    body = _fastq(BLOCK - 1, 500, 9).replace(b"\n", b"N")
    text = body + b"\n" + b"\n" + _fastq(3000, 100, 10)
    assert text[BLOCK - 1] == 10 and text[BLOCK] == 10
    return text


def _among_lines(counts, seed):
    """One line of the limiter's bytes between ordinary 2 000-base records, all in one block."""
    line = W.spread(counts, seed)
    assert 10 not in line
    room = BLOCK - len(line) - 1
    rec = W.synth_fastq(room, 2000, 21)
    rec = rec[:rec.rfind(b"\n", 0, room // 2) + 1]
    text = rec + line + b"\n" + rec
    assert len(text) <= BLOCK
    return text


def _all_values():
    """One permutation of the 256 byte values, 255 times over: an LZ77 encoder makes little of it, a Huffman code
    nothing, and every line (256 bytes, from one newline to the next) holds every value once, so a table per line is
    no better."""
    return np.tile(np.random.default_rng(2).permutation(256).astype(np.uint8), 255).tobytes()


TEXTS = {
    "one byte": lambda: b"A",
    "fastq 65279": lambda: _fastq(BLOCK - 1),
    "fastq 65280": lambda: _fastq(BLOCK),
    "fastq 65281": lambda: _fastq(BLOCK + 1),
    "small fastq": lambda: _fastq(3000, 100, 5),
    "one value": lambda: b"G" * BLOCK,
    "random": lambda: np.random.default_rng(1).integers(0, 256, 200000).astype(np.uint8).tobytes(),
    "long read": _long_read,
    "no final newline": lambda: _fastq(3001, 100, 5)[:-1] + b"I",
    "newline edges": _newline_edges,
    "plus lines": lambda: b"+\n" * (BLOCK // 2),
    "fibonacci": lambda: W.spread(W.fibonacci_bytes(), 6),
    "deep": lambda: W.spread(W.deep_bytes(), 6),
    "fibonacci line": lambda: _among_lines(W.fibonacci_bytes(), 6),
    "deep line": lambda: _among_lines(W.deep_bytes(), 6),
    "length code limiter": lambda: W.spread(W.clen_limiter_bytes(), 5),
    "all values": _all_values,
}
NAMES = list(TEXTS)


@functools.lru_cache(maxsize=None)
def text_of(name):
    return TEXTS[name]()


def deflate_abi(text, mode):
    """sarlacc_dev_bgzf_deflate straight through the C ABI: the text at an odd offset of a guarded buffer, the output
    between guards of 0xEE.  Returns (compressed bytes, offsets, number of blocks); the guards are checked here."""
    from sarlacc_amd import _lib, bgzf
    from sarlacc_amd._lib import check
    from sarlacc_amd.resident import DevBuffer
    lib = _lib.lib()
    n_blocks, cap = bgzf.deflate_bound(len(text))
    src = np.full(SHIFT + len(text) + GUARD, 0xEE, np.uint8)
    src[SHIFT:SHIFT + len(text)] = np.frombuffer(text, np.uint8)
    d_src = DevBuffer.from_numpy(src)
    d_out = DevBuffer.from_numpy(np.full(cap + 2 * GUARD, 0xEE, np.uint8))
    d_off = DevBuffer.from_numpy(np.full(n_blocks + 2, -7, np.int64))
    total = C.c_int64(-1)
    check(lib.sarlacc_dev_bgzf_deflate(C.c_void_p(d_src.ptr.value + SHIFT), len(text), mode, C.c_void_p(d_out.ptr.value + GUARD),
                                       cap, d_off, C.byref(total), None))
    out = d_out.to_numpy(np.uint8, cap + 2 * GUARD)
    assert 0 <= total.value <= cap
    assert (out[:GUARD] == 0xEE).all() and (out[GUARD + total.value:] == 0xEE).all(), "bytes written outside the output"
    assert np.array_equal(d_src.to_numpy(np.uint8, src.size), src), "the text was changed"
    off = d_off.to_numpy(np.int64, n_blocks + 2)
    assert off[-1] == -7, "offsets written past n_blocks + 1 entries"
    return out[GUARD:GUARD + total.value].tobytes(), off[:-1].copy(), n_blocks


@functools.lru_cache(maxsize=None)
def encoded(name, mode):
    return deflate_abi(text_of(name), mode)


def sizes(name, mode):
    return np.diff(encoded(name, mode)[1])


def device_inflate(comp, comp_off, text_off):
    from sarlacc_amd import _lib
    from sarlacc_amd._lib import check
    from sarlacc_amd.resident import DevBuffer
    n, total = len(comp_off) - 1, int(text_off[-1])
    d_comp = DevBuffer.from_numpy(np.frombuffer(comp, np.uint8))
    d_co, d_to, d_text = DevBuffer.from_numpy(comp_off), DevBuffer.from_numpy(text_off), DevBuffer(max(total, 1))
    check(_lib.lib().sarlacc_dev_bgzf_inflate(d_comp, d_co, d_to, n, 0, d_text, 1, None))
    return d_text.to_numpy(np.uint8, total).tobytes()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", NAMES)
def test_blocks_decode_to_the_text(name, mode):
    from sarlacc_amd import bgzf
    text = text_of(name)
    comp, off, n_blocks = encoded(name, mode)
    assert n_blocks == -(-len(text) // BLOCK)
    n, used, comp_off, text_off, eof = bgzf.scan(comp)
    assert n == n_blocks and used == len(comp) and not eof
    assert np.array_equal(comp_off, off)
    assert text_off[-1] == len(text) and np.array_equal(np.diff(text_off), [len(p) for p in W.pieces(text)])
    assert np.diff(off).max() <= SLOT
    assert gzip.decompress(comp + EOF_BLOCK) == text
    assert device_inflate(comp, comp_off, text_off) == text
    if len(text) <= 3001:
        assert ref_inflate(comp[18:-8])[0] == text
    again, off2, _ = deflate_abi(text, mode)
    assert again == comp and np.array_equal(off2, off)


@pytest.mark.parametrize("name", NAMES)
def test_modes_only_ever_shrink_a_block(name):
    s0, s1, s2 = (sizes(name, m) for m in MODES)
    assert (s0 <= s1).all() and (s1 <= s2).all()
    assert np.array_equal(s2, [len(p) + 31 for p in W.pieces(text_of(name))])       # mode 2 stores


def test_random_bytes_are_stored():
    for mode in MODES:
        assert np.array_equal(sizes("random", mode), [len(p) + 31 for p in W.pieces(text_of("random"))])
        assert len(encoded("random", mode)[0]) == 200000 + 31 * 4


def _optimal_bits(counts):
    """Payload bits of an optimal prefix code over the counts (the sum of the merged weights: the same for every
    Huffman code, however ties fall)."""
    heap, bits = list(counts), 0
    heapq.heapify(heap)
    while len(heap) > 1:
        w = heapq.heappop(heap) + heapq.heappop(heap)
        bits += w
        heapq.heappush(heap, w)
    return bits


def test_all_values_by_the_exact_counts():
    """256 values of 255 bytes and end-of-block: the best code spends more bits on the payload alone than the stored block
    on everything, so stored must win in every mode."""
    text = text_of("all values")
    assert _optimal_bits([255] * 256 + [1]) + 17 > 8 * (len(text) + W.STORED)
    assert len(zlib.compress(text, 6)) < len(text) // 50              # compressible, but not by a Huffman code
    for mode in MODES:
        assert sizes("all values", mode).tolist() == [len(text) + 31]


def _first_table(name, mode):
    return W.first_table(encoded(name, mode)[0][18:])


def test_one_value_is_two_codes_of_one_bit():
    for mode in (0, 1):
        clens, used, lit, dist = _first_table("one value", mode)
        assert [(s, l) for s, l in enumerate(lit) if l] == [(ord("G"), 1), (256, 1)] and dist == [0]
        assert sizes("one value", mode).tolist() == [18 + -(-(3 + BLOCK + 1 + _header_bits(clens, used)) // 8) + 8]


def _header_bits(clens, used):
    """Bits of a table header from its code-length code and symbol counts: HLIT, HDIST, HCLEN, the 3-bit lengths up to
    the last one used, the symbols and their extra bits."""
    from tests.bgzf_cases import CLEN_ORDER
    hclen = max(4, max(i + 1 for i, s in enumerate(CLEN_ORDER) if clens[s]))
    return 14 + 3 * hclen + sum(u * l for u, l in zip(used, clens)) + 2 * used[16] + 3 * used[17] + 7 * used[18]


def _kraft(lens, limit):
    return sum(2 ** (limit - l) for l in lens if l), 2 ** limit


def test_the_literal_limiter_acts():
    """The deep block's unlimited code is 20 bits deep however ties fall: what comes out is a complete code of at most
    15 bits.  The Fibonacci block as well (22 byte values and end-of-block: 23 symbols, up to 22 bits deep; with ties
    broken towards the shallower tree it is less, so the deep block is the one that forces the limiter)."""
    for name, counts in (("deep", W.deep_bytes()), ("fibonacci", W.fibonacci_bytes())):
        for mode in (0, 1):
            clens, used, lit, dist = _first_table(name, mode)
            assert max(lit) <= 15 and dist == [0] and len(lit) == 257
            assert _kraft(lit, 15)[0] == _kraft(lit, 15)[1] and _kraft(clens, 7)[0] == _kraft(clens, 7)[1]
            assert {s for s, l in enumerate(lit) if l} == {v for v, _ in counts} | {256}
    assert max(_first_table("deep", 1)[2]) == 15
    # ... and inside the per-line candidate: the line among ordinary records is taken with tables of its own
    for name in ("deep line", "fibonacci line"):
        assert sizes(name, 0)[0] < sizes(name, 1)[0]


def test_the_length_code_limiter_acts():
    """The block whose code lengths are skewed (tests.bgzf_write_cases): the literal lengths are the dyadic ones, the
    header's symbol counts want a code 8 bits deep, and what comes out is a complete code of at most 7."""
    want = {v: 15 - (c.bit_length() - 1) for v, c in W.clen_limiter_bytes()}
    for mode in (0, 1):
        clens, used, lit, dist = _first_table("length code limiter", mode)
        assert all(lit[v] == want.get(v, 0) for v in range(256)) and lit[256] == 15
        assert W.huffman_depth(used) > 7
        assert max(clens) == 7 and _kraft(clens, 7)[0] == _kraft(clens, 7)[1]


def test_plus_lines_take_one_table():
    """32 640 lines of "+\\n": two literals and end-of-block under one table, 1 + 2 bits a line (12 240 bytes); a table
    per 64-byte piece cannot win, and the attempt ends without overflowing anything (the guards of deflate_abi)."""
    for mode in (0, 1):
        assert sizes("plus lines", mode)[0] < BLOCK // 4 + 100
    assert encoded("plus lines", 0)[0] == encoded("plus lines", 1)[0]


# ---- sizes against zlib on the generator's text ----------------------------------------------------------------------

TABLE_ROOM = 8 * 300      # 300 bytes for each of the 8 blocks


@functools.lru_cache(maxsize=None)
def seeded_total(L, mode):
    comp, off, n = deflate_abi(W.seeded_text(L), mode)
    assert gzip.decompress(comp + EOF_BLOCK) == W.seeded_text(L) and n == 8
    return len(comp)


def test_long_reads_beat_zlib_level_6():
    y = W.yardsticks(2000)
    got = seeded_total(2000, 0)
    print("2 000-base reads, mode 0: %d bytes; zlib level 6 %d (ratio %.4f), zlib Huffman-only per line %d (ratio %.4f)"
          % (got, y["level6"], got / y["level6"], y["per_line"], got / y["per_line"]))
    assert got <= y["level6"]


@pytest.mark.parametrize("mode", (0, 1))
def test_short_reads_take_one_table(mode):
    """At most one table written without any repeat symbol (19 * 3 + 316 * 7 bits = 300 bytes) above zlib's Huffman-only
    stream; zlib's per-line stream is 18 % larger than that, so mode 0 cannot have taken per-line tables."""
    y = W.yardsticks(100)
    got = seeded_total(100, mode)
    print("100-base reads, mode %d: %d bytes; zlib Huffman-only %d (ratio %.4f)" % (mode, got, y["huffman"], got / y["huffman"]))
    assert got <= y["huffman"] + TABLE_ROOM
    assert y["per_line"] > y["huffman"] + TABLE_ROOM


def test_long_reads_one_table_and_the_gain_of_per_line_tables():
    y = W.yardsticks(2000)
    one, per_line = seeded_total(2000, 1), seeded_total(2000, 0)
    print("2 000-base reads, mode 1: %d bytes; zlib Huffman-only %d (ratio %.4f); mode 0 %d" % (one, y["huffman"], one / y["huffman"], per_line))
    assert one <= y["huffman"] + TABLE_ROOM
    assert one > per_line


# ---- DeviceReads.to_fastq(compress=True) and generics.write_fastq(compress=True) --------------------------------------

def _reads(seed, lengths):
    from sarlacc_amd import generics as G
    names, seqs, quals = draw(np.random.default_rng(seed), lengths)
    return G.Reads(seqs, quals, names)


@pytest.fixture(scope="module")
def drawn(tmp_path_factory):
    """60 reads of 0 - 5 000 bases with names, an empty one among them: (Reads, the host loop's text)."""
    rng = np.random.default_rng(31)
    lengths = rng.integers(0, 5001, 60)
    lengths[7] = 0
    reads = _reads(32, lengths)
    return reads, host_text(tmp_path_factory.mktemp("drawn"), reads)


def _check_file(path, written, want):
    from sarlacc_amd import bgzf
    data = path.read_bytes()
    assert written == len(data)
    assert bgzf.sniff(str(path)) == bgzf.BGZF and data.endswith(EOF_BLOCK)
    assert gzip.decompress(data) == want
    n, used, _, text_off, eof = bgzf.scan(data)
    assert used == len(data) and eof and text_off[-1] == len(want)


def test_to_fastq_compressed(drawn, tmp_path):
    from sarlacc_amd import generics as G
    reads, want = drawn
    assert len(want) > 2 * BLOCK
    dev = resident(reads)
    path = tmp_path / "reads.fastq.gz"
    _check_file(path, dev.to_fastq(str(path), compress=True), want)
    whole = path.read_bytes()
    for block_bytes in (1000, None):
        _check_file(path, dev.to_fastq(str(path), block_bytes=block_bytes, compress=True), want)
    assert dev.to_fastq(str(path), block_bytes=None, compress=True) == len(whole) and path.read_bytes() == whole
    _check_file(path, G.write_fastq(str(path), dev, compress=True), want)
    # a batch of one
    one = _reads(33, [700])
    _check_file(path, resident(one).to_fastq(str(path), compress=True), host_text(tmp_path, one, "one"))


def test_plain_output_is_what_it_was(drawn, tmp_path):
    """compress=False, given or left out, and whatever the file is called: the host loop's bytes."""
    from sarlacc_amd import generics as G
    reads, want = drawn
    dev = resident(reads)
    path = tmp_path / "plain.fastq.gz"
    assert dev.to_fastq(str(path)) == len(want) and path.read_bytes() == want
    assert dev.to_fastq(str(path), compress=False, block_bytes=5000) == len(want) and path.read_bytes() == want
    assert G.write_fastq(str(path), dev, compress=False) == len(want) and path.read_bytes() == want
    G.write_fastq(str(path), reads, compress=False)
    assert path.read_bytes() == want


def test_default_names_compressed(tmp_path):
    from sarlacc_amd import generics as G
    from sarlacc_amd.resident import DeviceReads
    _, seqs, quals = draw(np.random.default_rng(34), np.random.default_rng(35).integers(0, 300, 120))
    reads = G.Reads(seqs, quals)
    want = host_text(tmp_path, reads)
    assert b"@READ_120\n" in want
    dev = DeviceReads.upload(reads)
    assert dev.names is None
    path = tmp_path / "default.gz"
    _check_file(path, dev.to_fastq(str(path), compress=True), want)


def test_empty_batch_compressed(tmp_path):
    from sarlacc_amd import generics as G
    from sarlacc_amd.resident import DeviceReads
    path = tmp_path / "empty.gz"
    path.write_bytes(b"old")
    assert DeviceReads.upload(G.Reads([], [])).to_fastq(str(path), compress=True) == 28
    assert path.read_bytes() == EOF_BLOCK and gzip.decompress(path.read_bytes()) == b""
    assert G.write_fastq(str(path), G.Reads([], []), compress=True) == 28 and path.read_bytes() == EOF_BLOCK


def test_append_compressed(drawn, tmp_path):
    """Two appends onto a compressed file: the text is the concatenation (the earlier end-of-file blocks stay in the
    middle as empty members), and the device reader returns every read."""
    from sarlacc_amd.resident import DeviceReads
    reads, want = drawn
    more = _reads(36, [0, 1, 4000, 250])
    want_more = host_text(tmp_path, more, "more")
    path = tmp_path / "grown.gz"
    first = resident(reads).to_fastq(str(path), compress=True)
    second = resident(more).to_fastq(str(path), append=True, compress=True, block_bytes=3000)
    third = resident(reads).to_fastq(str(path), append=True, compress=True)
    data = path.read_bytes()
    assert len(data) == first + second + third and third == first
    assert data.count(EOF_BLOCK) >= 3 and data.endswith(EOF_BLOCK)
    assert gzip.decompress(data) == want + want_more + want
    back = DeviceReads.from_fastq(str(path))
    seq, qual = back.download()
    assert list(back.names) == reads.names + more.names + reads.names
    assert seq.to_strings() == reads.seq.to_strings() + more.seq.to_strings() + reads.seq.to_strings()
    assert qual.to_strings() == reads.qual.to_strings() + more.qual.to_strings() + reads.qual.to_strings()


def test_refusal_compressed(tmp_path):
    from sarlacc_amd import generics as G
    from sarlacc_amd._lib import SarlaccError
    names, seqs, quals = draw(np.random.default_rng(37), [30, 40, 50, 60])
    names[2] = "a\nb"
    reads = G.Reads(seqs, quals, names)
    path = tmp_path / "bad.gz"
    for writer in (lambda **kw: resident(reads).to_fastq(str(path), compress=True, **kw),
                   lambda **kw: G.write_fastq(str(path), reads, compress=True, **kw)):
        with pytest.raises(SarlaccError, match="record 3: read name holds a line break"):
            writer()
        assert not path.exists()
        path.write_bytes(EOF_BLOCK)
        with pytest.raises(SarlaccError, match="record 3: read name holds a line break"):
            writer(append=True)
        assert path.read_bytes() == EOF_BLOCK
        path.unlink()


def test_host_reads_compressed(drawn, tmp_path):
    from sarlacc_amd import generics as G
    reads, want = drawn
    path = tmp_path / "host.gz"
    _check_file(path, G.write_fastq(str(path), reads, compress=True), want)
    unnamed = G.Reads(reads.seq.to_strings()[:5], reads.qual.to_strings()[:5])
    _check_file(path, G.write_fastq(str(path), unnamed, compress=True), host_text(tmp_path, unnamed, "unnamed"))


def test_other_encoding_round_trip(tmp_path):
    """Quality names at and above byte 128: literals like any other."""
    from sarlacc_amd import generics as G
    from sarlacc_amd.resident import DeviceReads
    from tests.encodings import BY_NAME, draw_quals
    table = BY_NAME["n128_high"]
    rng = np.random.default_rng(38)
    lengths = rng.integers(0, 3001, 40)
    names, seqs, _ = draw(rng, lengths)
    quals = draw_quals(table, lengths, 38)
    flat = np.frombuffer(b"".join(quals), dtype=np.uint8)
    assert (flat >= 128).any() and flat.max() == 255 and not np.isin(flat, (10, 13)).any()
    want = b"".join(b"@" + nm.encode() + b"\n" + s.encode() + b"\n+\n" + q + b"\n" for nm, s, q in zip(names, seqs, quals))
    dev = resident(G.Reads(seqs, quals, names, encoding=table.enc))
    path = tmp_path / "high.gz"
    _check_file(path, dev.to_fastq(str(path), compress=True), want)
    back = DeviceReads.from_fastq(str(path), encoding=table.enc)
    assert back.fastq_text() == want
    assert back.download()[1].chars[:flat.size].tobytes() == flat.tobytes()


def test_bad_requests():
    from sarlacc_amd import _lib, bgzf
    from sarlacc_amd.resident import DevBuffer
    d = DevBuffer.from_numpy(np.frombuffer(b"ACGT\n" * 10, np.uint8))
    with pytest.raises(_lib.SarlaccError, match="unknown BGZF deflate mode 3"):
        bgzf.deflate_device(d, 50, mode=3)
    with pytest.raises(_lib.SarlaccError, match="negative"):
        bgzf.deflate_device(d, -1)
    with pytest.raises(_lib.SarlaccError, match="capacity 100 is below the bound 65536"):
        bgzf.deflate_device(d, 50, out=DevBuffer(100))
    total = C.c_int64(-1)
    _lib.check(_lib.lib().sarlacc_dev_bgzf_deflate(d, 0, 0, None, 0, None, C.byref(total), None))
    assert total.value == 0
    buf, nbytes = bgzf.deflate_device(d, 50)
    assert gzip.decompress(buf.to_numpy(np.uint8, nbytes).tobytes()) == b"ACGT\n" * 10
