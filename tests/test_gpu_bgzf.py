"""BGZF input on the device (bgzf.hip, sarlacc_amd/bgzf.py): the inflate kernel against Python's zlib on every block
type and copy shape and on hand-built streams at deflate's limits (tests/bgzf_cases.py; tests/test_bgzf_streams.py shows
on the CPU that they contain what they claim), its refusals of malformed input, and the compressed routes of from_fastq / stream_fastq /
adaptorAlign / realizeReads / sam2ranges against the same calls on the text.  Byte work: everything must be
identical."""
import gzip
import re
import struct
import zlib

import numpy as np
import pytest

from tests import bgzf_cases as B

pytestmark = pytest.mark.gpu

GUARD = 64


def inflate(data, check_crc=1, first_block=0, n_blocks=None, text_off=None):
    """One sarlacc_dev_bgzf_inflate call on the blocks of `data`; returns the text and checks the 64 guard bytes of
    0xA5 on either side, also when the call fails."""
    from sarlacc_amd import _lib, bgzf
    from sarlacc_amd.resident import DevBuffer
    n, used, comp_off, toff, _ = bgzf.scan(data)
    assert used == len(data)
    if n_blocks is not None:
        n, comp_off, toff = n_blocks, comp_off[:n_blocks + 1], toff[:n_blocks + 1]
    if text_off is not None:
        toff = np.asarray(text_off, np.int64)
    total = int(toff[-1])
    host = np.full(total + 2 * GUARD, 0xA5, np.uint8)
    d_text = DevBuffer.from_numpy(host)
    d_comp, d_co, d_to = DevBuffer.from_numpy(np.frombuffer(data, np.uint8)), DevBuffer.from_numpy(comp_off), DevBuffer.from_numpy(toff)
    rc = _lib.lib().sarlacc_dev_bgzf_inflate(d_comp, d_co, d_to, n, first_block, d_text.ptr.value + GUARD, check_crc, None)
    got = d_text.to_numpy(np.uint8, host.size)
    assert (got[:GUARD] == 0xA5).all() and (got[GUARD + total:] == 0xA5).all(), "guard bytes were written"
    _lib.check(rc)
    return got[GUARD:GUARD + total].tobytes()


def all_kinds():
    rng = np.random.default_rng(1951)

    def dna(n):
        return rng.choice(np.frombuffer(b"ACGTN\n", np.uint8), n, p=[0.24, 0.24, 0.24, 0.24, 0.02, 0.02]).tobytes()
    p = rng.integers(0, 256, 32768, dtype=np.uint8).tobytes()
    r3, r70 = rng.integers(0, 256, 3, dtype=np.uint8).tobytes(), rng.integers(0, 256, 70, dtype=np.uint8).tobytes()
    r63, r65 = r70[:63], r70[:65]
    every = bytes(range(256)) * 5 + rng.permutation(np.arange(256, dtype=np.uint8)).tobytes() * 3
    D, S = zlib.Z_DEFAULT_STRATEGY, None
    cases = [
        ("stored", dna(4001), 0, D, S), ("fixed", dna(3001), 6, zlib.Z_FIXED, S),
        ("level 1", dna(20011), 1, D, S), ("level 6", dna(30013), 6, D, S), ("level 9", dna(65001), 9, D, S),
        ("huffman only", dna(9007), 6, zlib.Z_HUFFMAN_ONLY, S), ("rle", dna(5003) + b"\0" * 777 + dna(11), 6, zlib.Z_RLE, S),
        ("full flush", dna(20000), 6, D, 7000), ("empty", b"", 6, D, S), ("one byte", b"Q", 6, D, S),
        ("random", rng.integers(0, 256, 0xff00, dtype=np.uint8).tobytes(), 6, D, S),
        ("run", b"A" * 0xff00, 6, D, S), ("far", p + p[:30000], 9, D, S),
        ("period 3", r3 * 1667, 6, D, S), ("period 63", r63 * 41, 9, D, S), ("period 65", r65 * 41, 9, D, S),
        ("period 70", r70 * 101, 6, D, S), ("every byte", every, 6, D, S), ("flush at 1", dna(777), 6, D, 1),
    ]
    out = [(name, data, B.bgzf_block(data, level, strategy, flush_at)) for name, data, level, strategy, flush_at in cases]
    # zlib looks back 32 506 bytes at the most
    q = p[:32500]
    out.append(("far by zlib", q + q[:30000], B.bgzf_block(q + q[:30000], 9)))
    # by hand: the largest distance and length, and matches fed by tokens a few places before them
    tokens = list(p) + [(258, 32768), (3, 32768), (258, 1), (100, 32768), 7, 8, (5, 2), (10, 7), (258, 9), (64, 63), (65, 64), (130, 65),
                        (3, 1), (4, 4), 9, (258, 258), (258, 259), (31, 33000 - 232)]
    raw = B.fixed_stream(tokens)
    text = zlib.decompress(raw, -15)
    out.append(("by hand", text, B.wrap(raw, zlib.crc32(text), len(text))))
    return out


@pytest.fixture(scope="module")
def kinds():
    return all_kinds()


def test_every_block_kind_in_one_call(kinds):
    assert zlib.decompress(kinds[0][2][18:-8], -15) == kinds[0][1] and kinds[0][2][18] & 6 == 0          # stored
    assert kinds[1][2][18] & 6 == 2                                                                      # fixed Huffman
    assert all(k[2][18] & 6 == 4 for k in kinds[2:7])                                                    # dynamic Huffman
    assert len(kinds[10][2]) == 65316 and kinds[10][2][18] & 6 == 0                            # random bytes: stored
    data = B.bgzf_file(*[k[2] for k in kinds])
    want = b"".join(k[1] for k in kinds)
    starts = np.cumsum([0] + [len(k[1]) for k in kinds])
    assert len(set(int(s) % 16 for s in starts)) >= 8, "the outputs should start at many alignments"
    got = inflate(data)
    for (name, text, _), a, b in zip(kinds, starts, starts[1:]):
        assert got[a:b] == text, name
    assert got == want == gzip.decompress(data)
    assert inflate(data, check_crc=0) == want


def test_no_block_and_one_block(kinds):
    data = B.bgzf_file(kinds[3][2], kinds[1][2])
    assert inflate(data, n_blocks=0) == b""
    assert inflate(data, n_blocks=1) == kinds[3][1]
    assert inflate(B.EOF_BLOCK) == b""


def _refused(data, reason, block=1, **kw):
    from sarlacc_amd._lib import SarlaccError
    with pytest.raises(SarlaccError) as e:
        inflate(data, **kw)
    assert str(e.value) == "BGZF block %d: %s" % (block, reason)
    # the library is usable again
    assert inflate(B.bgzf_file(B.bgzf_block(b"still works " * 50))) == b"still works " * 50


def test_error_names_the_block_counted_from_first_block():
    bad = bytearray(B.bgzf_block(b"payload " * 40, 0))
    bad[40] ^= 1
    _refused(bytes(bad), "CRC32 mismatch", block=6, first_block=5)
    good = B.bgzf_block(b"fine " * 100)
    _refused(good + good + bytes(bad) + good + bytes(bad), "CRC32 mismatch", block=3)       # the lowest failing block


def test_crc_and_length_checks():
    text = b"payload " * 40
    bad = bytearray(B.bgzf_block(text, 0))
    bad[40] ^= 1
    _refused(bytes(bad), "CRC32 mismatch")
    flipped = bytearray(text)
    flipped[40 - 18 - 5] ^= 1
    assert inflate(bytes(bad), check_crc=0) == bytes(flipped)
    for level in (0, 6):
        longer = bytearray(B.bgzf_block(text, level))
        longer[-4:] = struct.pack("<I", len(text) + 1)                # ISIZE raised by one; text_off follows it
        _refused(bytes(longer), "length mismatch")
        _refused(bytes(longer), "length mismatch", check_crc=0)
        shorter = bytearray(B.bgzf_block(text, level))
        shorter[-4:] = struct.pack("<I", len(text) - 1)
        _refused(bytes(shorter), "output exceeds the size field")
    # the size field and text_off disagree: only the check finds it
    _refused(B.bgzf_block(text), "length mismatch", text_off=[0, len(text) + 1])


@pytest.mark.parametrize("name", sorted(B.malformed()))
def test_malformed_deflate_streams(name):
    _refused(B.malformed_block(name), B.malformed()[name][2])
    _refused(B.malformed_block(name), B.malformed()[name][2], check_crc=0)


def test_truncated_dynamic_block_and_bad_frame():
    rng = np.random.default_rng(3)
    text = rng.choice(np.frombuffer(b"ACGT", np.uint8), 5000).tobytes()
    raw = B.deflate_raw(text, 6)
    for keep in (len(raw) // 2, 40, 3):
        _refused(B.wrap(raw[:keep], zlib.crc32(text), len(text)), "compressed data ends early")
    # reserved block type
    _refused(B.wrap(B.BitWriter().value(1, 1).value(3, 2).value(0, 13).bytes(), 0, 0), "invalid stored block")
    # a length symbol outside the defined range: fixed code 11000110 is symbol 286
    _refused(B.wrap(B.BitWriter().value(1, 1).value(1, 2).code(0xc6, 8).value(0, 16).bytes(), 0, 4), "invalid symbol")


# ---- hand-built streams ---------------------------------------------------------------------------------------------
def inflate_at(data, comp_off, text_off, first_block=0, check_crc=1):
    """One call on the blocks that the two offset lists name, `data` and the text buffer being those of the whole file;
    returns the failure's message (None: success) and the whole buffer with its 64 guard bytes on either side."""
    from sarlacc_amd import _lib
    from sarlacc_amd._lib import SarlaccError
    from sarlacc_amd.resident import DevBuffer
    comp_off, text_off = np.asarray(comp_off, np.int64), np.asarray(text_off, np.int64)
    host = np.full(int(text_off[-1]) + 2 * GUARD, 0xA5, np.uint8)
    d_text = DevBuffer.from_numpy(host)
    d_comp, d_co, d_to = DevBuffer.from_numpy(np.frombuffer(data, np.uint8)), DevBuffer.from_numpy(comp_off), DevBuffer.from_numpy(text_off)
    rc = _lib.lib().sarlacc_dev_bgzf_inflate(d_comp, d_co, d_to, len(comp_off) - 1, first_block, d_text.ptr.value + GUARD, check_crc, None)
    got = d_text.to_numpy(np.uint8, host.size)
    try:
        _lib.check(rc)
    except SarlaccError as e:
        return str(e), got
    return None, got


def _block_by_block(items, check_crc):
    """items: (name, text, block).  One call on all of them, every block's text compared on its own."""
    data = B.bgzf_file(*[block for _, _, block in items])
    got = inflate(data, check_crc=check_crc)
    starts = np.cumsum([0] + [len(text) for _, text, _ in items])
    for (name, text, _), a, b in zip(items, starts, starts[1:]):
        assert got[a:b] == text, name
    assert len(got) == starts[-1]
    return starts


def test_named_streams_in_one_call():
    items = [(name, text, block) for _, name, _, text, block in B.named_streams()]
    starts = _block_by_block(items, 1)
    assert len(set(int(s) % 16 for s in starts)) >= 8, "the outputs should start at many alignments"
    _block_by_block(items, 0)


def test_named_streams_one_call_each():
    for _, name, _, text, block in B.named_streams():
        assert inflate(block) == text, name


def test_generated_streams():
    items = [("generated %d" % k, text, block) for k, (_, text, block) in enumerate(B.generated_streams())]
    _block_by_block(items, 1)
    # from block 100 on: the offsets are those of the whole file, so they do not start at zero
    comp_off = np.asarray(B.block_offsets([block for _, _, block in items]), np.int64)
    text_off = np.asarray(B.block_offsets([text for _, text, _ in items]), np.int64)
    message, got = inflate_at(b"".join(block for _, _, block in items), comp_off[100:], text_off[100:], first_block=100)
    assert message is None
    assert (got[:GUARD + text_off[100]] == 0xA5).all() and (got[GUARD + text_off[-1]:] == 0xA5).all()
    for (name, text, _), a, b in zip(items[100:], text_off[100:], text_off[101:]):
        assert got[GUARD + a:GUARD + b].tobytes() == text, name


@pytest.mark.parametrize("name", sorted(B.refusals()))
def test_refusals_held_against_zlib(name):
    reason = B.refusals()[name][2]
    _refused(B.refusal_block(name), reason)
    _refused(B.refusal_block(name), reason, check_crc=0)


def test_blocks_do_not_see_each_others_text():
    # the first block ends in a run of A; a match at distance 1 that opens the second block must not reach it
    data = B.bgzf_block(b"A" * 100, 0) + B.refusal_block("a match opens the block")
    for check_crc in (1, 0):
        _refused(data, "distance beyond the start of the block", block=2, check_crc=check_crc)


@pytest.mark.parametrize("name", B.OVERFLOWS)
def test_overflow_writes_nothing_outside_the_refused_block(name):
    rng = np.random.default_rng(5)
    one, three = rng.integers(0, 256, 333, dtype=np.uint8).tobytes(), rng.integers(0, 256, 77, dtype=np.uint8).tobytes()
    blocks = [B.bgzf_block(one), B.refusal_block(name), B.bgzf_block(three)]
    size = B.refusals()[name][1]
    text_off = [0, len(one), len(one) + size, len(one) + size + len(three)]
    for check_crc in (1, 0):
        message, got = inflate_at(b"".join(blocks), B.block_offsets(blocks), text_off, check_crc=check_crc)
        assert message == "BGZF block 2: output exceeds the size field"
        assert (got[:GUARD] == 0xA5).all() and (got[GUARD + text_off[-1]:] == 0xA5).all(), "guard bytes were written"
        assert got[GUARD:GUARD + len(one)].tobytes() == one and got[GUARD + text_off[2]:GUARD + text_off[3]].tobytes() == three


# ---- FASTQ ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fastq(tmp_path_factory):
    from tests.test_gpu_fastq import fastq_text
    d = tmp_path_factory.mktemp("bgzf_fastq")
    text = fastq_text(np.random.default_rng(77), 300, 0, 700)
    half = text.index(b"\n@read_150 ") + 1
    paths = {"text": d / "r.fastq", "bgzf": d / "r.fastq.gz", "gzip": d / "two_members.fastq.gz", "no eof": d / "n.fastq.gz"}
    paths["text"].write_bytes(text)
    paths["bgzf"].write_bytes(B.bgzf_compress(text, block=5000))
    paths["no eof"].write_bytes(B.bgzf_compress(text, block=4999, eof=False))
    paths["gzip"].write_bytes(gzip.compress(text[:half - 100]) + gzip.compress(text[half - 100:]))
    return {k: str(v) for k, v in paths.items()}


def _same_batch(a, b):
    assert len(a) == len(b) and a.names == b.names
    for x, y in zip(a.download(), b.download()):
        assert np.array_equal(x.off, y.off) and np.array_equal(x.chars[:x.off[-1]], y.chars[:y.off[-1]])


@pytest.mark.parametrize("kind", ["bgzf", "gzip", "no eof"])
def test_from_fastq_of_a_compressed_file(fastq, kind):
    from sarlacc_amd.resident import DeviceReads
    want = DeviceReads.from_fastq(fastq["text"])
    assert len(want) == 300
    _same_batch(DeviceReads.from_fastq(fastq[kind]), want)


def test_from_fastq_of_hand_built_blocks(fastq, tmp_path):
    """Every sequence line under the ladder codes (1 ... 14, 15, 15 bits on both alphabets), the other lines as stored and
    fixed blocks: some 80 deflate blocks to a BGZF block."""
    from sarlacc_amd.resident import DeviceReads
    with open(fastq["text"], "rb") as fh:
        text = fh.read()
    data = B.handbuilt_fastq(text, records=20)
    assert gzip.decompress(data) == text
    (tmp_path / "hand.fastq.gz").write_bytes(data)
    want = DeviceReads.from_fastq(fastq["text"])
    assert len(want) == 300
    _same_batch(DeviceReads.from_fastq(str(tmp_path / "hand.fastq.gz")), want)


@pytest.mark.parametrize("kind", ["bgzf", "gzip", "no eof"])
def test_stream_fastq_of_a_compressed_file(fastq, kind):
    from sarlacc_amd.resident import DeviceReads
    for number, block_bytes in ((7, 12_000), (300, 5_000), (1000, 1 << 20)):
        want = list(DeviceReads.stream_fastq(fastq["text"], number, block_bytes=block_bytes))
        got = list(DeviceReads.stream_fastq(fastq[kind], number, block_bytes=block_bytes))
        assert len(got) == len(want) == -(-300 // number)
        for a, b in zip(got, want):
            _same_batch(a, b)


def test_record_error_in_a_compressed_file(tmp_path):
    from sarlacc_amd import bgzf
    from sarlacc_amd._lib import SarlaccError
    from sarlacc_amd.resident import DeviceReads
    text = b"".join(b"@r%d\nACGT\n+\nIIII\n" % k for k in range(40)).replace(b"@r25\n", b"r25\n")
    (tmp_path / "t.fastq").write_bytes(text)
    (tmp_path / "t.fastq.gz").write_bytes(B.bgzf_compress(text, block=100))
    for call in (lambda p: DeviceReads.from_fastq(p), lambda p: list(DeviceReads.stream_fastq(p, 10, block_bytes=150))):
        messages = []
        for name in ("t.fastq", "t.fastq.gz"):
            with pytest.raises(SarlaccError) as e:
                call(str(tmp_path / name))
            messages.append(str(e.value))
        assert messages[0] == messages[1] and "does not start with '@'" in messages[0]
    # a damaged block is named by its number in the file
    data = bytearray(B.bgzf_compress(text, block=100))
    second = len(B.bgzf_block(text[:100]))
    data[second + 30] ^= 0x55
    (tmp_path / "d.fastq.gz").write_bytes(bytes(data))
    with pytest.raises(SarlaccError, match="^BGZF block 2: "):
        DeviceReads.from_fastq(str(tmp_path / "d.fastq.gz"))
    # a file cut inside its last block of text (the end-of-file block is 28 bytes)
    good = B.bgzf_compress(text.replace(b"\nr25\n", b"\n@r25\n"), block=100)
    (tmp_path / "c.fastq.gz").write_bytes(good[:-40])
    with pytest.raises(SarlaccError, match="file ends inside BGZF block %d" % bgzf.scan(good[:-28])[0]):
        list(DeviceReads.stream_fastq(str(tmp_path / "c.fastq.gz"), 10, block_bytes=150))


def test_adaptor_align_filter_and_realize_from_a_compressed_path(tmp_path):
    from sarlacc_amd import generics as G
    from sarlacc_amd.mock import mock_reads
    from tests.test_gpu_fastq import A1, A2
    sim = mock_reads(A1, A2, nmolecules=10, nreads=6, seqlen=400, seed=1000)
    reads = G.Reads(sim["reads"], sim["quals"], ["READ_%d" % (i + 1) for i in range(len(sim["reads"]))])
    assert len(sim["reads"]) == 60
    path, gz = tmp_path / "mock.fastq", tmp_path / "mock.fastq.gz"
    G.write_fastq(str(path), reads)
    gz.write_bytes(B.bgzf_compress(path.read_bytes(), block=5000))
    a = G.adaptorAlign(A1, A2, str(path), tolerance=120, number=25)
    b = G.adaptorAlign(A1, A2, str(gz), tolerance=120, number=25)
    assert b["metadata"]["filepath"] == str(gz) and b["names"] == a["names"]
    assert np.array_equal(a["read.width"], b["read.width"]) and np.array_equal(a["reversed"], b["reversed"])
    for key in ("adaptor1", "adaptor2"):
        assert sorted(a[key]) == sorted(b[key])
        assert np.array_equal(a[key]["score"].view(np.int64), b[key]["score"].view(np.int64))
        assert np.array_equal(a[key]["start"], b[key]["start"]) and np.array_equal(a[key]["end"], b[key]["end"])
        assert a[key]["subseq"] == b[key]["subseq"]
    fa, fb = G.filterReads(a, 6, 6), G.filterReads(b, 6, 6)
    assert fa["names"] == fb["names"] and len(fa["read.width"]) == len(fb["read.width"]) > 30 and fb["metadata"]["filepath"] == str(gz)
    ra, rb = G.realizeReads(fa, number=25), G.realizeReads(fb, number=25)
    assert ra.names == rb.names and ra.seq.to_strings() == rb.seq.to_strings() and ra.qual.to_strings() == rb.qual.to_strings()


# ---- SAM -----------------------------------------------------------------------------------------------------------
def test_sam2ranges_of_a_compressed_file(tmp_path):
    from sarlacc_amd import SarlaccError, generics
    from tests import sam_restated as R
    from tests.test_gpu_sam import REFS, header, record
    rng = np.random.default_rng(11)
    refs = REFS + ["extra_contig_%04d" % k for k in range(400)]
    head = header(refs)
    assert len(head) > 10_000                      # the header spans more than one 5 000-byte block
    lines = [record(rng, i, refs) for i in range(1500)]
    text = (head + "\n".join(lines) + "\n").encode()

    def run(data, name, **kw):
        p = tmp_path / name
        p.write_bytes(data)
        return R.as_table(generics.sam2ranges(str(p), **kw))
    want = run(text, "t.sam", block_bytes=20_000)
    assert len(want["names"]) > 300
    assert run(B.bgzf_compress(text, block=5000), "t.sam.gz", block_bytes=20_000) == want
    assert run(B.bgzf_compress(text, block=5000, eof=False), "n.sam.gz", minq=10) == want
    assert run(B.bgzf_compress(text[:-1], block=len(head)), "b.sam.gz", block_bytes=3_000) == want    # the body starts a block
    assert run(gzip.compress(text), "p.sam.gz", block_bytes=20_000) == want
    for restricted in (["chr2", "nowhere"],):
        assert run(B.bgzf_compress(text, block=5000), "r.sam.gz", minq=None, restricted=restricted, block_bytes=20_000) == \
            run(text, "r.sam", minq=None, restricted=restricted)
    # header only, and nothing at all
    assert run(B.bgzf_compress(head.encode(), block=5000), "h.sam.gz") == run(head.encode(), "h.sam")
    assert run(B.bgzf_compress((head + "\n\r\n").encode(), block=5000), "e.sam.gz") == run((head + "\n\r\n").encode(), "e.sam")
    # a bad record: the same file line in both
    lines[1200] = "bad\t0\tchr1\t1\t60\t5S"
    bad = (head + "\n".join(lines) + "\n").encode()
    messages = []
    for data, name in ((bad, "bad.sam"), (B.bgzf_compress(bad, block=5000), "bad.sam.gz")):
        with pytest.raises(SarlaccError) as e:
            run(data, name, block_bytes=20_000)
        messages.append(str(e.value))
    assert messages[0] == messages[1] and re.match("SAM line %d: " % (head.count("\n") + 1201), messages[0])
