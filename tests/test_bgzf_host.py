"""BGZF input, the part that needs no device: the host block scan (sarlacc_bgzf_scan), the sniffing of text / gzip /
BGZF, the host FASTQ reader on compressed files, and the hand-made malformed deflate streams of the GPU test held
against zlib."""
import gzip
import struct
import zlib

import numpy as np
import pytest

from sarlacc_amd import bgzf, generics
from sarlacc_amd._lib import SarlaccError
from tests import bgzf_cases as B

RNG = np.random.default_rng(20)


def _ten_blocks():
    texts = [RNG.integers(65, 70, size=n, dtype=np.uint8).tobytes() for n in (1, 700, 0, 4999, 65280, 3, 1234, 77, 20000, 5)]
    return texts, [B.bgzf_block(t) for t in texts]


def test_builder_round_trips_through_gzip():
    texts, blocks = _ten_blocks()
    assert gzip.decompress(B.bgzf_file(*blocks)) == b"".join(texts)
    data = RNG.integers(0, 256, size=20000, dtype=np.uint8).tobytes()
    assert gzip.decompress(B.bgzf_block(data, 6, zlib.Z_DEFAULT_STRATEGY, flush_at=7000)) == data


def test_scan_reports_the_builders_offsets():
    texts, blocks = _ten_blocks()
    n, used, comp_off, text_off, eof = bgzf.scan(B.bgzf_file(*blocks, eof=False))
    assert n == 10 and used == sum(map(len, blocks)) and not eof
    assert comp_off.tolist() == B.block_offsets(blocks)
    assert text_off.tolist() == np.concatenate([[0], np.cumsum([len(t) for t in texts])]).tolist()


def test_buffer_cut_inside_a_block():
    _, blocks = _ten_blocks()
    whole = B.bgzf_file(*blocks)
    three = sum(map(len, blocks[:3]))
    for extra in (1, 11, 12, 17, 18, len(blocks[3]) - 1):
        n, used, comp_off, _, _ = bgzf.scan(whole[:three + extra])
        assert (n, used) == (3, three) and comp_off.tolist() == B.block_offsets(blocks[:3])
    assert bgzf.scan(b"")[:2] == (0, 0)


def test_max_blocks_is_respected():
    texts, blocks = _ten_blocks()
    n, used, comp_off, text_off, _ = bgzf.scan(B.bgzf_file(*blocks), max_blocks=4)
    assert n == 4 and used == sum(map(len, blocks[:4])) and len(comp_off) == 5
    assert text_off[-1] == sum(len(t) for t in texts[:4])
    assert bgzf.scan(B.bgzf_file(*blocks), max_blocks=0)[:2] == (0, 0)


def test_other_extra_subfields_are_skipped():
    before, after = b"AB\x03\x00xyz", b"ZZ\x00\x00" + b"RG\x05\x00hello"
    blocks = [B.bgzf_block(b"first", before=before), B.bgzf_block(b"second", after=after),
              B.bgzf_block(b"third", before=before, after=after)]
    assert gzip.decompress(b"".join(blocks)) == b"firstsecondthird"
    n, used, comp_off, text_off, _ = bgzf.scan(b"".join(blocks))
    assert n == 3 and comp_off.tolist() == B.block_offsets(blocks) and text_off.tolist() == [0, 5, 11, 16]


def test_end_of_file_flag():
    blk = B.bgzf_block(b"text")
    assert bgzf.scan(blk + B.EOF_BLOCK)[4] is True
    assert bgzf.scan(B.EOF_BLOCK + blk)[4] is False
    assert bgzf.scan(blk)[4] is False
    assert bgzf.scan(blk + B.bgzf_block(b""))[4] is True        # zlib's empty block is the same 28 bytes
    assert bgzf.scan(blk + B.EOF_BLOCK[:27])[4] is False          # incomplete: not counted
    assert bgzf.scan(blk + B.bgzf_block(b"", before=b"AB\x00\x00"))[4] is False   # empty, but not the 28-byte block


def _scan_error(data, first_block=0):
    with pytest.raises(SarlaccError) as e:
        bgzf.scan(data, first_block=first_block)
    return str(e.value)


def test_scan_errors():
    good = B.bgzf_block(b"good")
    bad = bytearray(good)
    bad[1] = 0x8c
    assert _scan_error(good + bytes(bad)) == "BGZF block 2: not a gzip member"
    assert _scan_error(good + b"@read\n") == "BGZF block 2: not a gzip member"
    bad = bytearray(good)
    bad[2] = 7
    assert _scan_error(bytes(bad), first_block=40) == "BGZF block 41: not a gzip member"
    assert _scan_error(good + good + gzip.compress(b"plain")) == "BGZF block 3: no BC subfield"
    raw = B.deflate_raw(b"abc")
    no_bc = b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff" + struct.pack("<H", 6) + b"XY\x02\x00\x00\x00" + raw + struct.pack("<II", zlib.crc32(b"abc"), 3)
    assert _scan_error(no_bc) == "BGZF block 1: no BC subfield"
    wrong_len = b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff" + struct.pack("<H", 7) + b"BC\x03\x00\x00\x00\x00" + raw + bytes(8)
    assert _scan_error(wrong_len) == "BGZF block 1: no BC subfield"
    small = bytearray(good)
    small[16:18] = struct.pack("<H", 24)                 # BSIZE + 1 = 25 < 18 + 8
    assert _scan_error(bytes(small)) == "BGZF block 1: block size field is inconsistent"
    big = bytearray(good)
    big[-4:] = struct.pack("<I", 65537)
    assert _scan_error(good + bytes(big), first_block=7) == "BGZF block 9: uncompressed size exceeds 65536"
    full = bytearray(good)
    full[-4:] = struct.pack("<I", 65536)                 # the limit itself is allowed
    assert bgzf.scan(bytes(full))[3].tolist() == [0, 65536]


def test_reader_names_the_block_a_file_ends_in(tmp_path):
    blocks = [B.bgzf_block(b"x" * 100) for _ in range(3)]
    path = tmp_path / "cut.gz"
    path.write_bytes(b"".join(blocks)[:-5])
    with open(path, "rb") as fh:
        r = bgzf.BgzfReader(fh)
        with pytest.raises(SarlaccError, match="file ends inside BGZF block 3"):
            r.take(None)


def test_reader_takes_whole_blocks_up_to_a_target(tmp_path):
    texts = [bytes([65 + k]) * 1000 for k in range(7)]
    path = tmp_path / "seven.gz"
    path.write_bytes(B.bgzf_file(*[B.bgzf_block(t) for t in texts]))
    with open(path, "rb") as fh:
        r = bgzf.BgzfReader(fh)
        sizes, firsts = [], []
        while True:
            got = r.take(2500)
            if got is None:
                break
            comp, comp_off, text_off, first = got
            assert len(comp) == comp_off[-1] and gzip.decompress(comp) == b"".join(texts)[sum(sizes):sum(sizes) + text_off[-1]]
            sizes.append(int(text_off[-1]))
            firsts.append(first)
        assert sizes == [3000, 3000, 1000] and firsts == [0, 3, 6] and r.exhausted()


def test_sniffing(tmp_path):
    cases = {"empty": (b"", bgzf.TEXT), "one": (b"\x1f", bgzf.TEXT), "text": (b"@r\nA\n+\n!\n", bgzf.TEXT),
             "magic only": (b"\x1f\x8b", bgzf.GZIP), "gzip": (gzip.compress(b"@r\nA\n+\n!\n"), bgzf.GZIP),
             "bgzf": (B.bgzf_compress(b"@r\nA\n+\n!\n"), bgzf.BGZF), "eof only": (B.EOF_BLOCK, bgzf.BGZF),
             "bc later": (B.bgzf_block(b"x", before=b"AB\x01\x00q"), bgzf.BGZF)}
    for name, (data, want) in cases.items():
        p = tmp_path / "f"
        p.write_bytes(data)
        assert bgzf.sniff(p) == want, name


FASTQ = b"@r1 first\nACGTN\n+\nIIII!\n@r2\n\n+\n\n@r3\nacgt\n+r3\n~~~~\n"


def test_read_fastq_of_compressed_files(tmp_path):
    (tmp_path / "t.fastq").write_bytes(FASTQ)
    (tmp_path / "b.fastq.gz").write_bytes(B.bgzf_compress(FASTQ, block=7))
    (tmp_path / "g.fastq.gz").write_bytes(gzip.compress(FASTQ[:24]) + gzip.compress(FASTQ[24:]))
    want = generics.read_fastq(tmp_path / "t.fastq")
    assert want.names == ["r1 first", "r2", "r3"]
    for name in ("b.fastq.gz", "g.fastq.gz"):
        got = generics.read_fastq(tmp_path / name)
        assert got.names == want.names and got.seq.to_strings() == want.seq.to_strings()
        assert got.qual.to_strings() == want.qual.to_strings()


def test_gzip_reader_reads_like_a_file(tmp_path):
    data = RNG.integers(0, 256, size=300000, dtype=np.uint8).tobytes()
    p = tmp_path / "m.gz"
    p.write_bytes(gzip.compress(data[:100000]) + gzip.compress(b"") + gzip.compress(data[100000:]))
    with open(p, "rb") as fh:
        r = bgzf.GzipReader(fh)
        got = [r.read(70001) for _ in range(6)]
    assert [len(g) for g in got] == [70001] * 4 + [300000 - 4 * 70001, 0] and b"".join(got) == data
    with open(p, "rb") as fh:
        assert bgzf.GzipReader(fh).read() == data
    p.write_bytes(gzip.compress(data)[:-9])
    with open(p, "rb") as fh, pytest.raises(SarlaccError, match="ends inside a member"):
        bgzf.GzipReader(fh).read()


@pytest.mark.parametrize("name", sorted(B.malformed()))
def test_malformed_streams_are_malformed_for_zlib(name):
    raw, _, _ = B.malformed()[name]
    with pytest.raises(zlib.error):
        zlib.decompress(raw, -15)


def test_host_header_blocks(tmp_path):
    text = b"".join(b"@SQ\tSN:c%d\tLN:%d\n" % (k, k + 1) for k in range(40))
    p = tmp_path / "h.gz"
    p.write_bytes(B.bgzf_compress(text, block=100))
    with open(p, "rb") as fh:
        got = list(bgzf.host_blocks(fh))
    assert b"".join(t for _, _, t in got) == text and [n for _, n, _ in got] == list(range(len(got)))
    assert got[1][0] == len(B.bgzf_block(text[:100]))
    # a damaged block in front of the body is refused here, by its number
    from tests.bgzf_cases import malformed_block
    p.write_bytes(B.bgzf_block(text[:100]) + malformed_block("stored"))
    with open(p, "rb") as fh, pytest.raises(SarlaccError, match="^BGZF block 2: "):
        list(bgzf.host_blocks(fh))
    flipped = bytearray(B.bgzf_block(text[:100], 0))
    flipped[30] ^= 1
    p.write_bytes(bytes(flipped))
    with open(p, "rb") as fh, pytest.raises(SarlaccError, match="^BGZF block 1: CRC32 mismatch"):
        list(bgzf.host_blocks(fh))
