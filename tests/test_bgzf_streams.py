"""The hand-built deflate streams of tests/bgzf_cases.py, the part that needs no device: zlib, the reference inflate and
gzip agree on the text of every named and generated stream; the streams contain what they claim (conditions on the
inputs of tests/test_gpu_bgzf.py, read from the reference inflate's statistics); zlib refuses what the device must
refuse."""
import gzip
import random
import struct
import zlib
from collections import Counter

import pytest

from tests import bgzf_cases as B


@pytest.fixture(scope="module")
def named():
    return {name: (text, block, B.ref_inflate(raw)) for _, name, raw, text, block in B.named_streams()}


@pytest.fixture(scope="module")
def generated():
    return [(text, block, B.ref_inflate(raw)) for raw, text, block in B.generated_streams()]


def test_reference_inflate_agrees_with_zlib_on_zlibs_streams():
    text = bytes(random.Random(5).choice(b"ACGTN\n") for _ in range(20000)) + b"\0" * 300
    for level, strategy in ((0, zlib.Z_DEFAULT_STRATEGY), (1, zlib.Z_DEFAULT_STRATEGY), (9, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_FIXED),
                            (6, zlib.Z_RLE), (6, zlib.Z_HUFFMAN_ONLY)):
        got, stats = B.ref_inflate(B.deflate_raw(text, level, strategy, flush_at=7000))
        assert got == text and stats[-1]["final"] and stats[-1]["text"] == len(text)
    tokens = [65, 66, (258, 2), (3, 1), 200, (100, 260)]
    w = B.fixed_block(B.BitWriter(), tokens, 1)
    assert w.bytes() == B.fixed_stream(tokens) and B.text_len(tokens) == len(zlib.decompress(w.bytes(), -15))


def test_every_stream_has_one_text(named, generated):
    assert len(generated) == 256 and len(named) == len(B.named_streams())
    for text, block, (ref, _) in list(named.values()) + generated:
        assert len(block) <= 65536 and len(text) <= 65536
        assert zlib.decompress(block[18:-8], -15) == text          # what block_of took as the text
        assert ref == text
        assert gzip.decompress(block) == text


def test_generated_streams_cover_the_limits(generated):
    lit, dist, start = Counter(), Counter(), Counter()
    crossing = lone = absent = 0
    for _, _, (_, stats) in generated:
        assert 1 <= len(stats) <= 7                                # 1-6 blocks, and the stored history of every fourth
        for st in stats:
            if st["type"] != "dynamic":
                continue
            lit += st["lit_hist"]
            dist += st["dist_hist"]
            start[st["start_bit"]] += 1
            crossing += st["crossing"]
            lone += st["longest"][2] == 1
            absent += st["longest"][2] == 0
    assert all(lit[n] >= 20 for n in range(11, 16)), sorted(lit.items())
    assert all(dist[n] >= 20 for n in range(9, 16)), sorted(dist.items())
    assert all(start[b] >= 5 for b in range(8)), sorted(start.items())
    assert crossing >= 20 and lone >= 10 and absent >= 10, (crossing, lone, absent)
    kinds = Counter(st["type"] for _, _, (_, stats) in generated for st in stats)
    assert min(kinds["stored"], kinds["fixed"], kinds["dynamic"]) >= 100


def test_named_streams_show_their_property(named):
    def last(name):
        return named[name][2][1][-1]
    LB, DB = B.table_bits()
    assert 1 <= DB < LB < 15
    # 1. ladders: every length 1 ... 15 decoded, the two 15-bit codes of either alphabet at least once each
    st = last("ladders")
    assert st["longest"][1:] == (15, 15)
    for hist in (st["lit_hist"], st["dist_hist"]):
        assert all(hist[n] >= 1 for n in range(1, 15)) and hist[15] >= 2
    # 2. at the direct tables' widths and one bit above
    st = last("edge ladder")
    assert st["longest"][1:] == (LB + 1, DB + 1)
    assert st["lit_hist"][LB] >= 1 and st["lit_hist"][LB + 1] >= 2 and st["dist_hist"][DB] >= 1 and st["dist_hist"][DB + 1] >= 2
    st = last("edge groups")
    assert st["lit_hist"][LB] >= 2 and st["lit_hist"][LB + 1] >= 4 and st["dist_hist"][DB] >= 2 and st["dist_hist"][DB + 1] >= 4
    # 3. full alphabets
    st = last("full alphabets")
    assert (st["hlit"], st["hdist"]) == (286, 30) and st["longest"][1:] == (9, 5)
    assert st["lit_hist"][8] + st["lit_hist"][9] >= 286 and st["dist_hist"][4] >= 2 and st["dist_hist"][5] >= 28
    assert st["len_seen"] >= {(257 + s, x) for s in range(29) for x in (0, (1 << B.LEN_EXTRA[s]) - 1)}
    assert st["dist_seen"] >= {(d, x) for d in range(30) for x in (0, (1 << B.DIST_EXTRA[d]) - 1)}
    # 4. 130 tokens of 48 bits at every bit offset
    for bit in range(8):
        st = last("maximal tokens at bit %d" % bit)
        assert st["start_bit"] == bit and st["token_bits"][48] == st["tokens"] == 130 and st["text"] <= 65536
    # 5. lone and absent codes
    st = last("lone end-of-block code")
    assert st["type"] == "dynamic" and st["longest"][1] == 1 and st["tokens"] == 0 and named["lone end-of-block code"][0] == b""
    st = last("lone distance code")
    assert st["longest"][2] == 1 and st["dist_hist"][1] == 1 and named["lone distance code"][0] == b"AAAA"
    st = last("no distance code")
    assert st["hdist"] == 1 and st["longest"][2] == 0 and st["tokens"] == 4
    # 6. the code-length code
    assert last("7-bit code-length code")["longest"][0] == 7
    st = last("hclen 19")
    assert st["hclen"] == 19 and st["longest"][1] == 15
    st = last("shortest header")
    assert st["hclen"] == 5 and st["hdist"] == 1 and st["longest"][2] == 0 and st["tokens"] == 255
    # 7. repeats
    counts = {(s, c) for s, c, _ in last("every repeat count")["repeats"]}
    assert counts >= {(16, 3), (16, 4), (16, 5), (16, 6), (17, 3), (17, 10), (18, 11), (18, 138)}
    for name, sym in (("16 across", 16), ("18 across", 18)):
        st = last(name)
        assert st["crossing"] and any(s == sym and at < st["hlit"] < at + c for s, c, at in st["repeats"]) and st["dist_hist"]
    st = last("16 first in distances")
    assert any(s == 16 and at == st["hlit"] for s, _, at in st["repeats"]) and not st["crossing"]
    # 8. bit offsets and sequences
    for bit in range(8):
        st = last("dynamic block at bit %d" % bit)
        assert st["type"] == "dynamic" and st["start_bit"] == bit and st["tokens"] == 7
        first, second = named["stored block after bit %d" % bit][2][1]
        assert first["type"] == "fixed" and first["end_bit"] == bit and second["type"] == "stored" and second["text"] > first["text"]
    text, _, (_, stats) = named["103 deflate blocks"]
    assert len(stats) >= 100 and stats[-1]["final"] and stats[-1]["text"] == stats[-2]["text"] == len(text)
    sizes = [b["text"] - a["text"] for a, b in zip([{"text": 0}] + stats, stats)]
    for kind in ("stored", "fixed", "dynamic"):
        assert sum(st["type"] == kind and n == 0 for st, n in zip(stats, sizes)) >= 10
        assert sum(st["type"] == kind and n > 0 for st, n in zip(stats, sizes)) >= 10
    assert text[:12] == b"<stored 00>f" and text.count(text[:12]) >= 4          # matches at distance `produced` copy the first bytes
    # 9. batches of 64 tokens
    assert last("chain of 63")["tokens"] == 64 and named["chain of 63"][0] == b"A" * 190
    assert last("chain across batches")["tokens"] == 65 and named["chain across batches"][0] == b"B" + b"A" * 190
    assert last("overlapping matches in one batch")["tokens"] <= 64
    # 10. sizes
    assert len(named["text of 65536 bytes"][0]) == 65536 and len(named["text of 65536 bytes"][1]) < 40000
    block = named["block of 65536 bytes"][1]
    assert len(block) == 65536 and struct.unpack("<H", block[16:18])[0] == 65535
    for n in (1, 63, 64, 65, 127, 128, 129):
        assert len(named["text of %d bytes" % n][0]) == n


@pytest.mark.parametrize("name", sorted(B.refusals()))
def test_refusals_are_refused_by_zlib(name):
    raw, isize, _ = B.refusals()[name]
    if name in B.OVERFLOWS:
        # valid deflate; the size field is the block's, and gzip holds the text against it
        assert len(zlib.decompress(raw, -15)) > isize
        with pytest.raises(gzip.BadGzipFile):
            gzip.decompress(B.wrap(raw, zlib.crc32(zlib.decompress(raw, -15)), isize))
        return
    with pytest.raises(zlib.error):
        zlib.decompress(raw, -15)
    with pytest.raises(ValueError):
        B.ref_inflate(raw)


def test_lone_codes_as_zlib_takes_them():
    """The device follows zlib: a lone code of 1 bit is a code, a lone code of 2 bits is not."""
    assert zlib.decompress(B.dynamic_block(B.BitWriter(), [0] * 256 + [1], [0], [], 1, cl_syms=[(18, 138), (18, 118), 1, 0]).bytes(), -15) == b""
    for name, message in (("lone end-of-block code of 2 bits", "invalid literal/lengths set"), ("lone distance code of 2 bits", "invalid distances set")):
        with pytest.raises(zlib.error, match=message):
            zlib.decompress(B.refusals()[name][0], -15)


def test_handbuilt_fastq_is_the_text():
    recs = [b"@r%d x\n%s\n+\n%s\n" % (k, bytes(random.Random(k).choice(b"ACGTN") for _ in range(k * 37 % 400)), b"I" * (k * 37 % 400))
            for k in range(40)]
    text = b"".join(recs)
    data = B.handbuilt_fastq(text, records=16)
    assert gzip.decompress(data) == text
    kinds, longest, matches = Counter(), set(), 0
    pos = 0
    while pos < len(data) - len(B.EOF_BLOCK):
        size = struct.unpack("<H", data[pos + 16:pos + 18])[0] + 1
        for st in B.ref_inflate(data[pos + 18:pos + size - 8])[1]:
            kinds[st["type"]] += 1
            if st["type"] == "dynamic":
                longest.add(st["longest"][1:])
                matches += sum(st["dist_hist"].values())
        pos += size
    assert pos == len(data) - len(B.EOF_BLOCK) and kinds["dynamic"] == 40 and min(kinds["stored"], kinds["fixed"]) >= 40
    assert longest == {(15, 15)} and matches >= 100
