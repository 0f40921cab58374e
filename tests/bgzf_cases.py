"""Builders of BGZF test files (SAM specification section 4.1): whole blocks made with zlib's raw deflate plus the
18-byte header and the 8-byte trailer, and a small bit writer for hand-made deflate streams that are malformed on
purpose.  gzip.decompress of a file built here returns the input; the CPU tests hold the malformed streams against
zlib.decompress(raw, -15)."""
import struct
import zlib

EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def wrap(raw, crc, isize, before=b"", after=b""):
    """One BGZF block around the raw deflate stream `raw`; `before` / `after` are whole extra subfields put on either
    side of the BC subfield."""
    xlen = len(before) + 6 + len(after)
    bsize = 12 + xlen + len(raw) + 8 - 1
    head = b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff" + struct.pack("<H", xlen) + before + b"BC\x02\x00" + \
        struct.pack("<H", bsize) + after
    return head + raw + struct.pack("<II", crc & 0xffffffff, isize)


def deflate_raw(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=None):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    if flush_at is None:
        return c.compress(data) + c.flush()
    return c.compress(data[:flush_at]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(data[flush_at:]) + c.flush()


def bgzf_block(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=None, before=b"", after=b""):
    raw = deflate_raw(data, level, strategy, flush_at)
    blk = wrap(raw, zlib.crc32(data), len(data), before, after)
    assert len(blk) <= 65536, "a BGZF block holds at most 64 KB"
    return blk


def bgzf_file(*blocks, eof=True):
    return b"".join(blocks) + (EOF_BLOCK if eof else b"")


def bgzf_compress(text, block=5000, level=6, eof=True):
    """`text` as a BGZF file of blocks of `block` bytes of text."""
    return bgzf_file(*[bgzf_block(text[i:i + block], level) for i in range(0, len(text), block)], eof=eof)


def block_offsets(blocks):
    """Offsets of a list of blocks laid end to end, the end of the last one included."""
    off = [0]
    for b in blocks:
        off.append(off[-1] + len(b))
    return off


class BitWriter:
    """Deflate's bit order: values LSB first, Huffman codes MSB first."""

    def __init__(self):
        self.bits = []

    def value(self, v, n):
        self.bits += [(v >> k) & 1 for k in range(n)]
        return self

    def code(self, c, n):
        self.bits += [(c >> (n - 1 - k)) & 1 for k in range(n)]
        return self

    def align(self):
        self.bits += [0] * (-len(self.bits) % 8)
        return self

    def raw(self, data):
        assert len(self.bits) % 8 == 0
        for byte in data:
            self.value(byte, 8)
        return self

    def bytes(self):
        b = self.bits + [0] * (-len(self.bits) % 8)
        return bytes(sum(b[i + k] << k for k in range(8)) for i in range(0, len(b), 8))


def _fixed_literal(w, byte):
    return w.code(0x30 + byte, 8) if byte < 144 else w.code(0x190 + byte - 144, 9)


LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]


def fixed_stream(tokens):
    """One final fixed-Huffman deflate block of the tokens: an int is a literal, (length, distance) a match.  zlib never
    emits a distance above 32 506; this does."""
    w = BitWriter().value(1, 1).value(1, 2)
    for t in tokens:
        if isinstance(t, int):
            _fixed_literal(w, t)
            continue
        length, dist = t
        s = max(i for i in range(29) if LEN_BASE[i] <= length)
        if s < 23:
            w.code(s + 1, 7)
        else:
            w.code(0xc0 + s - 23, 8)
        w.value(length - LEN_BASE[s], LEN_EXTRA[s])
        d = max(i for i in range(30) if DIST_BASE[i] <= dist)
        w.code(d, 5).value(dist - DIST_BASE[d], DIST_EXTRA[d])
    return w.code(0, 7).bytes()


def malformed():
    """name -> (raw deflate stream, size the trailer claims, the device's reason).  Every stream is final-block-first:
    a decoder meets the fault before anything else."""
    out = {}
    # fixed Huffman: the first symbol is a match of length 3 (symbol 257) at distance 1 (code 0), then end of block
    w = BitWriter().value(1, 1).value(1, 2).code(1, 7).code(0, 5).code(0, 7)
    out["distance"] = (w.bytes(), 3, "distance beyond the start of the block")
    # dynamic: 257 + 1 lengths, four code-length codes (16, 17, 18, 0) of 1 bit each: over-subscribed
    w = BitWriter().value(1, 1).value(2, 2).value(0, 5).value(0, 5).value(0, 4)
    for _ in range(4):
        w.value(1, 3)
    w.value(0, 32)
    out["oversubscribed code-length code"] = (w.bytes(), 4, "invalid code lengths")
    # dynamic: a complete code-length code (0 and 1, one bit each), then 257 literal/length codes of length 1
    w = BitWriter().value(1, 1).value(2, 2).value(0, 5).value(0, 5).value(14, 4)
    order = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
    for sym in order[:18]:
        w.value(1 if sym in (0, 1) else 0, 3)
    for _ in range(258):
        w.code(1, 1)
    w.value(0, 32)
    out["oversubscribed literal code"] = (w.bytes(), 4, "invalid code lengths")
    # stored: NLEN is not the complement of LEN
    w = BitWriter().value(1, 1).value(0, 2).align().value(5, 16).value((5 ^ 0xffff) ^ 1, 16).raw(b"hello")
    out["stored"] = (w.bytes(), 5, "invalid stored block")
    # fixed Huffman: five literals and no end-of-block symbol (43 bits: the 5 bits of padding are no symbol)
    w = BitWriter().value(1, 1).value(1, 2)
    for byte in b"hello":
        _fixed_literal(w, byte)
    out["truncated"] = (w.bytes(), 5, "compressed data ends early")
    return out


def malformed_block(name):
    raw, isize, _ = malformed()[name]
    return wrap(raw, zlib.crc32(b"hello"), isize)
