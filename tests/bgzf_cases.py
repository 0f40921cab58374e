"""Builders of BGZF test files (SAM specification section 4.1): whole blocks made with zlib's raw deflate plus the
18-byte header and the 8-byte trailer, and a small bit writer for hand-made deflate streams: malformed on purpose, or
valid and at the limits of the format, where zlib's own output never goes.  gzip.decompress of a file built here
returns the input; the CPU tests hold the malformed streams against zlib.decompress(raw, -15) and take the text of the
valid ones from it."""
import functools
import os
import random
import re
import struct
import zlib
from collections import Counter

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
            self.bits += _BYTE_BITS[byte]
        return self

    def bytes(self):
        b = self.bits + [0] * (-len(self.bits) % 8)
        return int("".join(map(str, reversed(b))) or "0", 2).to_bytes(len(b) // 8, "little")


_BYTE_BITS = [[(byte >> k) & 1 for k in range(8)] for byte in range(256)]


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


# ---- deflate blocks by hand ------------------------------------------------------------------------------------------
# Appenders of single deflate blocks to a BitWriter that may already hold bits, so that a block starts at any bit and a
# stream holds any sequence of block types; a reference inflate that reports what a stream contains; the named streams
# at the format's limits, a seeded generator, and the streams a decoder must refuse.  zlib judges the bytes throughout.
CLEN_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
REPEAT = {16: (3, 2), 17: (3, 3), 18: (11, 7)}            # repeat symbol -> (smallest count, extra bits)


def canonical(lens):
    """symbol -> (code, bits) of the canonical Huffman code of the lengths (RFC 1951 section 3.2.2).  The lengths are
    taken as given: nothing checks that the code is complete."""
    count = [0] * 17
    for n in lens:
        count[n] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for n in range(1, 17):
        code = (code + count[n - 1]) << 1
        nxt[n] = code
    out = {}
    for s, n in enumerate(lens):
        if n:
            out[s] = (nxt[n], n)
            nxt[n] += 1
    return out


FIXED_LIT = canonical([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
FIXED_DIST = canonical([5] * 32)


def match_symbols(length, dist):
    s = max(i for i in range(29) if LEN_BASE[i] <= length)
    d = max(i for i in range(30) if DIST_BASE[i] <= dist)
    return s, length - LEN_BASE[s], d, dist - DIST_BASE[d]


def put_tokens(w, lit, dist, tokens):
    """The tokens in the codes `lit` / `dist` (symbol -> (code, bits)).  An int is a literal and (length, distance) a
    match, as in fixed_stream.  Three forms say more: ("sym", s, xl, d, xd) is a match by its length symbol 257 + s and
    distance symbol d with the values of their extra bits (258 as 284 + 31; the undefined distance symbol 30);
    ("lit", s) is a bare literal/length symbol; ("bits", v, n) is n raw bits."""
    for t in tokens:
        if isinstance(t, int):
            w.code(*lit[t])
        elif t[0] == "lit":
            w.code(*lit[t[1]])
        elif t[0] == "bits":
            w.value(t[1], t[2])
        else:
            s, xl, d, xd = t[1:] if t[0] == "sym" else match_symbols(*t)
            w.code(*lit[257 + s]).value(xl, LEN_EXTRA[s]).code(*dist[d]).value(xd, DIST_EXTRA[d] if d < 30 else 0)
    return w


def text_len(tokens):
    """Bytes that the tokens produce."""
    return sum(1 if isinstance(t, int) else LEN_BASE[t[1]] + t[2] if t[0] == "sym" else t[0] for t in tokens)


def stored_block(w, data, final):
    return w.value(final, 1).value(0, 2).align().value(len(data), 16).value(len(data) ^ 0xffff, 16).raw(data)


def fixed_block(w, tokens, final):
    w.value(final, 1).value(1, 2)
    return put_tokens(w, FIXED_LIT, FIXED_DIST, tokens).code(0, 7)


def flat_lengths(n):
    """Lengths of a complete code of n >= 2 symbols, as even as can be, the shorter ones first."""
    k = n.bit_length() - 1
    longer = 2 * (n - (1 << k))
    return [k] * (n - longer) + [k + 1] * longer


def lens_of(assign, n=None):
    """List of n code lengths from symbol -> length."""
    out = [0] * (max(assign) + 1 if n is None else n)
    for s, v in assign.items():
        out[s] = v
    return out


def expand_lengths(cl_syms):
    """The code lengths that a sequence of code-length symbols stands for: an int is a length, (16 | 17 | 18, count) a
    repeat."""
    out = []
    for s in cl_syms:
        if isinstance(s, int):
            out.append(s)
        else:
            out += [out[-1] if s[0] == 16 else 0] * s[1]
    return out


def run_lengths(lens, rng=None):
    """Code-length symbols of the lengths with repeats: the longest ones, or with `rng` a random legal choice of where
    to repeat and how far.  The lengths are one list, so a repeat runs from the literal/length lengths into the
    distance lengths where the values allow it."""
    out, i = [], 0
    while i < len(lens):
        v, run = lens[i], 1
        while i + run < len(lens) and lens[i + run] == v:
            run += 1
        if v == 0 and run >= 3 and (rng is None or rng.random() < 0.8):
            sym, lo, hi = (18, 11, 138) if run >= 11 and (rng is None or rng.random() < 0.7) else (17, 3, 10)
            c = min(run, hi) if rng is None else rng.randint(lo, min(run, hi))
        elif i > 0 and lens[i - 1] == v and run >= 3 and (rng is None or rng.random() < 0.8):
            sym, c = 16, (min(run, 6) if rng is None else rng.randint(3, min(run, 6)))
        else:
            out.append(v)
            i += 1
            continue
        out.append((sym, c))
        i += c
    return out


def dynamic_block(w, lit_lens, dist_lens, tokens, final, cl_syms=None, clen_lens=None, hclen=None, eob=True, check=True):
    """One dynamic-Huffman block.  HLIT and HDIST are the sizes of the two lists, trailing zeros included (288 and 32
    lengths write the field values 31 and 31, which no valid block has).  `cl_syms` is the exact sequence of
    code-length symbols (see expand_lengths; default: every length on its own, no repeat), `clen_lens` the 19 lengths
    of the code-length code by symbol (default: a complete code, as flat as can be, of the symbols that occur) and
    `hclen` how many of them are written (default: up to the last non-zero one).  The codes are the canonical ones of
    the lengths as given.  check=False writes a header whose symbols do not spell the lengths; eob=False leaves the
    end-of-block code out."""
    lit_lens, dist_lens = list(lit_lens), list(dist_lens)
    if cl_syms is None:
        cl_syms = lit_lens + dist_lens
    if check:
        assert expand_lengths(cl_syms) == lit_lens + dist_lens
    if clen_lens is None:
        used = sorted(set(s if isinstance(s, int) else s[0] for s in cl_syms))
        if len(used) == 1:
            used.append(1 if used[0] == 0 else 0)
        clen_lens = lens_of(dict(zip(used, flat_lengths(len(used)))), 19)
    if hclen is None:
        hclen = max(4, 1 + max(i for i in range(19) if clen_lens[CLEN_ORDER[i]]))
    w.value(final, 1).value(2, 2).value(len(lit_lens) - 257, 5).value(len(dist_lens) - 1, 5).value(hclen - 4, 4)
    for i in range(hclen):
        w.value(clen_lens[CLEN_ORDER[i]], 3)
    cl = canonical(clen_lens)
    for s in cl_syms:
        if isinstance(s, int):
            w.code(*cl[s])
        else:
            w.code(*cl[s[0]]).value(s[1] - REPEAT[s[0]][0], REPEAT[s[0]][1])
    lit = canonical(lit_lens)
    put_tokens(w, lit, canonical(dist_lens), tokens)
    return w.code(*lit[256]) if eob else w


def shift_to(w, bit):
    """Non-final fixed blocks, the first of them empty, until the next block starts at bit `bit` of a byte: an empty
    one takes 10 bits, one with a 9-bit literal 19."""
    fixed_block(w, [], 0)
    while (bit - len(w.bits)) % 8 % 2:
        fixed_block(w, [200], 0)
    while (bit - len(w.bits)) % 8:
        fixed_block(w, [], 0)
    return w


# ---- reference inflate -----------------------------------------------------------------------------------------------
def _decode_table(lens, kind):
    """(code, bits) -> symbol, and the longest code.  Refuses what zlib refuses: an over-subscribed code, and an
    incomplete one unless it is a lone 1-bit literal/length or distance code, or no code at all."""
    count = Counter(n for n in lens if n)
    left = 1
    for n in range(1, 16):
        left = 2 * left - count[n]
        if left < 0:
            raise ValueError("over-subscribed %s code" % kind)
    longest = max(count, default=0)
    if left > 0 and longest and (kind == "code-length" or longest != 1):
        raise ValueError("incomplete %s code" % kind)
    return {cn: s for s, cn in canonical(lens).items()}, longest


_FIXED_TABLES = (_decode_table([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8, "literal/length")[0],
                 _decode_table([5] * 32, "distance")[0])


def ref_inflate(raw):
    """(text, stats) of a raw deflate stream: a plain inflate after RFC 1951, one bit at a time.  ValueError on a
    stream that is not valid.  stats has one dict per deflate block: type, final, start_bit and end_bit (0-7: the bit of
    a byte at which the block starts and the bit after its last one), text (bytes produced up to its end), tokens,
    lit_hist / dist_hist (code length -> symbols decoded through a code of that length, end of block included),
    token_bits (bits of a whole match -> matches) and len_seen / dist_seen ((symbol, value of its extra bits) of the
    matches); for a dynamic block also hlit, hdist, hclen, longest (of the code-length, literal/length and distance
    codes), repeats ((symbol, count, index of the first length it writes)) and crossing (a repeat begins in the
    literal/length lengths and ends in the distance lengths)."""
    pos, out, stats, final = 0, bytearray(), [], 0

    def bits(n):
        nonlocal pos
        if pos + n > 8 * len(raw):
            raise ValueError("the stream ends early")
        v = 0
        for k in range(n):
            v |= ((raw[pos >> 3] >> (pos & 7)) & 1) << k
            pos += 1
        return v

    def symbol(table):
        code = 0
        for n in range(1, 16):
            code = (code << 1) | bits(1)
            if (code, n) in table:
                return table[code, n], n
        raise ValueError("no such code")

    while not final:
        st = {"start_bit": pos & 7, "tokens": 0, "lit_hist": Counter(), "dist_hist": Counter(), "token_bits": Counter(),
              "len_seen": set(), "dist_seen": set()}
        final, kind = bits(1), bits(2)
        if kind == 3:
            raise ValueError("reserved block type")
        st.update(type=("stored", "fixed", "dynamic")[kind], final=final)
        if kind == 0:
            pos += -pos % 8
            n = bits(16)
            if n ^ 0xffff != bits(16):
                raise ValueError("invalid stored block")
            if (pos >> 3) + n > len(raw):
                raise ValueError("the stream ends early")
            out += raw[pos >> 3:(pos >> 3) + n]
            pos += 8 * n
        else:
            lit, dist = _FIXED_TABLES
            if kind == 2:
                hlit, hdist, hclen = bits(5) + 257, bits(5) + 1, bits(4) + 4
                if hlit > 286 or hdist > 30:
                    raise ValueError("too many length or distance symbols")
                cl = [0] * 19
                for i in range(hclen):
                    cl[CLEN_ORDER[i]] = bits(3)
                table, longest_cl = _decode_table(cl, "code-length")
                lens, repeats, crossing = [], [], False
                while len(lens) < hlit + hdist:
                    s, _ = symbol(table)
                    if s < 16:
                        lens.append(s)
                        continue
                    c = REPEAT[s][0] + bits(REPEAT[s][1])
                    if s == 16 and not lens:
                        raise ValueError("a repeat with nothing before it")
                    if len(lens) + c > hlit + hdist:
                        raise ValueError("a repeat past the last length")
                    crossing |= len(lens) < hlit < len(lens) + c
                    repeats.append((s, c, len(lens)))
                    lens += [lens[-1] if s == 16 else 0] * c
                if lens[256] == 0:
                    raise ValueError("no end-of-block code")
                lit, longest_lit = _decode_table(lens[:hlit], "literal/length")
                dist, longest_dist = _decode_table(lens[hlit:], "distance")
                st.update(hlit=hlit, hdist=hdist, hclen=hclen, longest=(longest_cl, longest_lit, longest_dist),
                          repeats=repeats, crossing=crossing)
            while True:
                at = pos
                s, n = symbol(lit)
                st["lit_hist"][n] += 1
                if s == 256:
                    break
                st["tokens"] += 1
                if s < 256:
                    out.append(s)
                    continue
                if s - 257 >= 29:
                    raise ValueError("invalid length symbol")
                extra = bits(LEN_EXTRA[s - 257])
                st["len_seen"].add((s, extra))
                length = LEN_BASE[s - 257] + extra
                d, n = symbol(dist)
                st["dist_hist"][n] += 1
                if d >= 30:
                    raise ValueError("invalid distance symbol")
                extra = bits(DIST_EXTRA[d])
                st["dist_seen"].add((d, extra))
                distance = DIST_BASE[d] + extra
                if distance > len(out):
                    raise ValueError("distance beyond the start of the stream")
                for _ in range(length):
                    out.append(out[-distance])
                st["token_bits"][pos - at] += 1
        st.update(end_bit=pos & 7, text=len(out))
        stats.append(st)
    return bytes(out), stats


def block_of(raw):
    """(text by zlib, BGZF block with the right CRC and ISIZE) of a valid raw deflate stream."""
    text = zlib.decompress(raw, -15)
    return text, wrap(raw, zlib.crc32(text), len(text))


# ---- named streams at the limits --------------------------------------------------------------------------------------
LADDER = list(range(1, 16)) + [15]          # lengths 1, 2, ..., 14, 15, 15: complete, every length present


def table_bits():
    """(LIT_BITS, DIST_BITS): the widths of the kernel's direct tables, from its source text."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "sarlacc_amd", "csrc", "bgzf.hip")
    m = re.search(r"constexpr int LIT_BITS = (\d+), DIST_BITS = (\d+);", open(path).read())
    return int(m.group(1)), int(m.group(2))


def _history():
    return random.Random(32768).randbytes(32768)


def _ladder_codes(lit_syms, dist_syms, lit_shape=LADDER, dist_shape=LADDER):
    """Code lengths that give the symbols, in their order, the lengths of the shapes."""
    assert 256 in lit_syms and len(lit_syms) == len(lit_shape) and len(dist_syms) == len(dist_shape)
    return lens_of(dict(zip(lit_syms, lit_shape)), max(257, max(lit_syms) + 1)), lens_of(dict(zip(dist_syms, dist_shape)))


def _every_code_once(lit_syms, dist_syms):
    """Tokens that use every literal, every length symbol and every distance symbol of the lists at least once; the
    distances need 32 768 bytes of history."""
    lits = [s for s in lit_syms if s < 256]
    lsym = [s - 257 for s in lit_syms if s > 256]
    n = max(len(lsym), len(dist_syms))
    return lits + [("sym", lsym[i % len(lsym)], 0, dist_syms[i % len(dist_syms)], 0) for i in range(n)]


LADDER_LIT = [65, 67, 71, 84, 10, 78, 64, 43, 73, 33, 257, 258, 264, 284, 285, 256]
LADDER_DIST = [0, 1, 2, 3, 5, 6, 8, 10, 13, 16, 19, 22, 25, 27, 28, 29]


def _named():
    H = _history()
    out = []

    def add(group, name, w):
        out.append((group, name, w.bytes()))

    def after_history():
        return stored_block(BitWriter(), H, 0)

    # 1. ladders: both codes 1, 2, ..., 14, 15, 15 and every code decoded; symbols 285 and 256 / 28 and 29 have 15 bits
    lit_lens, dist_lens = _ladder_codes(LADDER_LIT, LADDER_DIST)
    ladder_tokens = _every_code_once(LADDER_LIT, LADDER_DIST)
    add(1, "ladders", dynamic_block(after_history(), lit_lens, dist_lens, ladder_tokens, 1, cl_syms=run_lengths(lit_lens + dist_lens)))

    # 2. direct-table edges: one code of every length up to the table's width and two one bit longer; and several codes at
    # the width and one above it, so that the walk finds codes that are not the first of their length
    LB, DB = table_bits()
    for name, shape in (("edge ladder", lambda b: list(range(1, b + 1)) + [b + 1] * 2),
                        ("edge groups", lambda b: list(range(1, b - 1)) + [b] * 2 + [b + 1] * 4)):
        ls, ds = shape(LB), shape(DB)
        lit_syms = ([256] + list(range(257, 257 + 5)) + list(range(48, 48 + len(ls) - 6)))[::-1]
        dist_syms = list(range(29, 29 - len(ds), -1))[::-1]
        lit_lens, dist_lens = _ladder_codes(lit_syms, dist_syms, ls, ds)
        add(2, name, dynamic_block(after_history(), lit_lens, dist_lens, _every_code_once(lit_syms, dist_syms), 1,
                                   cl_syms=run_lengths(lit_lens + dist_lens)))

    # 3. full alphabets: 286 literal/length codes and 30 distance codes, every length and distance symbol at its
    # smallest and largest extra value (258 also as symbol 284 + 31)
    lit_lens, dist_lens = [8] * 226 + [9] * 60, [4] * 2 + [5] * 28
    ends = [(s, x) for s in range(29) for x in sorted({0, (1 << LEN_EXTRA[s]) - 1})]
    dends = [(d, x) for d in range(30) for x in sorted({0, (1 << DIST_EXTRA[d]) - 1})]
    tokens = list(range(256)) + [("sym",) + ends[i % len(ends)] + dends[i % len(dends)] for i in range(max(len(ends), len(dends)))]
    add(3, "full alphabets", dynamic_block(after_history(), lit_lens, dist_lens, tokens, 1))

    # 4. maximal tokens: 130 matches of 15 + 5 + 15 + 13 bits (length symbols 281 / 284, distance symbols 28 / 29),
    # at every bit offset
    lit_syms = [65, 66, 67, 68, 69, 70, 71, 72, 73, 74, 75, 76, 77, 256, 281, 284]
    dist_syms = list(range(14, 28)) + [28, 29]
    lit_lens, dist_lens = _ladder_codes(lit_syms, dist_syms)
    tokens = [("sym", (24, 27)[i & 1], (7 * i) % 32, (28, 29)[(i >> 1) & 1], (8191, 0, 4097 * i % 8192)[i % 3]) for i in range(130)]
    for shift in range(8):
        w = after_history()
        if shift:
            shift_to(w, shift)
        add(4, "maximal tokens at bit %d" % shift, dynamic_block(w, lit_lens, dist_lens, tokens, 1, cl_syms=run_lengths(lit_lens + dist_lens)))

    # 5. lone and absent codes
    add(5, "lone end-of-block code", dynamic_block(BitWriter(), [0] * 256 + [1], [0], [], 1, cl_syms=[(18, 138), (18, 118), 1, 0]))
    a3 = lens_of({65: 1, 256: 2, 257: 2})
    add(5, "lone distance code", dynamic_block(BitWriter(), a3, [1], [65, (3, 1)], 1, cl_syms=run_lengths(a3 + [1])))
    ab = lens_of({65: 1, 66: 2, 256: 2})
    add(5, "no distance code", dynamic_block(BitWriter(), ab, [0], [65, 66, 66, 65], 1, cl_syms=run_lengths(ab + [0])))

    # 6. the code-length code
    lens = [6] * 32 + [7] * 32 + [8] * 32 + [9] * 63 + [0] * 97 + [9]
    cl_syms = ([6] + [(16, 6)] * 5 + [6] + [7] + [(16, 6)] * 5 + [7] + [8] + [(16, 6)] * 5 + [8] + [9] + [(16, 6)] * 10 + [9, 9] +
               [0, (18, 96)] + [9] + [(17, 4)])
    add(6, "7-bit code-length code", dynamic_block(BitWriter(), lens, [0] * 4, list(range(159)), 1, cl_syms=cl_syms,
                                                   clen_lens=lens_of({16: 1, 9: 2, 6: 3, 7: 4, 8: 5, 0: 6, 17: 7, 18: 7}, 19)))
    lit_lens, dist_lens = _ladder_codes(LADDER_LIT, LADDER_DIST)
    add(6, "hclen 19", dynamic_block(after_history(), lit_lens, dist_lens, ladder_tokens, 1, cl_syms=run_lengths(lit_lens + dist_lens)))
    add(6, "shortest header", dynamic_block(BitWriter(), [0] + [8] * 256, [0], list(range(1, 256)), 1,
                                            cl_syms=[0, 8] + [(16, 6)] * 42 + [(16, 3), 0], clen_lens=lens_of({16: 1, 0: 2, 8: 2}, 19)))

    # 7. repeats: 16 x 3..6, 17 x 3 and 10, 18 x 11 and 138 (22 + 50 codes of 8 bits and 23 of 5: complete)
    cl_syms = ([8, (16, 3), (17, 3), 8, (16, 4), (17, 10), 8, (16, 5), (18, 11), 8, (16, 6), (18, 138)] +
               [5, (16, 6), (16, 6), (16, 6), (16, 4)] + [8] + [(16, 6)] * 8 + [8] + [1, 1])
    lens = expand_lengths(cl_syms)
    coded = [s for s in range(256) if lens[s]]
    add(7, "every repeat count", dynamic_block(BitWriter(), lens[:257], lens[257:], coded + coded[::-1], 1, cl_syms=cl_syms))
    # a 16-run from the last literal/length lengths (253 ... 257) into the distance lengths: 16 + 16 codes of 4 bits
    cl_syms = [4, (16, 6), (16, 4), (18, 138), (18, 104), 4, (16, 6), (16, 6), (16, 5), (16, 3)]
    lens = expand_lengths(cl_syms)
    add(7, "16 across", dynamic_block(BitWriter(), lens[:258], lens[258:], list(range(11)) + [253, 254, 255, (3, 14), (3, 1), (3, 12)], 1, cl_syms=cl_syms))
    # an 18-run from trailing zero literal/length lengths (HLIT = 270) into the distance lengths
    lit_lens = lens_of({97: 2, 98: 2, 256: 2, 257: 2}, 270)
    cl_syms = run_lengths(lit_lens[:258]) + [(18, 22), 1, 1]
    add(7, "18 across", dynamic_block(BitWriter(), lit_lens, [0] * 10 + [1, 1], [97, 98] * 30 + [(3, 33), (3, 49), (3, 60)], 1, cl_syms=cl_syms))
    # a 16 as the first distance length copies the length of symbol 256
    lit_lens = lens_of({65: 1, 66: 2, 256: 2})
    add(7, "16 first in distances", dynamic_block(BitWriter(), lit_lens[:256] + [2], [2] * 4, [65, 66, 65], 1,
                                                  cl_syms=run_lengths(lit_lens[:256]) + [2, (16, 4)]))

    # 8. bit offsets and block sequences
    small_lit, small_dist = lens_of(dict(zip([97, 98, 99, 100, 256, 257, 258, 259], [3] * 8))), [4] * 2 + [5] * 28
    for bit in range(8):
        w = BitWriter()
        if bit:
            shift_to(w, bit)
        add(8, "dynamic block at bit %d" % bit, dynamic_block(w, small_lit, small_dist, [97, 98, 99, 100, (5, 3), (4, 1), 97], 1,
                                                              cl_syms=run_lengths(small_lit + small_dist)))
    for bit in range(8):
        # a fixed block of 8-bit literals ends at bit 2; every 9-bit literal moves its end on by one
        w = fixed_block(BitWriter(), list(b"end") + [200] * ((bit - 2) % 8), 0)
        add(8, "stored block after bit %d" % bit, stored_block(w, b"stored after bit %d" % bit, 1))
    w, produced = BitWriter(), 0
    for i in range(17):
        data = b"<stored %02d>" % i
        stored_block(w, data, 0)
        produced += len(data)
        tokens = list(b"fix") + [(6, 8)]                                           # into this stored block
        tokens.append((12, produced + text_len(tokens)))                           # to the first byte of the BGZF block
        fixed_block(w, tokens, 0)
        produced += text_len(tokens)
        tokens = [97, 98, 99, (4, 3), (5, 14 + i)]                                 # into Huffman output and stored bytes
        tokens += [(3, produced + text_len(tokens) if i % 5 == 0 else 20), 100]
        dynamic_block(w, small_lit, small_dist, tokens, 0, cl_syms=run_lengths(small_lit + small_dist))
        produced += text_len(tokens)
        stored_block(w, b"", 0)
        fixed_block(w, [], 0)
        dynamic_block(w, [0] * 256 + [1], [0], [], 0, cl_syms=[(18, 138), (18, 118), 1, 0])
    add(8, "103 deflate blocks", stored_block(w, b"", 1))

    # 9. batch shapes: a batch is 64 tokens
    add(9, "chain of 63", fixed_block(BitWriter(), [65] + [(3, 1)] * 63, 1))
    add(9, "chain across batches", fixed_block(BitWriter(), [66, 65] + [(3, 1)] * 63, 1))
    tokens = [120, (5, 1), 121, 122, (7, 2)]
    for k, d in enumerate((63, 64, 65)):
        tokens += [48 + 3 * k, 49 + 3 * k, 50 + 3 * k, (d - 3, 3), (2 * d + 5 + k, d)]
    add(9, "overlapping matches in one batch", fixed_block(BitWriter(), tokens, 1))

    # 10. sizes
    rng = random.Random(65536)
    dna = bytes(rng.choice(b"ACGTN\n") for _ in range(65536))
    out.append((10, "text of 65536 bytes", deflate_raw(dna, 6)))
    add(10, "block of 65536 bytes", stored_block(BitWriter(), rng.randbytes(65536 - 26 - 5), 1))
    for n in (1, 63, 64, 65, 127, 128, 129):
        data = rng.randbytes(n)
        add(10, "text of %d bytes" % n, fixed_block(BitWriter(), list(data), 1) if n & 1 else stored_block(BitWriter(), data, 1))
    return out


@functools.lru_cache(maxsize=None)
def named_streams():
    """(group of the list above, name, raw deflate stream, text by zlib, BGZF block) of every named stream."""
    return tuple((group, name, raw) + block_of(raw) for group, name, raw in _named())


# ---- generated streams ------------------------------------------------------------------------------------------------
def random_code(rng, n, limit, deep=0.5):
    """Lengths of a random complete code of n >= 2 symbols, none longer than `limit`: leaves of a binary tree split at
    random, the deepest one with probability `deep`, so that long codes are common."""
    limit = max(limit, (n - 1).bit_length())
    leaves = [0]
    while len(leaves) < n:
        open_ = [i for i, d in enumerate(leaves) if d < limit]
        i = max(open_, key=lambda j: leaves[j]) if rng.random() < deep else rng.choice(open_)
        leaves[i] += 1
        leaves.append(leaves[i])
    rng.shuffle(leaves)
    return leaves


def _random_tokens(rng, produced, room, history):
    """Tokens for one Huffman block that favour the edges: lengths 3 and 258, distances 1, `produced` and 32 768,
    lengths above distances."""
    alphabet = [rng.randrange(256) for _ in range(rng.choice((1, 2, 5, 20, 64)))]
    tokens, made = [], 0
    for _ in range(rng.choice((0, 1, 3, 30, 120, 300))):
        now = produced + made
        if now == 0 or rng.random() < 0.55:
            t = rng.choice(alphabet)
        else:
            length = rng.choice((3, 3, 258, 258, rng.randint(3, 258), rng.randint(3, 20), rng.randint(3, 20)))
            pick = rng.random()
            if pick < 0.15:
                dist = 1
            elif pick < 0.3:
                dist = now
            elif pick < 0.45 and history and now >= 32768:
                dist = 32768
            elif pick < 0.65:
                dist = rng.randint(1, min(now, length))                  # overlapping: the distance is at most the length
            else:
                dist = min(now, 1 << rng.randint(0, 15)) - rng.randrange(min(now, 1 << rng.randint(0, 15)) // 2 + 1)
            t = (length, min(max(dist, 1), 32768, now))
        if made + text_len([t]) > room:
            break
        tokens.append(t)
        made += text_len([t])
    return tokens, made


def _random_dynamic(rng, w, tokens, final):
    """The tokens as a dynamic block under random codes: complete ones of the symbols used and some more, a lone 1-bit
    or an absent distance code where the tokens allow it, a random complete code-length code, random repeats."""
    lit_used = {256} | {t if isinstance(t, int) else 257 + match_symbols(*t)[0] for t in tokens}
    dist_used = {match_symbols(*t)[2] for t in tokens if not isinstance(t, int)}
    spare = [s for s in range(286) if s not in lit_used]
    lit_syms = sorted(lit_used | set(rng.sample(spare, rng.choice((0, 1, 4, 16, 40)))))
    limit = rng.randint(7, 15)
    if len(lit_syms) == 1:
        lit_lens = lens_of({256: 1})
    else:
        lit_lens = lens_of(dict(zip(lit_syms, random_code(rng, len(lit_syms), limit))), rng.randint(max(257, lit_syms[-1] + 1), 286))
    spare = [d for d in range(30) if d not in dist_used]
    if not dist_used and rng.random() < 0.6:
        dist_lens = [0] * rng.choice((1, 1, 2, 7))                               # absent
    elif len(dist_used) <= 1 and rng.random() < 0.7:
        only = min(dist_used) if dist_used else rng.randrange(30)
        dist_lens = lens_of({only: 1}, rng.randint(only + 1, 30))                # lone
    else:
        more = max(2 - len(dist_used), rng.choice((1, 3, 8, 15, 25)))
        dist_syms = sorted(dist_used | set(rng.sample(spare, min(more, len(spare)))))
        dist_lens = lens_of(dict(zip(dist_syms, random_code(rng, len(dist_syms), limit, 0.75))), rng.randint(dist_syms[-1] + 1, 30))
    cl_syms = run_lengths(lit_lens + dist_lens, rng)
    used = sorted(set(s if isinstance(s, int) else s[0] for s in cl_syms) | set(rng.sample(range(19), rng.choice((0, 0, 1, 3)))))
    if len(used) == 1:
        used.append((used[0] + 1) % 19)
    clen_lens = lens_of(dict(zip(used, random_code(rng, len(used), 7))), 19)
    return dynamic_block(w, lit_lens, dist_lens, tokens, final, cl_syms=cl_syms, clen_lens=clen_lens)


@functools.lru_cache(maxsize=None)
def generated_streams(seed=1951, count=256):
    """`count` random BGZF blocks as (raw, text by zlib, block): 1-6 deflate blocks of random type each, every fourth
    behind 32 768 stored bytes of history, a few KB of new text at the most."""
    rng = random.Random(seed)
    H = _history()
    out = []
    for k in range(count):
        w, produced = BitWriter(), 0
        history = k % 4 == 3
        if history:
            stored_block(w, H, 0)
            produced = len(H)
        n = rng.randint(1, 6)
        for j in range(n):
            final = int(j == n - 1)
            kind = rng.choice((0, 1, 2, 2, 2))
            if kind == 0:
                data = rng.randbytes(rng.choice((0, 1, 7, 100, 300)))
                stored_block(w, data, final)
                produced += len(data)
                continue
            tokens, made = _random_tokens(rng, produced, 3000, history)
            if kind == 1:
                fixed_block(w, tokens, final)
            else:
                _random_dynamic(rng, w, tokens, final)
            produced += made
        raw = w.bytes()
        out.append((raw,) + block_of(raw))
    return tuple(out)


# ---- streams to refuse ------------------------------------------------------------------------------------------------
def refusals():
    """name -> (raw deflate stream, size the trailer claims, the device's reason).  zlib refuses each of the streams as
    well, except the last two, which are valid deflate with a size field too small for them."""
    out = {}
    a3 = lens_of({65: 1, 256: 2, 257: 2})
    short = dict(cl_syms=[0, 8] + [(16, 6)] * 42 + [(16, 3), 0])

    def dyn(lit_lens, dist_lens, tokens, **kw):
        kw.setdefault("cl_syms", run_lengths(list(lit_lens) + list(dist_lens)))
        return dynamic_block(BitWriter(), lit_lens, dist_lens, tokens, 1, **kw).value(0, 32).bytes()
    out["lone end-of-block code of 2 bits"] = (dyn([0] * 256 + [2], [0], []), 0, "invalid code lengths")
    out["lone distance code of 2 bits"] = (dyn(a3, [2], [65, (3, 1)]), 4, "invalid code lengths")
    out["two literal/length codes of 2 bits"] = (dyn(lens_of({65: 2, 256: 2}), [0], [65]), 1, "invalid code lengths")
    out["incomplete code-length code"] = (dyn([0] + [8] * 256, [0], [1, 2, 3], clen_lens=lens_of({16: 2, 0: 2, 8: 2}, 19), **short), 3,
                                          "invalid code lengths")
    fixed_lens = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
    out["HLIT field 30"] = (dyn(fixed_lens[:287], [5] * 30, [65]), 1, "invalid code lengths")
    out["HLIT field 31"] = (dyn(fixed_lens, [5] * 30, [65]), 1, "invalid code lengths")
    out["HDIST field 30"] = (dyn(fixed_lens[:286], [5] * 31, [65]), 1, "invalid code lengths")
    out["HDIST field 31"] = (dyn(fixed_lens[:286], [5] * 32, [65]), 1, "invalid code lengths")
    out["16 as the first code-length symbol"] = (dyn([8] * 257, [0], [1, 2, 3], cl_syms=[(16, 3), 8] + [(16, 6)] * 42 + [(16, 3), 0],
                                                     check=False), 3, "invalid code lengths")
    out["a repeat past the last length"] = (dyn([0] + [8] * 256, [0], [1, 2, 3], cl_syms=[0, 8] + [(16, 6)] * 42 + [(16, 5)], check=False), 3,
                                            "invalid code lengths")
    out["no code for symbol 256"] = (dyn(lens_of({65: 1, 66: 1}, 257), [0], [65, 66], eob=False), 2, "invalid code lengths")
    out["lone 1-bit distance code, the other bit"] = (dyn(a3, [1], [65, ("lit", 257), ("bits", 1, 1)]), 4, "invalid symbol")
    out["no distance code, a length symbol"] = (dyn(a3, [0], [65, ("lit", 257), ("bits", 0, 8)]), 4, "invalid symbol")
    out["distance symbol 30 in a fixed block"] = (fixed_block(BitWriter(), [65, ("sym", 0, 0, 30, 0)], 1).value(0, 32).bytes(), 4, "invalid symbol")
    w = stored_block(BitWriter(), b"abc", 0)
    fixed_block(w, [100, 101], 0)
    out["distance produced + 1 in the third deflate block"] = (fixed_block(w, [(3, 6)], 1).bytes(), 8, "distance beyond the start of the block")
    out["a match opens the block"] = (fixed_block(BitWriter(), [(3, 1)], 1).bytes(), 3, "distance beyond the start of the block")
    out["a match ends past the size field"] = (fixed_block(BitWriter(), [65, (4, 1)], 1).bytes(), 4, "output exceeds the size field")
    out["a literal past the size field"] = (fixed_block(BitWriter(), [65, 66, 67], 1).bytes(), 2, "output exceeds the size field")
    return out


OVERFLOWS = ("a match ends past the size field", "a literal past the size field")


def refusal_block(name):
    raw, isize, _ = refusals()[name]
    return wrap(raw, 0, isize)


# ---- a FASTQ file by hand ---------------------------------------------------------------------------------------------
def handbuilt_fastq(text, records=16):
    """FASTQ text as a BGZF file of hand-built blocks of `records` records: every sequence line is a dynamic block under
    the ladder codes (lengths 1 ... 14, 15, 15 on both alphabets) with matches found by a small greedy search, the other
    lines are stored and fixed blocks in turn."""
    lit_syms = [65, 67, 71, 84, 10, 78, 257, 258, 259, 260, 261, 262, 265, 269, 285, 256]
    lengths = sorted(n for s in lit_syms if s > 256 for n in range(LEN_BASE[s - 257], LEN_BASE[s - 257] + (1 << LEN_EXTRA[s - 257])))
    lit_lens, dist_lens = _ladder_codes(lit_syms, list(range(14, 30)))            # distances 129 ... 32 768
    cl_syms = run_lengths(lit_lens + dist_lens)
    lines = text.split(b"\n")
    assert lines.pop() == b"" and len(lines) % 4 == 0
    blocks = []
    for first in range(0, len(lines), 4 * records):
        w, done, seen, turn = BitWriter(), b"", {}, 0
        group = lines[first:first + 4 * records]
        for k, line in enumerate(group):
            line, final = line + b"\n", int(k == len(group) - 1)
            whole = done + line
            if k % 4 == 1:
                tokens, i = [], len(done)
                while i < len(whole):
                    at, n = seen.get(whole[i:i + 4], -1), 0
                    if at >= 0 and i - at >= 129:
                        while n < 258 and i + n < len(whole) and whole[at + n] == whole[i + n]:
                            n += 1
                        n = max([m for m in lengths if m <= n], default=0)
                    tokens.append((n, i - at) if n else whole[i])
                    i += n or 1
                dynamic_block(w, lit_lens, dist_lens, tokens, final, cl_syms=cl_syms)
            elif turn % 2:
                fixed_block(w, list(line), final)
            else:
                stored_block(w, line, final)
            turn += k % 4 != 1
            for p in range(max(0, len(done) - 3), len(whole) - 3):
                seen[whole[p:p + 4]] = p
            done = whole
        blocks.append(block_of(w.bytes())[1])
    return bgzf_file(*blocks)
