"""Texts and yardsticks of the BGZF writer's tests (sarlacc_dev_bgzf_deflate): the synthetic FASTQ of
tools/perf_bgzf_ingest.py, zlib's own raw deflate of the same 65 280-byte pieces to measure against, the texts that
drive the two length limiters, and a reader of zlib's table headers.  Nothing here calls the code under test."""
import functools
import heapq
import zlib

import numpy as np

from tests.bgzf_cases import CLEN_ORDER, REPEAT

BLOCK = 0xff00            # text bytes per BGZF block
FRAMING = 26              # 18 bytes of header, 8 of trailer
STORED = 5                # a stored deflate block around the bytes


def synth_fastq(nbytes, L, seed):
    """About `nbytes` of 4-line FASTQ of `L`-base reads with the statistics of tools/perf_bgzf_ingest.py: a 36-byte name
    line with a running number, uniform ACGT, qualities from error probabilities ~ U(0, 0.06) as Phred+33."""
    rng = np.random.default_rng(seed)
    name = np.frombuffer(b"@read_0000000 ch=12 start_time=1234\n", dtype=np.uint8)
    n = max(nbytes // (name.size + 2 * L + 4), 1)
    rec = np.empty((n, name.size + L + 1 + 2 + L + 1), np.uint8)
    rec[:, :name.size] = name
    idx = np.arange(n)
    for d in range(7):
        rec[:, 6 + 6 - d] = 48 + (idx // 10 ** d) % 10
    o = name.size
    rec[:, o:o + L] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, (n, L))]
    rec[:, o + L] = 10
    rec[:, o + L + 1] = ord("+")
    rec[:, o + L + 2] = 10
    err = np.maximum(rng.random((n, L)) * 0.06, 1e-9)
    rec[:, o + L + 3:o + 2 * L + 3] = (33 + np.clip(np.rint(-10 * np.log10(err)), 0, 60)).astype(np.uint8)
    rec[:, -1] = 10
    return rec.reshape(-1).tobytes()


@functools.lru_cache(maxsize=None)
def seeded_text(L, blocks=8):
    """Exactly `blocks` BGZF blocks of the synthetic FASTQ of `L`-base reads (the last record may be cut)."""
    return synth_fastq(blocks * BLOCK + 2 * L + 100, L, 1000)[:blocks * BLOCK]


def pieces(text):
    return [text[i:i + BLOCK] for i in range(0, len(text), BLOCK)]


def zlib_raw(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, cuts=()):
    """Raw deflate with memLevel 9; `cuts`: offsets at which a new deflate block is forced (flush(Z_BLOCK))."""
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    out, start = [], 0
    for cut in cuts:
        out.append(c.compress(data[start:cut]) + c.flush(zlib.Z_BLOCK))
        start = cut
    out.append(c.compress(data[start:]) + c.flush())
    raw = b"".join(out)
    assert zlib.decompress(raw, -15) == data
    return raw


def line_starts(piece):
    """Offsets inside `piece` at which a line begins (0 and the end left out)."""
    a = np.flatnonzero(np.frombuffer(piece, np.uint8) == 10) + 1
    return [int(x) for x in a if x < len(piece)]


@functools.lru_cache(maxsize=None)
def yardsticks(L, blocks=8):
    """Bytes of seeded_text(L) as BGZF by zlib, per block raw deflate + 26: level 6, level 1, Z_HUFFMAN_ONLY as zlib cuts
    it, and Z_HUFFMAN_ONLY with a new deflate block at every line start."""
    tot = {"level6": 0, "level1": 0, "huffman": 0, "per_line": 0}
    for p in pieces(seeded_text(L, blocks)):
        tot["level6"] += len(zlib_raw(p, 6)) + FRAMING
        tot["level1"] += len(zlib_raw(p, 1)) + FRAMING
        tot["huffman"] += len(zlib_raw(p, 6, zlib.Z_HUFFMAN_ONLY)) + FRAMING
        tot["per_line"] += len(zlib_raw(p, 6, zlib.Z_HUFFMAN_ONLY, line_starts(p))) + FRAMING
    return tot


def huffman_depth(freqs):
    """Depth of the deepest leaf of an unlimited Huffman code over the non-zero frequencies."""
    heap = [(f, 0) for f in freqs if f > 0]
    if len(heap) < 2:
        return len(heap)
    heapq.heapify(heap)
    while len(heap) > 1:
        (fa, da), (fb, db) = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (fa + fb, max(da, db) + 1))
    return heap[0][1]


class _Bits:
    def __init__(self, raw):
        self.v, self.pos = int.from_bytes(raw, "little"), 0

    def take(self, n):
        x = (self.v >> self.pos) & ((1 << n) - 1)
        self.pos += n
        return x


def first_table(raw):
    """The table header of the first deflate block of `raw`, which must be dynamic: (lengths of the code-length code by
    symbol, how often the header uses every code-length symbol, the literal/length lengths, the distance lengths)."""
    b = _Bits(raw)
    b.take(1)
    assert b.take(2) == 2, "not a dynamic block"
    hlit, hdist, hclen = b.take(5) + 257, b.take(5) + 1, b.take(4) + 4
    clens = [0] * 19
    for i in range(hclen):
        clens[CLEN_ORDER[i]] = b.take(3)
    code, decode = 0, {}
    for l in range(1, 8):                      # canonical codes, read MSB first
        for s in range(19):
            if clens[s] == l:
                decode[(l, code)] = s
                code += 1
        code <<= 1
    lens, used = [], [0] * 19
    while len(lens) < hlit + hdist:
        c, l = 0, 0
        while (l, c) not in decode:
            c, l = (c << 1) | b.take(1), l + 1
            assert l <= 7
        s = decode[(l, c)]
        used[s] += 1
        if s < 16:
            lens.append(s)
        else:
            base, extra = REPEAT[s]
            lens += [lens[-1] if s == 16 else 0] * (base + b.take(extra))
    assert len(lens) == hlit + hdist
    return clens, used, lens[:hlit], lens[hlit:]


def fibonacci_bytes(values=22, first=40):
    """Byte values first, first + 1, ... with the counts 1, 1, 2, 3, 5, ...: 22 of them sum to 46 367 and are, with
    end-of-block's 1, the 23 symbols of the literal code (a 23rd Fibonacci count would bring the sum to 75 024, beyond a
    block).  A Huffman code over them is up to 22 bits deep, depending on how ties are broken.  [(value, count)]."""
    fib = [1, 1]
    while len(fib) < values:
        fib.append(fib[-1] + fib[-2])
    return list(zip(range(first, first + values), fib))


def deep_bytes(values=20, first=40):
    """Counts 1, 3, 5, 9, 15, ... (each the sum of the two before it and 1, end-of-block's 1 being the first of the
    series): no ties, so EVERY Huffman code over the 20 values (sum 57 290) and end-of-block is the chain, 20 bits deep,
    and a 15-bit limiter has to act whatever it does with ties.  [(value, count)]."""
    s = [1, 1]
    while len(s) < values + 1:
        s.append(s[-1] + s[-2] + 1)
    return list(zip(range(first, first + values), s[1:]))


def spread(counts, seed):
    """The bytes of [(value, count)] in a seeded random order, no newline among them unless it is a value."""
    a = np.concatenate([np.full(c, v, np.uint8) for v, c in counts])
    return a[np.random.default_rng(seed).permutation(a.size)].tobytes()


# A block whose CODE LENGTHS are skewed, so that the code over the length alphabet wants more than 7 bits.
# NUMBER_OF_LENGTH[L] byte values get the count 2^(15 - L), which makes L their exact Huffman length: the counts and
# end-of-block's 1 sum to 2^15, a dyadic distribution (found by a search over the assignments of the class sizes to
# lengths whose Kraft sum is one).  The values are every second byte from 2 on, so each length stands alone between
# zeros: no repeat symbol 16, a literal 0 after each.  With end-of-block among the 15s the header uses the code-length
# symbols 1, 15, 11, 9, 5, 12, 13 and 0 about 1, 4, 5, 9, 15, 25, 41 and 100 times and 17 or 18 once or twice: each
# count beyond the sum of the two before it, so the Huffman code over them is a chain at least 8 bits deep (the exact
# counts of 0, 1, 17 and 18 depend on how an encoder cuts the runs of zeros at either end).
NUMBER_OF_LENGTH = {1: 1, 5: 15, 9: 9, 11: 5, 12: 25, 13: 41, 15: 3}


def clen_limiter_bytes():
    """[(value, count)] of the block described above."""
    out, v = [], 2
    for L, k in sorted(NUMBER_OF_LENGTH.items(), reverse=True):     # the longest lengths at the lowest values
        for _ in range(k):
            if v == 10:
                v += 2
            out.append((v, 1 << (15 - L)))
            v += 2
    assert v <= 257
    return out
