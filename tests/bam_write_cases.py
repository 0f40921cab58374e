"""Reads -> unaligned BAM records, restated on the CPU (test helper, not a test): what sarlacc_dev_bam_format_size /
_format and DeviceReads.to_bam have to write, record by record in plain Python, with no thought for how the kernels
divide the work.  Records come from tests/bam_cases.raw_record and tests/bam_reads_cases.pack_seq; nothing here calls
the code under test.

Record i is unmapped and unpaired: refID -1, pos -1, mapq 0, bin 4680, no CIGAR, flag 4, next_refID -1, next_pos -1,
tlen 0, the NUL-terminated name, SEQ as 4-bit codes through "=ACMGRSVTWYHKDBN" (high nibble first), QUAL as byte - 33,
no tags.  The name is the read's name up to its first space or tab, '*' where nothing is left, READ_<first_index + i>
where the batch has no names.  Refusals name the 1-based record, the lowest bad record wins, and within a record the
order is name (length, then bytes), SEQ, QUAL."""
import functools
import struct
import zlib

import numpy as np

from tests import bam_cases as B
from tests import bgzf_write_cases as W
from tests.bam_reads_cases import LETTERS, pack_seq

BIN = 4680                # reg2bin(-1, 0)
FLAG = 4
DEFAULT_HEADER = b"@HD\tVN:1.6\tSO:unsorted\n"
NAME_LONG = "read name longer than 254 bytes"
NAME_BYTE = "read name holds a byte outside '!'..'~'"
BASE = "base cannot be stored in BAM"
QUAL = "quality byte outside Phred+33"
BASES = LETTERS[1:].encode()      # the 15 letters a record can hold ('=' is not one of them)
TABLE_ROOM = 300          # bytes of one table written without any repeat symbol: 19 * 3 + 316 * 7 bits


def kept(name):
    """The bytes of a read's name in front of its first space or tab."""
    for k, c in enumerate(name):
        if c in b" \t":
            return name[:k]
    return name


def qname(name):
    """What the record holds of a read's name: the kept part, '*' where that is nothing."""
    return kept(name) or b"*"


def default_name(index):
    return b"READ_%d" % index


def refusal(name, seq, qual):
    """The message a read is refused with, or None.  `name` None: a default name."""
    if name is not None:
        if len(kept(name)) > 254:
            return NAME_LONG
        if any(c < 33 or c > 126 for c in kept(name)):
            return NAME_BYTE
    if any(c not in BASES for c in seq):
        return BASE
    if any(q < 33 or q > 126 for q in qual):
        return QUAL
    return None


def first_refusal(names, seqs, quals):
    """(1-based record, message) of the lowest refused read, or None."""
    for k, (s, q) in enumerate(zip(seqs, quals)):
        why = refusal(None if names is None else names[k], s, q)
        if why:
            return k + 1, why
    return None


def record(name, seq, qual):
    """One read as a record (its block_size included); `name` as the record holds it."""
    assert len(seq) == len(qual)
    codes = [LETTERS.index(chr(c)) for c in seq]
    return B.raw_record(-1, -1, name + b"\0", 0, FLAG, [], len(seq), pack_seq(codes), bytes(q - 33 for q in qual), bin_=BIN)


def record_list(names, seqs, quals, first_index=1):
    assert first_refusal(names, seqs, quals) is None
    return [record(default_name(first_index + k) if names is None else qname(names[k]), s, q)
            for k, (s, q) in enumerate(zip(seqs, quals))]


def expected_records(names, seqs, quals, first_index=1):
    """The record stream of a batch (no header in it) as bytes.  `names` None: default names from first_index on."""
    return b"".join(record_list(names, seqs, quals, first_index))


def layout(names, seqs, quals, first_index=1):
    """(n + 1 record offsets, 2 n cuts: SEQ start and QUAL start of every record) in the record stream."""
    recs = record_list(names, seqs, quals, first_index)
    off = np.zeros(len(recs) + 1, np.int64)
    if recs:
        np.cumsum([len(r) for r in recs], out=off[1:])
    cuts = np.zeros(2 * len(recs), np.int64)
    for k, s in enumerate(seqs):
        cuts[2 * k + 1] = off[k + 1] - len(s)
        cuts[2 * k] = cuts[2 * k + 1] - (len(s) + 1) // 2
    return off, cuts


def header_bytes(text=None):
    """The header of an unaligned BAM file: magic, l_text, text, n_ref = 0."""
    return B.header_bytes(DEFAULT_HEADER if text is None else text, [])


def draw(rng, lengths, letters=b"ACGT"):
    """(names, seqs, quals) as lists of bytes: names with a comment behind a blank, qualities over all of 33..126."""
    pool = np.frombuffer(letters, np.uint8)
    names = [b"read_%d ch=%d start=%d" % (k, k % 512, 7 * k) for k in range(len(lengths))]
    seqs = [pool[rng.integers(0, pool.size, n)].tobytes() for n in lengths]
    quals = [rng.integers(33, 127, n).astype(np.uint8).tobytes() for n in lengths]
    return names, seqs, quals


def synth_records(nbytes, L, seed):
    """(about `nbytes` of records of `L`-base reads, their 2 n cuts) with the statistics of bgzf_write_cases.synth_fastq:
    a 13-byte name field with a running number, uniform ACGT, qualities from error probabilities ~ U(0, 0.06)."""
    rng = np.random.default_rng(seed)
    name = b"read_0000000\0"
    size = 36 + len(name) + (L + 1) // 2 + L
    n = max(nbytes // size, 1)
    rec = np.zeros((n, size), np.uint8)
    rec[:, :36] = np.frombuffer(record(name[:-1], b"A" * L, b"!" * L)[:36], np.uint8)
    rec[:, 36:36 + len(name)] = np.frombuffer(name, np.uint8)
    idx = np.arange(n)
    for d in range(7):
        rec[:, 36 + 5 + 6 - d] = 48 + (idx // 10 ** d) % 10
    o = 36 + len(name)
    codes = np.array([1, 2, 4, 8], np.uint8)[rng.integers(0, 4, (n, L + (L & 1)))]
    if L & 1:
        codes[:, -1] = 0
    rec[:, o:o + (L + 1) // 2] = (codes[:, 0::2] << 4) | codes[:, 1::2]
    err = np.maximum(rng.random((n, L)) * 0.06, 1e-9)
    rec[:, o + (L + 1) // 2:] = np.clip(np.rint(-10 * np.log10(err)), 0, 60).astype(np.uint8)
    cuts = np.empty(2 * n, np.int64)
    cuts[0::2] = idx * size + o
    cuts[1::2] = idx * size + o + (L + 1) // 2
    return rec.reshape(-1).tobytes(), cuts


@functools.lru_cache(maxsize=None)
def seeded_records(L, blocks=8):
    """Exactly `blocks` BGZF blocks of the synthetic record stream of `L`-base reads (the last record may be cut) and
    the cuts of all its records (those behind the end included: a writer has to ignore them)."""
    raw, cuts = synth_records(blocks * W.BLOCK + 2 * L + 100, L, 1000)
    return raw[:blocks * W.BLOCK], cuts


def piece_ends(cuts, n, origin=0):
    """Where the pieces of a block of n bytes end, the block starting at stream offset `origin`: at the first cut that
    lies at least 64 bytes into the piece, and at n."""
    ends, b = [], 0
    for c in (int(c) - origin for c in cuts):
        if b + 64 <= c < n:
            ends.append(c)
            b = c
    return ends + [n]


@functools.lru_cache(maxsize=None)
def yardsticks(L, blocks=8):
    """Bytes of seeded_records(L) as BGZF by zlib, per block raw deflate + 26: level 6, Z_HUFFMAN_ONLY as zlib cuts it,
    and Z_HUFFMAN_ONLY with a new deflate block at every piece end."""
    raw, cuts = seeded_records(L, blocks)
    tot = {"level6": 0, "huffman": 0, "per_field": 0}
    for k, p in enumerate(W.pieces(raw)):
        tot["level6"] += len(W.zlib_raw(p, 6)) + W.FRAMING
        tot["huffman"] += len(W.zlib_raw(p, 6, zlib.Z_HUFFMAN_ONLY)) + W.FRAMING
        tot["per_field"] += len(W.zlib_raw(p, 6, zlib.Z_HUFFMAN_ONLY, piece_ends(cuts, len(p), k * W.BLOCK)[:-1])) + W.FRAMING
    return tot


def block_parts(block):
    """(raw deflate payload, CRC-32, ISIZE) of one BGZF block as the writer lays it out (18 bytes of header)."""
    crc, isize = struct.unpack("<II", block[-8:])
    return block[18:-8], crc, isize


# ---- the batches of the tests ------------------------------------------------------------------------------------------

LENGTHS = (0, 1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 4095, 4096, 4097, 12289)


@functools.lru_cache(maxsize=None)
def batch_lengths():
    """A read of every length of LENGTHS and a few more: all 15 letters, qualities over 33..126 with both ends present,
    names of 1 and 254 bytes, an empty one, one that is a comment only, one with a blank and a comment."""
    rng = np.random.default_rng(11)
    lengths = list(LENGTHS) + [200, 7, 1000]
    names, seqs, quals = draw(rng, lengths, BASES)
    seqs[-1] = BASES * 66 + BASES[:10]
    quals[-1] = bytes([33, 126]) * 500
    names[1], names[2], names[3], names[4] = b"x", b"n" * 254, b"", b"\tcomment only"
    names[5] = b"read_5 ch=12 start_time=1234"
    names[6] = b"y\tcomment"
    return names, seqs, quals


@functools.lru_cache(maxsize=None)
def batch_tiny():
    """3 000 reads of 0 .. 3 bases: a 4-KB tile of the stream holds more than 64 records."""
    rng = np.random.default_rng(12)
    n = 3000
    seqs = [np.frombuffer(BASES, np.uint8)[rng.integers(0, 15, k)].tobytes() for k in rng.integers(0, 4, n)]
    quals = [rng.integers(33, 127, len(s)).astype(np.uint8).tobytes() for s in seqs]
    names = [b"t%d" % k for k in range(n)]
    return names, seqs, quals


@functools.lru_cache(maxsize=None)
def batch_span():
    """One read that spans more than three 4-KB tiles of the stream, short reads on both sides of it."""
    return draw(np.random.default_rng(13), [5, 0, 40, 3, 14001, 2, 0, 33, 9], BASES)


@functools.lru_cache(maxsize=None)
def batch_forty():
    return draw(np.random.default_rng(14), np.random.default_rng(15).integers(0, 120, 40).tolist(), BASES)


@functools.lru_cache(maxsize=None)
def batch_file():
    """60 reads of 0 .. 5 000 bases with names, an empty read among them."""
    lengths = np.random.default_rng(16).integers(0, 5001, 60).tolist()
    lengths[7] = 0
    return draw(np.random.default_rng(17), lengths, BASES)


BATCHES = {"lengths": batch_lengths, "tiny": batch_tiny, "span": batch_span, "forty": batch_forty, "file": batch_file}
