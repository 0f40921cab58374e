"""BAM records -> reads, restated on the CPU (test helper, not a test): what DeviceReads.from_bam has to return for the
raw bytes of a BAM file, written record by record in plain Python and numpy, with no thought for how the kernels
divide the work.  Files are built with tests/bam_cases.raw_record / header_bytes and tests/bgzf_cases.bgzf_compress.

A record becomes a read unless flag & exclude_flags.  SEQ: 4-bit codes through "=ACMGRSVTWYHKDBN", high nibble first;
with flag & 0x10 the bases are reversed and each code's four bits reversed (the complement).  QUAL: value + 33, reversed
with 0x10; a first byte of 0xff means no qualities, every one is then missing_qual + 33.  Refusals name the 1-based
record, the lowest bad record wins, and within a record the order is layout, SEQ, QUAL."""
import struct

import numpy as np

from tests import bam_cases as B

LETTERS = "=ACMGRSVTWYHKDBN"
LAYOUT = "record fields do not fit its block size"
SEQ_EQ = "SEQ holds '='"
QUAL_HIGH = "quality value above 93"
SIZE = "block size below 32"
CUT = "file ends inside the record"


def complement(code):
    """The code whose four bits are those of `code` in reverse order."""
    return int("{:04b}".format(code)[::-1], 2)


def pack_seq(codes):
    """4-bit codes as SEQ bytes: two per byte, high nibble first, the low nibble of an odd last byte 0."""
    codes = list(codes) + [0] * (len(codes) & 1)
    return bytes((codes[i] << 4) | codes[i + 1] for i in range(0, len(codes), 2))


def seq_codes(text):
    return [LETTERS.index(c) for c in text]


def read_record(name, flag, codes, quals, **kw):
    """An unaligned-style record (no reference, no CIGAR) of the codes and the quality values (None: the 0xff marker)."""
    qual = b"\xff" * len(codes) if quals is None else bytes(quals)
    return B.raw_record(-1, -1, name + b"\0", 0, flag, [], len(codes), pack_seq(codes), qual, **kw)


def records_of(raw):
    """([block of every complete record], how the chain ends: None, SIZE or CUT) of uncompressed BAM bytes."""
    assert raw[:4] == B.MAGIC
    l_text, = struct.unpack_from("<i", raw, 4)
    p = 8 + l_text
    n_ref, = struct.unpack_from("<i", raw, p)
    p += 4
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", raw, p)
        p += 8 + l_name
    out = []
    while p < len(raw):
        if p + 4 > len(raw):
            return out, CUT
        bs, = struct.unpack_from("<i", raw, p)
        if bs < 32:
            return out, SIZE
        if p + 4 + bs > len(raw):
            return out, CUT
        out.append(raw[p + 4:p + 4 + bs])
        p += 4 + bs
    return out, None


def one_read(block, exclude_flags, missing_qual):
    """A record's block -> None (dropped), (name, seq, qual) or the message of its refusal."""
    _, _, l_name, _, _, n_cig, flag, l_seq = struct.unpack_from("<iiBBHHHi", block, 0)
    at = 32 + l_name + 4 * n_cig
    if l_name == 0 or l_seq < 0 or at + (l_seq + 1) // 2 + l_seq > len(block) or block[32 + l_name - 1] != 0:
        return LAYOUT
    if flag & exclude_flags:
        return None
    packed = block[at:at + (l_seq + 1) // 2]
    codes = [(packed[i // 2] >> (0 if i & 1 else 4)) & 15 for i in range(l_seq)]
    if 0 in codes:
        return SEQ_EQ
    quals = list(block[at + len(packed):at + len(packed) + l_seq])
    if quals and quals[0] == 0xff:
        quals = [missing_qual] * l_seq
    elif any(q > 93 for q in quals):
        return QUAL_HIGH
    if flag & 0x10:
        codes = [complement(c) for c in reversed(codes)]
        quals = quals[::-1]
    return block[32:32 + l_name - 1], "".join(LETTERS[c] for c in codes).encode(), bytes(q + 33 for q in quals)


def reads(raw, exclude_flags=0x900, missing_qual=1):
    """Uncompressed BAM bytes -> (names, seqs, quals) as lists of bytes, or (record, message) of the refusal."""
    blocks, end = records_of(raw)
    names, seqs, quals = [], [], []
    for k, block in enumerate(blocks):
        r = one_read(block, exclude_flags, missing_qual)
        if isinstance(r, str):
            return k + 1, r
        if r is not None:
            names.append(r[0])
            seqs.append(r[1])
            quals.append(r[2])
    if end is not None:
        return len(blocks) + 1, end
    return names, seqs, quals


def random_read(rng, length, flag=0, name=None, missing=False):
    """A record of random codes 1..15 and qualities 0..93."""
    codes = rng.integers(1, 16, length).tolist()
    quals = None if missing else rng.integers(0, 94, length).tolist()
    return read_record(name if name is not None else b"r", flag, codes, quals)


def flat(strings):
    """A list of bytes as (bytes, offsets)."""
    off = np.zeros(len(strings) + 1, np.int64)
    if strings:
        np.cumsum([len(s) for s in strings], out=off[1:])
    return b"".join(strings), off
