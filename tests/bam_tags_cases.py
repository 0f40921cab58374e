"""BAM tags restated on the CPU (test helper, not a test): what the tag calls of include/sarlacc_amd.h ("tags of a
resident batch") have to report and write, in plain Python with no thought for how the kernels divide the work.  Nothing
here calls the code under test.  Entries are built by tests/bam_cases.encode_tag, records by bam_cases.raw_record
(tags=...) as tests/bam_write_cases.record builds them.

An aux area is a run of entries: tag (two bytes), type letter, value (SAM specification section 4.2.4).  It is malformed
when fewer than 3 bytes are left in front of its end, the type letter is not one of AcCsSiIfZHB, a fixed value or a B
header or payload runs past the end, a B subtype is not one of cCsSiIf, or a Z / H has no NUL in front of the end."""
import struct

import numpy as np

from tests import bam_cases as B
from tests import bam_write_cases as BW
from tests.bam_reads_cases import LETTERS, pack_seq

FIXED = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}
SUBTYPES = "cCsSiIf"
MALFORMED = "malformed tags"


class Malformed(Exception):
    pass


def walk(aux):
    """The entries of an aux area as (tag, type, start, value start, value bytes, end); value bytes are those of
    Z / H without the NUL and of B with its 5-byte header.  Malformed where the rules above say so."""
    out, p, end = [], 0, len(aux)
    while p < end:
        if end - p < 3:
            raise Malformed("fewer than 3 bytes")
        tag, ty = bytes(aux[p:p + 2]), chr(aux[p + 2])
        v = p + 3
        if ty in FIXED:
            vlen = size = FIXED[ty]
        elif ty in "ZH":
            q = v
            while q < end and aux[q] != 0:
                q += 1
            if q >= end:
                raise Malformed("no NUL")
            vlen, size = q - v, q - v + 1
        elif ty == "B":
            if end - v < 5:
                raise Malformed("B header")
            sub = chr(aux[v])
            if sub not in SUBTYPES:
                raise Malformed("B subtype")
            vlen = size = 5 + struct.unpack_from("<I", aux, v + 1)[0] * FIXED[sub]
        else:
            raise Malformed("type letter")
        if size > end - v:
            raise Malformed("value past the end")
        out.append((tag, ty, p, v, vlen, v + size))
        p = v + size
    return out


def find(aux, tag):
    """(type letter code, value offset, value bytes, entry offset, entry bytes) of the first entry named `tag`, all 0
    when there is none -- after the whole area has been walked."""
    for t, ty, at, v, vlen, nxt in walk(aux):
        if t == tag:
            return ord(ty), v, vlen, at, nxt - at
    return 0, 0, 0, 0, 0


def first_malformed(areas):
    """1-based number of the lowest read with malformed tags, or None."""
    for k, a in enumerate(areas):
        try:
            walk(a)
        except Malformed:
            return k + 1
    return None


def z_entry(tag, value):
    return tag + b"Z" + value + b"\0"


def i_entry(tag, value):
    return tag + b"i" + struct.pack("<i", value)


def splice(areas, src=None, cuts=None, tag=None, kind=None, column=None, mask=None):
    """The aux areas a splice writes: read r is areas[src[r]] without the span cuts[r] = (offset, bytes), followed
    where mask[r] by the new entry `tag` of type `kind` ('Z': bytes, 'i': int) with the value column[r]."""
    src = range(len(areas)) if src is None else src
    out = []
    for r, s in enumerate(src):
        a = areas[s]
        if cuts is not None:
            a = a[:cuts[r][0]] + a[cuts[r][0] + cuts[r][1]:]
        if kind is not None and (mask is None or mask[r]):
            a = a + (z_entry(tag, column[r]) if kind == "Z" else i_entry(tag, int(column[r])))
        out.append(a)
    return out


def set_tag(areas, tag, kind, column, mask=None):
    """set_tag restated: the first entry named `tag` replaced where mask[r], the new one appended."""
    cuts = []
    for r, a in enumerate(areas):
        _, _, _, at, n = find(a, tag)
        cuts.append((at, n) if mask is None or mask[r] else (0, 0))
    return splice(areas, cuts=cuts, tag=tag, kind=kind, column=column, mask=mask)


def drop_tag(areas, tag):
    return [b"".join(a[at:nxt] for t, _, at, _, _, nxt in walk(a) if t != tag) for a in areas]


def string_values(areas, tag):
    """(values as bytes, present) of a string tag; the value of A is its one byte."""
    vals, present = [], []
    for a in areas:
        ty, v, vlen, _, _ = find(a, tag)
        assert ty == 0 or chr(ty) in "AZH"
        vals.append(a[v:v + vlen])
        present.append(ty != 0)
    return vals, np.array(present, bool)


_INT_FMT = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I"}


def int_values(areas, tag):
    vals, present = [], []
    for a in areas:
        ty, v, _, _, _ = find(a, tag)
        assert ty == 0 or chr(ty) in _INT_FMT
        vals.append(struct.unpack_from(_INT_FMT[chr(ty)], a, v)[0] if ty else 0)
        present.append(ty != 0)
    return np.array(vals, np.int64), np.array(present, bool)


# ---- the writer with tags ------------------------------------------------------------------------------------------------

TWICE = "tag %s appears twice"


def tags_refusal(aux):
    """The message the writer refuses an aux area with, or None: malformed first, then the first entry whose tag an
    earlier entry carries."""
    try:
        entries = walk(aux)
    except Malformed:
        return MALFORMED
    seen = set()
    for t, *_ in entries:
        if t in seen:
            return TWICE % t.decode("latin-1")
        seen.add(t)
    return None


def first_refusal(names, seqs, quals, areas):
    """(1-based record, message) of the lowest refused read: bam_write_cases' order, then the tags."""
    for k, (s, q, a) in enumerate(zip(seqs, quals, areas)):
        why = BW.refusal(None if names is None else names[k], s, q) or tags_refusal(a)
        if why:
            return k + 1, why
    return None


def record(name, seq, qual, aux):
    """bam_write_cases.record with the aux bytes behind QUAL."""
    codes = [LETTERS.index(chr(c)) for c in seq]
    return B.raw_record(-1, -1, name + b"\0", 0, BW.FLAG, [], len(seq), pack_seq(codes), bytes(q - 33 for q in qual), aux, bin_=BW.BIN)


def record_list(names, seqs, quals, areas, first_index=1):
    assert first_refusal(names, seqs, quals, areas) is None
    plain = BW.record_list(names, seqs, quals, first_index)
    out = [record(BW.default_name(first_index + k) if names is None else BW.qname(names[k]), s, q, a)
           for k, (s, q, a) in enumerate(zip(seqs, quals, areas))]
    # the record is what it is without tags, with the aux bytes behind QUAL and counted in block_size
    assert all(r[4:] == p[4:] + a and struct.unpack_from("<i", r)[0] == len(p) - 4 + len(a) for r, p, a in zip(out, plain, areas))
    return out


def layout(names, seqs, quals, areas, first_index=1):
    """(n + 1 record offsets, 3 n cuts: SEQ start, QUAL start and tag start of every record) in the record stream."""
    recs = record_list(names, seqs, quals, areas, first_index)
    off = np.zeros(len(recs) + 1, np.int64)
    if recs:
        np.cumsum([len(r) for r in recs], out=off[1:])
    cuts = np.zeros(3 * len(recs), np.int64)
    for k, (s, a) in enumerate(zip(seqs, areas)):
        cuts[3 * k + 2] = off[k + 1] - len(a)
        cuts[3 * k + 1] = cuts[3 * k + 2] - len(s)
        cuts[3 * k] = cuts[3 * k + 1] - (len(s) + 1) // 2
    return off, cuts


# ---- generators ----------------------------------------------------------------------------------------------------------

def random_field(rng, tag):
    """One TAG:TYPE:VALUE field that bam_cases.encode_tag can encode, over every type and B subtype."""
    ty = rng.choice(list("AifZHB"))
    if ty == "A":
        val = chr(int(rng.integers(33, 127)))
    elif ty == "i":
        val = str(int(rng.choice([0, 1, -1, 127, 128, -128, -129, 255, 256, 65535, 65536, -32768, -32769, 2 ** 31 - 1, -2 ** 31,
                                  2 ** 32 - 1, int(rng.integers(-2 ** 31, 2 ** 32))])))
    elif ty == "f":
        val = repr(float(np.float32(rng.normal())))
    elif ty == "Z":
        val = "".join(chr(int(c)) for c in rng.integers(32, 127, int(rng.integers(0, 40)))).replace("\t", " ")
    elif ty == "H":
        val = "".join(rng.choice(list("0123456789ABCDEF"), 2 * int(rng.integers(0, 9))))
    else:
        sub = str(rng.choice(list(SUBTYPES)))
        lo, hi = {"c": (-128, 128), "C": (0, 256), "s": (-32768, 32768), "S": (0, 65536), "i": (-2 ** 31, 2 ** 31),
                  "I": (0, 2 ** 32), "f": (0, 100)}[sub]
        val = ",".join([sub] + [str(int(v)) for v in rng.integers(lo, hi, int(rng.integers(0, 12)))])
    return "%s:%s:%s" % (tag, ty, val)


TAG_POOL = ["RG", "ch", "st", "qs", "mv", "MM", "ML", "RX", "BC", "NM", "ts", "du", "pi", "sp", "X0", "a9"]


def random_fields(rng, max_tags=8):
    """A list of fields with distinct tags."""
    tags = rng.permutation(TAG_POOL)[:int(rng.integers(0, max_tags + 1))]
    return [random_field(rng, str(t)) for t in tags]


def encode(fields):
    return b"".join(B.encode_tag(f) for f in fields)


def random_areas(rng, n, empty=0.2, max_tags=8):
    return [b"" if rng.random() < empty else encode(random_fields(rng, max_tags)) for _ in range(n)]


def basecaller_aux(rng, L, k):
    """A basecaller-like tag set for a read of L bases: a few short tags, RG:Z, mv:B:c of one entry per 6 bases, MM:Z, ML:B:C."""
    nmod = L // 25
    fields = ["qs:f:%r" % float(np.float32(rng.uniform(5, 30))), "du:f:%r" % float(np.float32(rng.uniform(0.1, 20))),
              "ns:i:%d" % (6 * L), "ts:i:%d" % rng.integers(0, 500), "mx:i:1", "ch:i:%d" % (k % 512), "st:Z:2026-01-01T00:00:%02d.000+00:00" % (k % 60),
              "rn:i:%d" % k, "fn:Z:file_%d.pod5" % (k % 7), "sm:f:%r" % float(np.float32(rng.normal(90, 5))), "sd:f:%r" % float(np.float32(rng.normal(20, 2))),
              "sv:Z:pa", "dx:i:0", "RG:Z:run1_model_v5", "mv:B:c," + ",".join(["6"] + [str(int(v)) for v in rng.integers(0, 2, L // 6)]),
              "MM:Z:C+m?" + "".join(",%d" % v for v in rng.integers(0, 30, nmod)) + ";", "ML:B:C" + "".join(",%d" % v for v in rng.integers(0, 256, nmod))]
    return encode(fields)
