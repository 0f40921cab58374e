"""Builders of BAM test files (test helper, not a test): an encoder from SAM text to BAM bytes (SAM specification
section 4.2), a pure-Python decoder back to SAM text for the self-check, and a generator of SAM records that BAM can
hold.  Expected values always come from tests/sam_restated.sam2ranges on the equivalent SAM text; a refusal's record
number is the restatement's file line counted over the alignment records (record_of_line)."""
import re
import struct

import numpy as np

from tests import sam_restated as R
from tests.bgzf_cases import bgzf_compress

MAGIC = b"BAM\1"
OPS = "MIDNSHP=X"
BASES = "=ACMGRSVTWYHKDBN"
INT_MAX = 2 ** 31 - 1
_INT = re.compile(r"[+-]?[0-9]+")
_CIGAR = re.compile(r"([0-9]+[MIDNSHP=X])+")
_OP = re.compile(r"([0-9]+)([MIDNSHP=X])")
_B_FMT = {"c": "b", "C": "B", "s": "h", "S": "H", "i": "i", "I": "I", "f": "f"}
_SEQ_CODES = bytes(BASES.index(chr(c)) if chr(c) in BASES else 15 for c in range(256))
_QUAL_MINUS_33 = bytes((c - 33) & 255 for c in range(256))
_B_SIZE = {"c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}


def _int(s, lo, hi):
    if not _INT.fullmatch(s):
        return None
    v = int(s)
    return v if lo <= v <= hi else None


def encode_tag(field):
    """One TAG:TYPE:VALUE field as BAM bytes, None when it is not a tag BAM can hold."""
    m = re.fullmatch(r"([A-Za-z][A-Za-z0-9]):([AifZHB]):(.*)", field, re.S)
    if m is None:
        return None
    tag, ty, val = m.group(1).encode(), m.group(2), m.group(3)
    try:
        if ty == "A":
            return tag + b"A" + val.encode() if len(val) == 1 else None
        if ty == "i":
            v = int(val)
            for letter, fmt, lo, hi in (("C", "B", 0, 255), ("c", "b", -128, 127), ("S", "H", 0, 65535), ("s", "h", -32768, 32767),
                                        ("I", "I", 0, 2 ** 32 - 1), ("i", "i", -2 ** 31, INT_MAX)):
                if lo <= v <= hi:
                    return tag + letter.encode() + struct.pack("<" + fmt, v)
            return None
        if ty == "f":
            return tag + b"f" + struct.pack("<f", float(val))
        if ty in "ZH":
            return tag + ty.encode() + val.encode() + b"\0"
        sub, *vals = val.split(",")
        conv = float if sub == "f" else int
        return tag + b"B" + sub.encode() + struct.pack("<I", len(vals)) + struct.pack("<%d%s" % (len(vals), _B_FMT[sub]), *map(conv, vals))
    except (ValueError, KeyError, struct.error):
        return None


def raw_record(refid, pos, name, mapq, flag, cigar, l_seq=0, seq=b"", qual=b"", tags=b"", n_cigar_op=None, bin_=0,
               next_refid=-1, next_pos=-1, tlen=0, block_size=None):
    """One BAM record from its binary parts: `name` the read-name bytes with their NUL, `cigar` a list of
    (length, op code) or ready bytes.  n_cigar_op and block_size may be set apart from what follows them (malformed
    records)."""
    cig = cigar if isinstance(cigar, bytes) else b"".join(struct.pack("<I", (a << 4) | b) for a, b in cigar)
    n = len(cig) // 4 if n_cigar_op is None else n_cigar_op
    body = struct.pack("<iiBBHHHiiii", refid, pos, len(name) & 255, mapq, bin_, n, flag, l_seq, next_refid, next_pos, tlen) + \
        name + cig + seq + qual + tags
    return struct.pack("<i", len(body) if block_size is None else block_size) + body


def header_bytes(text, refs):
    """magic, l_text, text, n_ref and the reference list [(name, length)]."""
    out = [MAGIC, struct.pack("<i", len(text)), text, struct.pack("<i", len(refs))]
    for name, length in refs:
        nm = name.encode() + b"\0"
        out.append(struct.pack("<i", len(nm)) + nm + struct.pack("<i", length))
    return b"".join(out)


def encode_record(line, names, cg_at=None):
    """One SAM body line (bytes) as a BAM record; `names` the seqinfo names with '*' last.  None for what BAM cannot hold.
    A CG tag goes behind the other tags, or in front of tag number `cg_at`."""
    f = line.decode().split("\t")
    if len(f) < 6:
        return None
    f += ["*", "0", "0", "*", "*"][len(f) - 6:] if len(f) < 11 else []
    qname, rname, cigar, rnext, seq, qual = f[0].encode(), f[2], f[5], f[6], f[9], f[10]
    flag, mapq, pos = _int(f[1], 0, 65535), _int(f[4], 0, 255), _int(f[3], -INT_MAX, INT_MAX + 1)
    pnext, tlen = _int(f[7], -INT_MAX, INT_MAX), _int(f[8], -INT_MAX - 1, INT_MAX)
    if None in (flag, mapq, pos, pnext, tlen) or len(qname) > 254 or b"\0" in qname:
        return None
    nref = len(names) - 1
    refid = -1 if rname == "*" else names.index(rname) if rname in names else nref + 7      # not in the header: out of range
    next_refid = -1 if rname == "*" else refid if rnext == "=" else names.index(rnext) if rnext in names[:-1] else -1
    if cigar == "*":
        ops = []
    elif _CIGAR.fullmatch(cigar):
        ops = [(int(a), OPS.index(b)) for a, b in _OP.findall(cigar)]
        if any(a >= 1 << 28 for a, _ in ops):
            return None
    else:
        return None
    if seq == "*":
        if qual != "*":
            return None
        l_seq, seqb, qualb = 0, b"", b""
    else:
        l_seq = len(seq)
        try:
            codes = np.frombuffer(seq.upper().encode("latin-1").translate(_SEQ_CODES) + b"\0", np.uint8)
            qb = qual.encode("latin-1")
        except UnicodeEncodeError:
            return None
        seqb = ((codes[0:l_seq:2] << 4) | codes[1:l_seq + 1:2]).tobytes()
        if qual == "*":
            qualb = b"\xff" * l_seq
        elif len(qb) == l_seq and 33 <= min(qb) and max(qb) <= 126:
            qualb = qb.translate(_QUAL_MINUS_33)
        else:
            return None
    tags = []
    for t in f[11:]:
        b = encode_tag(t)
        if b is None or t.startswith("CG:"):
            return None
        tags.append(b)
    if len(ops) > 65535:      # the real CIGAR goes into a CG tag behind a two-op stand-in
        width = sum(a for a, b in ops if OPS[b] in "MDN=X")
        if width >= 1 << 28:
            return None
        tags.insert(len(tags) if cg_at is None else cg_at,
                    b"CGBI" + struct.pack("<I", len(ops)) + np.array([(a << 4) | b for a, b in ops], "<u4").tobytes())
        ops = [(l_seq, 4), (width, 3)]
    return raw_record(refid, pos - 1, qname + b"\0", mapq, flag, ops, l_seq, seqb, qualb, b"".join(tags), next_refid=next_refid,
                      next_pos=pnext - 1, tlen=tlen)


def split_sam(text):
    """(header lines, seqinfo names, seqinfo lengths, non-blank body lines) of SAM text, read as the restatement reads it."""
    lines = R.read_lines(text)
    n = 0
    while n < len(lines) and lines[n].startswith(b"@"):
        n += 1
    names, lengths = R.seqinfo([(i + 1, ln) for i, ln in enumerate(lines[:n])])
    return lines[:n], names, lengths, [ln for ln in lines[n:] if ln != b""]


def sam_to_bam(text):
    """The SAM text as (header bytes, list of record bytes): header text, reference list from the @SQ lines, records.
    None for text that BAM cannot hold."""
    try:
        head, names, lengths, body = split_sam(text)
    except R.SamError:
        return None
    recs = [encode_record(ln, names) for ln in body]
    if any(r is None for r in recs):
        return None
    htext = b"".join(ln + b"\n" for ln in head)
    return header_bytes(htext, list(zip(names[:-1], lengths[:-1]))), recs


def bam_bytes(text):
    enc = sam_to_bam(text)
    return None if enc is None else enc[0] + b"".join(enc[1])


def bam_file(text, block=5000, eof=True):
    """The SAM text as a BAM file of BGZF blocks of `block` bytes; None for text that BAM cannot hold."""
    raw = bam_bytes(text)
    return None if raw is None else bgzf_compress(raw, block=block, eof=eof)


def record_of_line(text, line):
    """1-based number, among the alignment records, of the record on the 1-based file line `line`."""
    lines = R.read_lines(text)
    n = 0
    while n < len(lines) and lines[n].startswith(b"@"):
        n += 1
    return sum(1 for ln in lines[n:line] if ln != b"")


def _tags_text(b):
    """The tags of a record as SAM fields and the CG:B,I array if there is one."""
    out, cg, p = [], None, 0
    while p < len(b):
        tag, ty = b[p:p + 2].decode(), chr(b[p + 2])
        p += 3
        if ty == "A":
            out.append("%s:A:%s" % (tag, chr(b[p])))
            p += 1
        elif ty in "cCsSiI":
            size = _B_SIZE[ty]
            out.append("%s:i:%d" % (tag, struct.unpack_from("<" + _B_FMT[ty], b, p)[0]))
            p += size
        elif ty == "f":
            out.append("%s:f:%r" % (tag, struct.unpack_from("<f", b, p)[0]))
            p += 4
        elif ty in "ZH":
            q = b.index(b"\0", p)
            out.append("%s:%s:%s" % (tag, ty, b[p:q].decode()))
            p = q + 1
        elif ty == "B":
            sub, cnt = chr(b[p]), struct.unpack_from("<I", b, p + 1)[0]
            vals = struct.unpack_from("<%d%s" % (cnt, _B_FMT[sub]), b, p + 5)
            p += 5 + cnt * _B_SIZE[sub]
            if tag == "CG" and sub == "I" and cg is None:
                cg = vals
            else:
                out.append("%s:B:%s" % (tag, ",".join([sub] + [repr(v) for v in vals])))
        else:
            raise ValueError("unknown tag type %r" % ty)
    return out, cg


def bam_to_sam(raw):
    """Uncompressed BAM bytes as SAM text: the @SQ lines from the reference list, the other header lines of the text,
    one line per record."""
    assert raw[:4] == MAGIC
    l_text, = struct.unpack_from("<i", raw, 4)
    text = raw[8:8 + l_text]
    p = 8 + l_text
    n_ref, = struct.unpack_from("<i", raw, p)
    p += 4
    names, lines = [], []
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", raw, p)
        name = raw[p + 4:p + 4 + l_name - 1].decode()
        l_ref, = struct.unpack_from("<i", raw, p + 4 + l_name)
        p += 8 + l_name
        names.append(name)
        lines.append("@SQ\tSN:%s\tLN:%d" % (name, l_ref))
    lines += [ln.decode() for ln in text.split(b"\n") if ln and not ln.startswith(b"@SQ")]
    while p < len(raw):
        bs, = struct.unpack_from("<i", raw, p)
        r = raw[p + 4:p + 4 + bs]
        p += 4 + bs
        refid, pos, l_name, mapq, _, n_cig, flag, l_seq, nrefid, npos, tlen = struct.unpack_from("<iiBBHHHiiii", r, 0)
        q = 32
        qname = r[q:q + l_name - 1].decode()
        q += l_name
        ops = [(v >> 4, v & 15) for v in struct.unpack_from("<%dI" % n_cig, r, q)]
        q += 4 * n_cig
        seq = "".join(BASES[(r[q + i // 2] >> (0 if i & 1 else 4)) & 15] for i in range(l_seq))
        q += (l_seq + 1) // 2
        qual = r[q:q + l_seq]
        q += l_seq
        tags, cg = _tags_text(r[q:])
        if cg is not None and len(ops) == 2 and ops[0] == (l_seq, 4) and ops[1][1] == 3:
            ops = [(v >> 4, v & 15) for v in cg]
        ref = lambda i: "*" if i == -1 else names[i] if 0 <= i < n_ref else "?%d" % i      # noqa: E731
        f = [qname, str(flag), ref(refid), str(pos + 1), str(mapq), "".join("%d%s" % (a, OPS[b]) for a, b in ops) or "*",
             "*" if nrefid == -1 else "=" if nrefid == refid else ref(nrefid), str(npos + 1), str(tlen), seq or "*",
             "*" if not l_seq or qual == b"\xff" * l_seq else "".join(chr(c + 33) for c in qual)] + tags
        lines.append("\t".join(f))
    return ("\n".join(lines) + "\n").encode()


# ---- generator --------------------------------------------------------------------------------------------------------
REFS = ["chr%d" % i for i in range(1, 8)] + ["contig_with_a_long_name_%d" % i for i in range(3)]


def header(refs=REFS):
    h = ["@HD\tVN:1.6\tSO:unsorted"] + ["@SQ\tSN:%s\tLN:%d" % (r, 1000 * (i + 1)) for i, r in enumerate(refs)]
    h.insert(3, "@CO\tbetween the @SQ lines")
    h.append("@PG\tID:minimap2\tPN:minimap2\tVN:2.24")
    return "\n".join(h) + "\n"


def cigar(rng, nops):
    """Random CIGAR with nops middle ops over all nine letters (at least one that is not H/S), optional clips."""
    lens = rng.integers(1, 60, nops)
    letters = rng.choice(list("MMMMIDNP=X"), nops)
    letters[rng.integers(0, nops)] = rng.choice(list("MDN=X"))
    parts = ["%d%s" % (a, b) for a, b in zip(lens, letters)]
    lead, trail = [], []
    for side in (lead, trail):
        r = rng.random()
        if r < 0.25:
            side.append("%dH" % rng.integers(1, 500))
        if rng.random() < 0.5:
            side.append("%dS" % rng.integers(1, 500))
        if r > 0.9:
            side.append("%dH" % rng.integers(1, 9))   # H after S at the start / S before H at the end: only the first rule applies
    return "".join(lead + parts + trail[::-1])


def record(rng, i, refs=REFS, nops=None, mapped=False, seqlen=None):
    """One encodable SAM record.  Dropped records (FLAG & 4) may carry '*' CIGARs, clip-only CIGARs and a reference that
    is not in the header (an out-of-range refID in the BAM)."""
    flag = int(rng.choice([0, 4, 16, 256, 2048])) | int(rng.choice([0, 0, 4, 16, 256, 2048, 1, 2, 64, 128]))
    if mapped:
        flag &= ~4
    mapq = int(rng.integers(0, 256))
    if flag & 4:
        rname = str(rng.choice(refs + ["*", "not_in_header"]))
        cig = str(rng.choice(["*", "7S", "10M"]))
        pos = str(rng.choice(["0", "2147483648", "17"]))
    else:
        rname = str(rng.choice(refs + ["*"]))
        cig = cigar(rng, int(nops if nops is not None else rng.integers(1, 40)))
        pos = str(int(rng.integers(-5, 10 ** 6)))
    n = int(rng.integers(0, 12)) if seqlen is None else seqlen
    seq = "".join(rng.choice(list("ACGTN"), n)) if n else "*"
    qual = "".join(chr(int(c)) for c in rng.integers(33, 75, n)) if n and rng.random() < 0.8 else "*"
    f = ["read_%d_%s" % (i, "x" * int(rng.integers(0, 30))), str(flag), rname, pos, str(mapq), cig, "*", "0", "0", seq, qual]
    f += ["NM:i:%d" % rng.integers(0, 70000), "tp:A:P", "cs:Z:abc"][:int(rng.integers(0, 4))]
    return "\t".join(f)


def sam_text(rng, n, refs=REFS, **kw):
    return (header(refs) + "\n".join(record(rng, i, refs, **kw) for i in range(n)) + "\n").encode()
