"""sam2ranges (R/sam2ranges.R:8-95): SAM alignment records -> ranges.

The header is read here on the host, as the reference reads it line by line (:17-39); the body is read in blocks and
every block is parsed on the device (sam.hip: sarlacc_dev_sam_index / _extract), which replaces read.delim and the
regular expressions over every CIGAR (:49-74, .get_clip_length :80-95).  Where the port departs from the reference
("Known deviations"): the first alignment record is kept (the reference's `skip = N` drops it), the
seqinfo comes from the @SQ lines only whatever other header lines stand between them, and inputs on which the
reference would produce NA or fail further down are refused with the 1-based file line.

A BAM file takes the same road in its binary form: read_bam_header on the host, the records inflated on the device and
located and parsed there (bam.hip: sarlacc_dev_bam_index / _extract); refusals name the 1-based alignment record.
"""
import ctypes as C
import math
import numbers
import re

import numpy as np

from . import _lib
from ._lib import SarlaccError, check
from .strset import StringSet, StrList

# the `sub` patterns of :35-36; the greedy .* makes the LAST tag win
_SN = re.compile(rb".*\tSN:([^\t]+)(?:\t.*)?", re.S)
_LN = re.compile(rb".*\tLN:([^\t]+)(?:\t.*)?", re.S)
_INT = re.compile(rb"[+-]?[0-9]+")
INT_MAX = 2 ** 31 - 1


def _strip_eol(line):
    if line.endswith(b"\n"):
        line = line[:-1]
    if line.endswith(b"\r"):
        line = line[:-1]
    return line


def parse_header(lines):
    """Seqinfo of the header lines (bytes, without their line ends): the @SQ lines in order, then '*' with length 0
    (:35-37).  Returns (names, lengths)."""
    names, lengths, seen = [], [], set()
    for i, line in enumerate(lines):
        if not line.startswith(b"@SQ"):
            continue
        sn, ln = _SN.fullmatch(line), _LN.fullmatch(line)
        if sn is None:
            raise SarlaccError("SAM line %d: @SQ line without SN:" % (i + 1))
        if ln is None or not _INT.fullmatch(ln.group(1)) or not 0 <= int(ln.group(1)) <= INT_MAX:
            raise SarlaccError("SAM line %d: @SQ line without a non-negative integer LN:" % (i + 1))
        name = sn.group(1).decode()
        if name in seen or name == "*":
            raise SarlaccError("SAM line %d: duplicate @SQ name '%s'" % (i + 1, name))
        seen.add(name)
        names.append(name)
        lengths.append(int(ln.group(1)))
    return names + ["*"], np.array(lengths + [0], dtype=np.int64)


def read_header(fh):
    """Leading lines that start with '@' (:20-33) of a file opened in binary mode.  Returns (seqinfo names, lengths,
    number of header lines, whether the file ends inside the header); `fh` is left at the first body line."""
    lines = []
    while True:
        pos = fh.tell()
        line = fh.readline()
        if not line:
            return parse_header(lines) + (len(lines), True)
        if not line.startswith(b"@"):
            fh.seek(pos)
            return parse_header(lines) + (len(lines), False)
        lines.append(_strip_eol(line))


def check_args(minq, restricted):
    """The argument checks R would make of `minq` (a numeric scalar compared as MAPQ >= minq) and `restricted`
    (a character vector).  Returns (use_minq, integer threshold, restricted list or None)."""
    if minq is not None:
        if isinstance(minq, (bool, np.bool_)) or not isinstance(minq, numbers.Real):
            raise ValueError("'minq' should be NULL or a numeric scalar")
        minq = float(minq)
        if math.isnan(minq):
            raise ValueError("'minq' should not be NA")
    if restricted is not None:
        if isinstance(restricted, (str, bytes)):
            restricted = [restricted]
        restricted = list(restricted)
        if not all(isinstance(r, str) for r in restricted):
            raise ValueError("'restricted' should be NULL or a character vector")
    if minq is None:
        return False, 0, restricted
    # MAPQ is an integer: MAPQ >= minq  <=>  MAPQ >= ceil(minq)
    thr = -(2 ** 62) if minq == -math.inf else 2 ** 62 if minq == math.inf else max(-(2 ** 62), min(2 ** 62, math.ceil(minq)))
    return True, thr, restricted


def _empty(names, lengths):
    z = np.zeros(0, np.int32)
    return {"seqnames": z, "start": z.copy(), "end": z.copy(), "width": z.copy(), "strand": np.zeros(0, "<U1"),
            "left.clip": z.copy(), "right.clip": z.copy(), "names": StrList([]),
            "seqinfo": {"seqnames": list(names), "seqlengths": lengths}}


def _flat(strings):
    bs = [s.encode() for s in strings]
    off = np.zeros(len(bs) + 1, np.int64)
    if bs:
        np.cumsum([len(b) for b in bs], out=off[1:])
    return np.frombuffer(b"".join(bs) + b"\0", np.uint8).copy(), off


class _Tables:
    """The name table arguments of sarlacc_dev_sam_index, built once per call."""

    def __init__(self, names, restricted):
        self.ref, self.ref_off = _flat(names)
        self.n_ref = len(names)
        self.mask = None
        extra = []
        if restricted is not None:
            listed = set(restricted)
            self.mask = np.array([n in listed for n in names], np.uint8)
            known = set(names)
            extra = sorted(listed - known)
        self.extra, self.extra_off = _flat(extra)
        self.n_extra = len(extra)


def _parse_block(d_text, nbytes, first_line, tables, use_minq, thr):
    """One block of body text in HBM -> (number of lines, columns of the kept records)."""
    lib = _lib.lib()
    nlines, nk, nb = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    check(lib.sarlacc_dev_sam_index(d_text, nbytes, first_line, tables.ref, tables.ref_off, tables.n_ref, tables.mask,
                                    tables.extra, tables.extra_off, tables.n_extra, 1 if use_minq else 0, thr, C.byref(nlines),
                                    C.byref(nk), C.byref(nb), None))
    return nlines.value, _columns(lib.sarlacc_dev_sam_extract, d_text, nk.value, nb.value)


def _columns(extract, d_text, n, nbytes):
    """Step 2 of either pair (sarlacc_dev_sam_extract / sarlacc_dev_bam_extract): the columns of the `n` kept records."""
    from .resident import DevBuffer
    cols = DevBuffer(max(21 * n, 1))            # five int32 columns, then the strand bytes
    names, noff = DevBuffer(max(nbytes, 1)), DevBuffer(8 * (n + 1))
    base = cols.ptr.value
    check(extract(d_text, *[base + 4 * n * k for k in (0, 1, 2)], base + 20 * n,
                  *[base + 4 * n * k for k in (3, 4)], names, noff, None))
    host = cols.to_numpy(np.uint8, 21 * n)
    out = [host[4 * n * k:4 * n * (k + 1)].view(np.int32) for k in range(5)] + [host[20 * n:21 * n]]
    chars = names.to_numpy(np.uint8, nbytes)
    out.append(StringSet(chars if chars.size else np.zeros(1, np.uint8), noff.to_numpy(np.int64, n + 1)))
    return out


def blocks(fh, block_bytes):
    """The rest of an open binary file in blocks of about `block_bytes` that end at their last newline (the remainder
    is carried over); a block grows when one line is longer than it.  The last block may end without a newline."""
    block_bytes = int(block_bytes)
    if block_bytes < 1:
        raise ValueError("'block_bytes' must be a positive integer")
    carry = b""
    while True:
        fresh = fh.read(block_bytes)
        text = carry + fresh if carry else fresh
        if not fresh:
            if text:
                yield text
            return
        cut = text.rfind(b"\n") + 1
        if cut == 0:
            carry = text          # no line ends in this block yet: read more
            continue
        carry = text[cut:]
        yield text[:cut] if carry else text


def _text_parts(fh, block_bytes, restricted, use_minq, thr):
    """(seqinfo names, lengths, parsed blocks) of a file of SAM text opened in binary mode; no blocks: an empty result."""
    from .resident import DevBuffer
    names, lengths, nhead, ended = read_header(fh)
    if ended:
        return names, lengths, []          # :42-46, before any data is read
    first = fh.read(1 << 16)
    if len(first) < 1 << 16 and not first.lstrip(b"\r\n"):
        return names, lengths, []          # a body of blank lines only
    fh.seek(-len(first), 1)
    tables = _Tables(names, restricted)
    parts, line = [], nhead + 1
    for text in blocks(fh, block_bytes):
        d_text = DevBuffer.from_numpy(np.frombuffer(text, np.uint8))
        nlines, cols = _parse_block(d_text, len(text), line, tables, use_minq, thr)
        line += nlines
        parts.append(cols)
    return names, lengths, parts


def _bgzf_header(fh):
    """The header of a BGZF SAM file, inflated on the host with zlib, leading blocks only, up to the first body line:
    (header lines, (file offset, number) of the block that holds the first body byte and that byte's offset in the
    block's text -- None when the file ends inside the header)."""
    from . import bgzf
    lines, pending, origin = [], b"", None
    for offset, number, text in bgzf.host_blocks(fh):
        p = 0
        if not pending:
            origin = (offset, number, 0)
        while pending or p < len(text):
            if (pending[:1] or text[p:p + 1]) != b"@":
                return lines, origin
            nl = text.find(b"\n", p)
            if nl < 0:
                pending += text[p:]
                break
            lines.append(_strip_eol(pending + text[p:nl + 1]))
            pending, p = b"", nl + 1
            origin = (offset, number, p)
    if pending:
        lines.append(_strip_eol(pending))
    return lines, None


def _bgzf_parts(path, block_bytes, restricted, use_minq, thr):
    """_text_parts for a BGZF file: the body is inflated on the device from the block that holds its first byte; a parse
    block ends at the last newline of the device text (sarlacc_dev_rfind_byte) and the rest is carried over on the device."""
    from . import bgzf
    with open(path, "rb") as fh:
        lines, origin = _bgzf_header(fh)
        names, lengths = parse_header(lines)
        if origin is None:
            return names, lengths, []
        fh.seek(origin[0])
        stream = bgzf.DeviceTextStream(fh, block_bytes, first_block=origin[1], skip=origin[2])
        tables = _Tables(names, restricted)
        parts, line, carry, eof, first = [], len(lines) + 1, None, False, True
        while not eof:
            d_text, nbytes, eof = stream.next(carry)
            if d_text is None or nbytes == 0:
                break
            if first and eof and nbytes < 1 << 16:     # a body of blank lines only (a small file: the only host look at body text)
                from .resident import DevBuffer
                if not DevBuffer.borrow(d_text.ptr.value, nbytes).to_numpy(np.uint8, nbytes).tobytes().lstrip(b"\r\n"):
                    return names, lengths, []
            first = False
            cut = nbytes if eof else bgzf.rfind_newline(d_text, 0, nbytes)
            if cut:
                nlines, cols = _parse_block(d_text, cut, line, tables, use_minq, thr)
                line += nlines
                parts.append(cols)
            carry = (d_text, cut, nbytes - cut) if cut < nbytes else None    # (no line ends in this block yet: it grows)
    return names, lengths, parts


BAM_MAGIC = b"BAM\1"
UNALIGNED_HEADER = "@HD\tVN:1.6\tSO:unsorted\n"


def bam_header_bytes(text=None):
    """The header of an unaligned BAM file (SAM specification section 4.2): magic, l_text, the text as given (str or
    bytes; None: UNALIGNED_HEADER) and n_ref = 0.  A text with @SQ lines is refused: the file lists no reference, and
    the records DeviceReads.to_bam writes name none."""
    raw = UNALIGNED_HEADER if text is None else text
    raw = raw.encode() if isinstance(raw, str) else bytes(raw)
    if any(line.startswith(b"@SQ") for line in raw.split(b"\n")):
        raise SarlaccError("BAM header: @SQ lines in the header of an unaligned BAM file (its records name no reference)")
    return BAM_MAGIC + len(raw).to_bytes(4, "little") + raw + (0).to_bytes(4, "little")


def is_bam(path):
    """Whether the file is BGZF and its first four inflated bytes are the BAM magic."""
    from . import bgzf
    if bgzf.sniff(path) != bgzf.BGZF:
        return False
    head = b""
    try:
        with open(path, "rb") as fh:
            for _, _, text in bgzf.host_blocks(fh):
                head += text[:4 - len(head)]
                if len(head) == 4:
                    break
    except SarlaccError:
        return False        # a damaged first block: the BGZF text path reports it
    return head == BAM_MAGIC


class _HostBlocks:
    """read(n) over bgzf.host_blocks that knows where the next unread byte lies: (file offset, number) of its BGZF block
    and its offset in that block's inflated bytes."""

    def __init__(self, fh):
        from . import bgzf
        self.gen, self.offset, self.number, self.text, self.p = bgzf.host_blocks(fh), 0, 0, b"", 0

    def read(self, n, what):
        out = []
        while n > 0:
            if self.p == len(self.text):
                try:
                    self.offset, self.number, self.text = next(self.gen)
                except StopIteration:
                    raise SarlaccError("BAM header: file ends inside %s" % what) from None
                self.p = 0
                continue
            piece = self.text[self.p:self.p + n]
            out.append(piece)
            self.p += len(piece)
            n -= len(piece)
        return b"".join(out)

    def i32(self, what):
        return int.from_bytes(self.read(4, what), "little", signed=True)


def read_bam_header(fh):
    """The header of a BAM file opened in binary mode (SAM specification section 4.2), inflated on the host with zlib,
    leading blocks only: magic, l_text, text, n_ref, then per reference l_name (which counts the NUL), name, l_ref.
    Returns (seqinfo names + '*', lengths + 0, (file offset, number) of the BGZF block that holds the first byte after
    the header and that byte's offset in the block's inflated bytes).  The seqinfo is the binary reference list, not the
    @SQ lines of the text."""
    r = _HostBlocks(fh)
    if r.read(4, "the magic") != BAM_MAGIC:
        raise SarlaccError("BAM header: the file does not start with the BAM magic")
    l_text = r.i32("the header")
    if l_text < 0:
        raise SarlaccError("BAM header: negative text length")
    r.read(l_text, "the header text")
    n_ref = r.i32("the header")
    if n_ref < 0:
        raise SarlaccError("BAM header: negative number of references")
    names, lengths, seen = [], [], set()
    for k in range(n_ref):
        l_name = r.i32("reference %d" % (k + 1))
        if l_name < 0:
            raise SarlaccError("BAM header: reference %d: negative name length" % (k + 1))
        if l_name == 0:
            raise SarlaccError("BAM header: reference %d: empty name field" % (k + 1))
        raw = r.read(l_name, "reference %d" % (k + 1))
        if raw[-1:] != b"\0":
            raise SarlaccError("BAM header: reference %d: name without its NUL" % (k + 1))
        l_ref = r.i32("reference %d" % (k + 1))
        if l_ref < 0:
            raise SarlaccError("BAM header: reference %d: negative length" % (k + 1))
        name = raw[:-1].decode()
        if name in seen or name == "*":
            raise SarlaccError("BAM header: reference %d: duplicate name '%s'" % (k + 1, name))
        seen.add(name)
        names.append(name)
        lengths.append(l_ref)
    return names + ["*"], np.array(lengths + [0], dtype=np.int64), (r.offset, r.number, r.p)


def _bam_parts(path, block_bytes, restricted, use_minq, thr):
    """_bgzf_parts for a BAM file: the records are inflated on the device from the block that holds the first of them, a
    parse block ends at its last complete record (used_bytes of sarlacc_dev_bam_index) and the rest is carried over on
    the device; a buffer in which no record is complete grows."""
    from . import bgzf
    lib = _lib.lib()
    with open(path, "rb") as fh:
        names, lengths, origin = read_bam_header(fh)
        mask = None
        if restricted is not None:       # names that are not in the header never match
            listed = set(restricted)
            mask = np.array([n in listed for n in names], np.uint8)
        fh.seek(origin[0])
        stream = bgzf.DeviceTextStream(fh, block_bytes, first_block=origin[1], skip=origin[2])
        parts, record, carry, eof = [], 1, None, False
        while not eof:
            d_bam, nbytes, eof = stream.next(carry)
            if d_bam is None or nbytes == 0:
                break
            nrec, used, nk, nb = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)
            check(lib.sarlacc_dev_bam_index(d_bam, nbytes, record, 1 if eof else 0, len(names) - 1, mask, 1 if use_minq else 0,
                                            thr, C.byref(nrec), C.byref(used), C.byref(nk), C.byref(nb), None))
            if nrec.value:
                parts.append(_columns(lib.sarlacc_dev_bam_extract, d_bam, nk.value, nb.value))
                record += nrec.value
            carry = (d_bam, used.value, nbytes - used.value) if used.value < nbytes else None
    return names, lengths, parts


def sam2ranges(sam, minq=10, restricted=None, block_bytes=256 << 20):
    """sam2ranges (R/sam2ranges.R:8-95).  See generics.sam2ranges.  `sam` may be plain text, BGZF (the body is inflated on
    the device, bgzf.py), BAM (BGZF around binary records: located and parsed on the device, bam.hip) or plain gzip
    (inflated by Python's gzip module on the host: slow, for correctness only)."""
    from . import bgzf
    use_minq, thr, restricted = check_args(minq, restricted)
    if int(block_bytes) < 1:
        raise ValueError("'block_bytes' must be a positive integer")
    if is_bam(sam):
        names, lengths, parts = _bam_parts(sam, block_bytes, restricted, use_minq, thr)
    elif bgzf.sniff(sam) == bgzf.BGZF:
        names, lengths, parts = _bgzf_parts(sam, block_bytes, restricted, use_minq, thr)
    else:
        with bgzf.open_text(sam) as fh:
            names, lengths, parts = _text_parts(fh, block_bytes, restricted, use_minq, thr)
    if not parts:
        return _empty(names, lengths)
    ref, start, width, lclip, rclip, strand = (np.concatenate([p[k] for p in parts]) for k in range(6))
    qn = parts[0][6] if len(parts) == 1 else StringSet.concat([p[6] for p in parts])
    return {"seqnames": ref, "start": start, "end": (start.astype(np.int64) + width - 1).astype(np.int32), "width": width,
            "strand": strand.view("S1").astype("<U1"), "left.clip": lclip, "right.clip": rclip, "names": StrList(qn),
            "seqinfo": {"seqnames": list(names), "seqlengths": lengths}}
