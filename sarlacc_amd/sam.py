"""sam2ranges (R/sam2ranges.R:8-95): SAM alignment records -> ranges.

The header is read here on the host, as the reference reads it line by line (:17-39); the body is read in blocks and
every block is parsed on the device (sam.hip: sarlacc_dev_sam_index / _extract), which replaces read.delim and the
regular expressions over every CIGAR (:49-74, .get_clip_length :80-95).  Where the port departs from the reference
("Known deviations"): the first alignment record is kept (the reference's `skip = N` drops it), the
seqinfo comes from the @SQ lines only whatever other header lines stand between them, and inputs on which the
reference would produce NA or fail further down are refused with the 1-based file line.
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
    from .resident import DevBuffer
    lib = _lib.lib()
    nlines, nk, nb = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    check(lib.sarlacc_dev_sam_index(d_text, nbytes, first_line, tables.ref, tables.ref_off, tables.n_ref, tables.mask,
                                    tables.extra, tables.extra_off, tables.n_extra, 1 if use_minq else 0, thr, C.byref(nlines),
                                    C.byref(nk), C.byref(nb), None))
    n = nk.value
    cols = DevBuffer(max(21 * n, 1))            # five int32 columns, then the strand bytes
    names, noff = DevBuffer(max(nb.value, 1)), DevBuffer(8 * (n + 1))
    base = cols.ptr.value
    check(lib.sarlacc_dev_sam_extract(d_text, *[base + 4 * n * k for k in (0, 1, 2)], base + 20 * n,
                                      *[base + 4 * n * k for k in (3, 4)], names, noff, None))
    host = cols.to_numpy(np.uint8, 21 * n)
    out = [host[4 * n * k:4 * n * (k + 1)].view(np.int32) for k in range(5)] + [host[20 * n:21 * n]]
    chars = names.to_numpy(np.uint8, nb.value)
    out.append(StringSet(chars if chars.size else np.zeros(1, np.uint8), noff.to_numpy(np.int64, n + 1)))
    return nlines.value, out


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


def sam2ranges(sam, minq=10, restricted=None, block_bytes=256 << 20):
    """sam2ranges (R/sam2ranges.R:8-95).  See generics.sam2ranges.  `sam` may be plain text, BGZF (the body is inflated on
    the device, bgzf.py) or plain gzip (inflated by Python's gzip module on the host: slow, for correctness only)."""
    from . import bgzf
    use_minq, thr, restricted = check_args(minq, restricted)
    if int(block_bytes) < 1:
        raise ValueError("'block_bytes' must be a positive integer")
    if bgzf.sniff(sam) == bgzf.BGZF:
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
