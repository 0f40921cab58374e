"""Compressed input: BGZF (bgzip; SAM specification section 4.1) and plain gzip files of FASTQ or SAM text.

A BGZF file is a series of independent gzip members of at most 64 KB each.  The host only walks their headers
(sarlacc_bgzf_scan); the compressed bytes are uploaded and every block is inflated by one wavefront
(sarlacc_dev_bgzf_inflate, bgzf.hip) into a device text buffer that the FASTQ and SAM parsers read where it lies, so
the inflated text never visits the host.  Plain gzip (no BC subfield) cannot be split without inflating it: it is
streamed through zlib on the host into the text path, a slow path kept for correctness only.  Anything that does
not start with the gzip magic is text and takes the text path untouched.

Compressed output: deflate_device turns text in device memory into BGZF blocks there (sarlacc_dev_bgzf_deflate,
bgzf_deflate.hip), so that only compressed bytes come back; DeviceReads.to_fastq(compress=True) writes them and
EOF_BLOCK behind them.  DeviceReads.to_bam does the same with BAM records, whose fields it hands over as the pieces
that may get a Huffman table of their own (sarlacc_dev_bgzf_deflate_cuts)."""
import ctypes as C
import zlib

import numpy as np

from . import _lib
from ._lib import SarlaccError, check

TEXT, GZIP, BGZF = "text", "gzip", "bgzf"
# the empty block that ends a BGZF file (SAM specification section 4.1.2)
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def sniff_bytes(head):
    """TEXT, GZIP or BGZF from the first bytes of a file (the whole gzip header with its extra field should be there:
    a few hundred bytes do)."""
    if len(head) < 2 or head[0] != 0x1f or head[1] != 0x8b:
        return TEXT
    if len(head) < 12 or head[2] != 8 or not head[3] & 4:
        return GZIP
    xlen = head[10] | (head[11] << 8)
    f, end = 12, min(12 + xlen, len(head))
    while f + 4 <= end:
        slen = head[f + 2] | (head[f + 3] << 8)
        if head[f:f + 2] == b"BC" and slen == 2:
            return BGZF
        f += 4 + slen
    return GZIP


def sniff(path):
    with open(path, "rb") as fh:
        return sniff_bytes(fh.read(1 << 16))


def scan(buf, max_blocks=None, first_block=0):
    """sarlacc_bgzf_scan on host bytes: (number of complete blocks, bytes they occupy, compressed offsets, text
    offsets, whether the last one is the end-of-file block)."""
    a = np.frombuffer(buf, np.uint8) if not isinstance(buf, np.ndarray) else buf
    if max_blocks is None:
        max_blocks = a.size // 26 + 1          # no block is shorter than header + trailer
    comp_off, text_off = np.zeros(max_blocks + 1, np.int64), np.zeros(max_blocks + 1, np.int64)
    n, used, eof = C.c_int64(0), C.c_int64(0), C.c_int(0)
    check(_lib.lib().sarlacc_bgzf_scan(a if a.size else np.zeros(1, np.uint8), a.size, int(max_blocks), int(first_block),
                                       comp_off, text_off, C.byref(n), C.byref(used), C.byref(eof)))
    return n.value, used.value, comp_off[:n.value + 1], text_off[:n.value + 1], bool(eof.value)


class GzipReader:
    """read(n) over a plain gzip file of any number of concatenated members, inflated on the host with zlib -- the slow
    path: one thread, a few hundred MB/s.  read(n) returns exactly n bytes until the text ends, like a file."""

    def __init__(self, fh):
        self.fh, self.z, self.out, self.have, self.done = fh, zlib.decompressobj(31), [], 0, False

    def _more(self):
        raw = self.z.unused_data or self.fh.read(1 << 20)
        if self.z.eof:
            if not raw:
                self.done = True
                return
            self.z = zlib.decompressobj(31)
        elif not raw:
            raise SarlaccError("gzip file ends inside a member")
        piece = self.z.decompress(raw)
        self.out.append(piece)
        self.have += len(piece)

    def read(self, n=-1):
        while not self.done and (n < 0 or self.have < n):
            self._more()
        data = b"".join(self.out)
        if n < 0 or n >= len(data):
            self.out, self.have = [], 0
            return data
        self.out, self.have = [data[n:]], len(data) - n
        return data[:n]


def open_text(path):
    """A binary reader of the TEXT of a plain, gzip or BGZF file, on the host (generics.read_fastq)."""
    import gzip
    return open(path, "rb") if sniff(path) == TEXT else gzip.open(path, "rb")


class BgzfReader:
    """Whole BGZF blocks of an open file, taken until their inflated size reaches a target.  `first_block` numbers the
    first block at the file's position (error messages count blocks from the start of the file)."""

    def __init__(self, fh, first_block=0):
        self.fh, self.buf, self.block, self.file_eof = fh, b"", int(first_block), False

    def _read(self, nbytes):
        fresh = self.fh.read(max(int(nbytes), 1 << 16))
        if not fresh:
            self.file_eof = True
        else:
            self.buf = self.buf + fresh if self.buf else fresh

    def exhausted(self):
        if not self.buf and not self.file_eof:
            self._read(1 << 16)
        return self.file_eof and not self.buf

    def take(self, target):
        """(compressed bytes, compressed offsets, text offsets, number of the first block) of the next blocks, as few as
        hold `target` bytes of text (None: all that is left); None at the end of the file."""
        while True:
            n, used, comp_off, text_off, _ = scan(self.buf, first_block=self.block) if self.buf else (0, 0, None, None, False)
            enough = n > 0 and target is not None and text_off[n] >= target
            if not enough and not self.file_eof:
                # compressed FASTQ runs at a third to a quarter of its text
                self._read((1 << 30) if target is None else max(int(target) // 4, 1 << 16))
                continue
            if self.file_eof and used < len(self.buf) and not enough:
                raise SarlaccError("file ends inside BGZF block %d" % (self.block + n + 1))
            if n == 0:
                return None
            m = n if not enough else max(int(np.searchsorted(text_off, target, side="left")), 1)
            end = int(comp_off[m])
            comp, self.buf = self.buf[:end], self.buf[end:]
            first, self.block = self.block, self.block + m
            return comp, comp_off[:m + 1].copy(), text_off[:m + 1].copy(), first


def inflate_into(d_text, at, comp, comp_off, text_off, first_block, check_crc=True):
    """Uploads the blocks and inflates them into the device buffer `d_text` from byte `at` on."""
    from .resident import DevBuffer
    n = len(comp_off) - 1
    if n == 0:
        return
    d_comp = DevBuffer.from_numpy(np.frombuffer(comp, np.uint8))
    d_co, d_to = DevBuffer.from_numpy(comp_off), DevBuffer.from_numpy(text_off)
    check(_lib.lib().sarlacc_dev_bgzf_inflate(d_comp, d_co, d_to, n, int(first_block), d_text.ptr.value + int(at),
                                              1 if check_crc else 0, None))


def deflate_bound(nbytes):
    """sarlacc_bgzf_deflate_bound: (number of BGZF blocks, bytes the output buffer must hold) for `nbytes` of text."""
    n, cap = C.c_int64(0), C.c_int64(0)
    check(_lib.lib().sarlacc_bgzf_deflate_bound(int(nbytes), C.byref(n), C.byref(cap)))
    return n.value, cap.value


def deflate_device(d_text, nbytes, mode=0, out=None, cuts=None, cut_origin=0):
    """Device text -> BGZF blocks in device memory (sarlacc_dev_bgzf_deflate; no end-of-file block): (DevBuffer,
    compressed bytes).  mode 0 takes per block the smallest of one Huffman table, a table per line and stored; 1 leaves
    the per-line tables out, 2 stores.  `out` is a buffer to reuse, of at least deflate_bound(nbytes)[1] bytes.
    With `cuts` the pieces that get a table of their own end at the caller's boundaries, not behind newlines
    (sarlacc_dev_bgzf_deflate_cuts: bytes without lines, BAM records): sorted int64 offsets, either a host sequence,
    which is uploaded, or (device buffer or address, number of cuts); position cuts[j] - cut_origin of the text."""
    from .resident import DevBuffer
    cap = deflate_bound(nbytes)[1]
    d_comp = out if out is not None else DevBuffer(max(cap, 1))
    total = C.c_int64(0)
    if cuts is None:
        check(_lib.lib().sarlacc_dev_bgzf_deflate(d_text, int(nbytes), int(mode), d_comp, d_comp.nbytes, None, C.byref(total), None))
        return d_comp, total.value
    if isinstance(cuts, tuple):
        d_cuts, n_cuts = cuts
    else:
        host = np.ascontiguousarray(cuts, dtype=np.int64)
        d_cuts, n_cuts = (DevBuffer.from_numpy(host) if host.size else None), host.size
    check(_lib.lib().sarlacc_dev_bgzf_deflate_cuts(d_text, int(nbytes), d_cuts, int(n_cuts), int(cut_origin), int(mode), d_comp,
                                                   d_comp.nbytes, None, C.byref(total), None))
    return d_comp, total.value


class DeviceTextStream:
    """The text of a BGZF file as a sequence of device buffers of about `block_bytes`, each the unused tail of the one
    before (copied on the device, sarlacc_dev_copy) followed by freshly inflated whole blocks: every compressed block is
    inflated once.  `skip` bytes at the start of the first block taken are left out (a SAM header)."""

    def __init__(self, fh, block_bytes, first_block=0, skip=0, check_crc=True):
        self.reader, self.block_bytes, self.skip, self.check_crc = BgzfReader(fh, first_block), block_bytes, int(skip), check_crc

    def next(self, carry=None):
        """(device buffer, bytes of text in it, whether the file has ended).  `carry` = (buffer, offset, bytes) of the
        text to keep in front.  (None, 0, True) when nothing is left at all."""
        from .resident import DevBuffer
        nc = carry[2] if carry else 0
        got = self.reader.take(None if self.block_bytes is None else int(self.block_bytes) + self.skip)
        eof = self.reader.exhausted()
        if got is None:
            if not nc:
                return None, 0, True
            fresh = 0
        else:
            comp, comp_off, text_off, first = got
            fresh = int(text_off[-1])
        skip, self.skip = (0 if nc else min(self.skip, fresh)), 0      # only the first buffer skips, and it has no carry
        d_text = DevBuffer(max(nc + fresh, 1))
        if fresh:
            inflate_into(d_text, nc, comp, comp_off, text_off, first, self.check_crc)
        if nc:
            check(_lib.lib().sarlacc_dev_copy(d_text, carry[0].ptr.value + carry[1], nc, None))
        return _Slice(d_text, skip), nc + fresh - skip, eof


class _Slice:
    """A device buffer from an offset on, kept alive with its owner."""
    _as_parameter_ = property(lambda self: self.ptr)

    def __init__(self, owner, start):
        self.owner, self.ptr = owner, C.c_void_p(owner.ptr.value + int(start))


def rfind_newline(d_text, at, nbytes):
    """Position after the last newline of the `nbytes` of device text from byte `at` of d_text (0: none)."""
    pos = C.c_int64(-1)
    check(_lib.lib().sarlacc_dev_rfind_byte(d_text.ptr.value + int(at), int(nbytes), 10, C.byref(pos), None))
    return pos.value + 1


def host_blocks(fh):
    """Generator over (file offset, block number, inflated bytes) of the leading BGZF blocks, inflated on the host with
    zlib: for the SAM header only."""
    number, offset = 0, 0
    while True:
        head = fh.read(12)
        if not head:
            return
        if len(head) == 12:
            head += fh.read(head[10] | (head[11] << 8))
        bsize = _bsize(head, number)
        if bsize + 1 < len(head) + 8:
            raise SarlaccError("BGZF block %d: block size field is inconsistent" % (number + 1))
        rest = fh.read(bsize + 1 - len(head))
        if len(head) + len(rest) < bsize + 1:
            raise SarlaccError("file ends inside BGZF block %d" % (number + 1))
        block = head + rest
        scan(block, first_block=number)                      # the header checks, with the library's messages
        try:
            text = zlib.decompress(block[len(head):-8], -15)
        except zlib.error as e:
            raise SarlaccError("BGZF block %d: %s" % (number + 1, e))
        if len(text) != int.from_bytes(block[-4:], "little") or zlib.crc32(text) != int.from_bytes(block[-8:-4], "little"):
            raise SarlaccError("BGZF block %d: CRC32 mismatch" % (number + 1))
        yield offset, number, text
        offset += len(block)
        number += 1


def _bsize(head, number):
    if len(head) < 12 or len(head) < 12 + (head[10] | (head[11] << 8)):
        raise SarlaccError("file ends inside BGZF block %d" % (number + 1))
    f = 12
    while f + 4 <= len(head):
        slen = head[f + 2] | (head[f + 3] << 8)
        if head[f:f + 2] == b"BC" and slen == 2:
            return head[f + 4] | (head[f + 5] << 8)
        f += 4 + slen
    scan(head, first_block=number)       # raises the library's message for this header
    raise SarlaccError("BGZF block %d: no BC subfield" % (number + 1))
