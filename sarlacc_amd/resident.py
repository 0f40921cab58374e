"""Device-resident read batches (include/sarlacc_amd.h "resident batches"): reads are uploaded
once and stay in HBM while they are windowed, shuffled and aligned many times -- the access
pattern of tuneAlignment / getAdaptorThresholds (/root/reference/R/tuneAlignment.R,
R/getAdaptorThresholds.R).  No torch needed: allocation and copies go through the C ABI."""
import collections
import ctypes as C

import numpy as np

from . import _lib, device
from ._lib import check
from .encoding import phred_encoding
from .strset import StringSet


class DevBuffer:
    _as_parameter_ = property(lambda self: self.ptr)   # a buffer is passed to the library as it is

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)
        self.ptr = C.c_void_p()
        check(_lib.lib().sarlacc_dev_malloc(C.byref(self.ptr), self.nbytes))

    @classmethod
    def borrow(cls, address, nbytes):
        """A view of device memory somebody else owns (e.g. a torch tensor's data_ptr()): never freed here."""
        b = object.__new__(cls)
        b.nbytes = int(nbytes)
        b.ptr = C.c_void_p(int(address))
        b.owned = False
        return b

    @classmethod
    def from_numpy(cls, a):
        a = np.ascontiguousarray(a)
        b = cls(a.nbytes)
        check(_lib.lib().sarlacc_dev_upload(b, a, a.nbytes))
        return b

    def to_numpy(self, dtype, count):
        out = _lib.host_array(max(count, 1), dtype)
        check(_lib.lib().sarlacc_dev_download(out, self, int(count) * out.itemsize))
        return out[:count]

    def __del__(self):
        try:
            if self.ptr and getattr(self, "owned", True):
                _lib.lib().sarlacc_dev_free(self.ptr)
                self.ptr = C.c_void_p()
        except Exception:
            pass


def _record_ranges(ro, block_bytes):
    """The record ranges [(first, last)] a writer formats at a time, from the n + 1 record offsets `ro`: the largest run
    of whole records whose bytes fit in `block_bytes` (None: everything), a single record larger than that in a range of
    its own size."""
    n = len(ro) - 1
    ranges, first = [], 0
    while first < n:
        last = n if block_bytes is None else max(int(np.searchsorted(ro, ro[first] + int(block_bytes), side="right")) - 1, first + 1)
        ranges.append((first, last))
        first = last
    return ranges


# What a writer needs to format any record range of a batch (DeviceReads._write_plan): the library's range formatter,
# the device buffers of names, name offsets, n + 1 record offsets and (BAM) cuts, the host copy `ro` of the record
# offsets and the record ranges [(first, last)] of the blocks; `per` cuts per record, and the batch's tags where the
# records carry them (then `format` is the library's formatter with tags).
WritePlan = collections.namedtuple("WritePlan", "format names noff rec_off cuts ro ranges per tags", defaults=(2, None))


class DeviceReads:
    """seq / qual / offsets in HBM + the host copy of the offsets.  `.tags` (a tags.DeviceTags, None by default) holds
    the reads' BAM tags where from_bam / stream_bam kept them or set_tag made them."""

    def __init__(self, seq, qual, off_dev, off_host, encoding):
        self.seq, self.qual, self.off, self.off_host, self.encoding = seq, qual, off_dev, off_host, encoding
        self.names = None
        self.tags = None

    @classmethod
    def upload(cls, reads):
        """reads: generics.Reads"""
        s, q = reads.seq, reads.qual
        if (s.widths() != q.widths()).any():
            raise _lib.SarlaccError("sequence and quality strings should have the same length")
        return cls(DevBuffer.from_numpy(s.chars), DevBuffer.from_numpy(q.chars), DevBuffer.from_numpy(s.off), s.off.copy(),
                   reads.encoding)

    @classmethod
    def from_fastq(cls, source, encoding=None):
        """FASTQ text (path, bytes or uint8 array) -> resident batch, parsed on the device
        (sarlacc_dev_fastq_index / _extract; replaces FastqStreamer + .FASTQ2QSDS,
        R/adaptorAlign.R:26-37,:104-110).  Read names are kept on the host in `.names`.  A path may name a plain, gzip or
        BGZF file (bgzf.sniff): BGZF is inflated on the device, plain gzip by zlib on the host (slow, for correctness only)."""
        if isinstance(source, (bytes, bytearray)):
            text = np.frombuffer(bytes(source), dtype=np.uint8)
        elif isinstance(source, np.ndarray):
            text = np.ascontiguousarray(source, dtype=np.uint8)
        else:
            from . import bgzf
            kind = bgzf.sniff(source)
            if kind == bgzf.BGZF:    # inflated on the device: the text never visits the host
                with open(source, "rb") as fh:
                    d_text, nbytes, _ = bgzf.DeviceTextStream(fh, None).next()
                return cls._from_device_text(d_text if d_text is not None else DevBuffer(1), nbytes, encoding)
            if kind == bgzf.GZIP:    # the slow path: one zlib thread on the host
                with open(source, "rb") as fh:
                    text = np.frombuffer(bgzf.GzipReader(fh).read(), dtype=np.uint8)
            else:
                text = np.fromfile(source, dtype=np.uint8)
        d_text = DevBuffer.from_numpy(text if text.size else np.zeros(1, np.uint8))
        return cls._from_device_text(d_text, text.size, encoding)

    @classmethod
    def _from_device_text(cls, text_ptr, nbytes, encoding):
        nrec, tb, tn = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        check(_lib.lib().sarlacc_dev_fastq_index(text_ptr, int(nbytes), C.byref(nrec), C.byref(tb), C.byref(tn), None))
        return cls._extracted(nrec.value, tb.value, tn.value, encoding,
                              lambda *bufs: check(_lib.lib().sarlacc_dev_fastq_extract(text_ptr, *bufs, None)))

    @classmethod
    def _extracted(cls, n, bases, name_bytes, encoding, extract):
        """A resident batch of n reads with `bases` bases and `name_bytes` bytes of names, once
        extract(seq, qual, off, names, name_off) has filled its device buffers; `.names` is a StrList over the names."""
        seq, qual = DevBuffer(max(bases, 1)), DevBuffer(max(bases, 1))
        off, names, noff = DevBuffer(8 * (n + 1)), DevBuffer(max(name_bytes, 1)), DevBuffer(8 * (n + 1))
        extract(seq, qual, off, names, noff)
        out = cls(seq, qual, off, off.to_numpy(np.int64, n + 1), encoding)
        from .strset import StrList
        nraw = names.to_numpy(np.uint8, name_bytes)
        out.names = StrList(StringSet(nraw if nraw.size else np.zeros(1, np.uint8), noff.to_numpy(np.int64, n + 1)))   # decoded on demand
        return out

    @classmethod
    def _text_chunks(cls, address, nbytes, number, eof, encoding):
        """Generator over the chunks of at most `number` records in the nbytes of FASTQ text at the device address:
        where the text ends inside a chunk and more follows (not eof) the chunk is left for the next buffer.  Returns
        the bytes used."""
        pos = 0
        while pos < nbytes:
            nrec, used = C.c_int64(0), C.c_int64(0)
            here = address + pos
            check(_lib.lib().sarlacc_dev_fastq_split(here, nbytes - pos, number, C.byref(nrec), C.byref(used), None))
            if nrec.value < number and not eof:
                break                           # the chunk continues in the next buffer
            if nrec.value < number:
                used.value = nbytes - pos       # last chunk: may end without a newline, or in blank lines
            chunk = cls._from_device_text(here, used.value, encoding)
            pos += used.value
            if len(chunk):
                yield chunk
        return pos

    @classmethod
    def stream_fastq(cls, path, number, encoding=None, block_bytes=256 << 20):
        """Generator over the file in chunks of at most `number` records, each a resident batch: the
        FastqStreamer(filepath, n=number) + yield() loop of R/adaptorAlign.R:26-37.  The file is read in
        blocks of `block_bytes`; where a block ends inside a record the device reports the end of the
        last complete one (sarlacc_dev_fastq_split) and the rest is carried over to the next block, so
        neither the host nor the device ever holds more than one block plus one chunk.  A BGZF file is inflated on the
        device, whole BGZF blocks worth `block_bytes` of text at a time, and the carry-over stays there (_stream_bgzf); a
        plain gzip file is inflated by zlib on the host into the text route (slow, for correctness only).  The chunks
        and the error messages are those of the text."""
        number = int(number)
        if number < 1:
            raise ValueError("'number' must be a positive integer")
        from . import bgzf
        kind = bgzf.sniff(path)
        carry = np.zeros(0, np.uint8)
        with open(path, "rb") as fh:
            if kind == bgzf.BGZF:
                yield from cls._stream_bgzf(fh, number, encoding, block_bytes)
                return
            if kind == bgzf.GZIP:
                fh = bgzf.GzipReader(fh)     # the slow path: inflated by zlib on the host, then as text
            eof = False
            while not eof:
                fresh = np.frombuffer(fh.read(int(block_bytes)), dtype=np.uint8)
                eof = fresh.size < int(block_bytes)
                text = np.concatenate([carry, fresh]) if carry.size else fresh
                if text.size == 0:
                    break
                d_text = DevBuffer.from_numpy(text)
                pos = yield from cls._text_chunks(d_text.ptr.value, text.size, number, eof, encoding)
                carry = text[pos:].copy()

    @classmethod
    def _stream_bgzf(cls, fh, number, encoding, block_bytes):
        """stream_fastq over a BGZF file: whole blocks worth about `block_bytes` of text are inflated on the device behind
        the unused tail of the buffer before, which is copied on the device; the chunks are those of the text route."""
        from . import bgzf
        stream, carry, eof = bgzf.DeviceTextStream(fh, block_bytes), None, False
        while not eof:
            d_text, nbytes, eof = stream.next(carry)
            if d_text is None or nbytes == 0:
                break
            pos = yield from cls._text_chunks(d_text.ptr.value, nbytes, number, eof, encoding)
            carry = (d_text, pos, nbytes - pos) if pos < nbytes else None

    @classmethod
    def stream_reads(cls, path, number, encoding=None, block_bytes=256 << 20, keep_tags=False):
        """stream_bam for a BAM file (sam.is_bam), stream_fastq for anything else: the read source of adaptorAlign and
        realizeReads.  A BAM file stores Phred values, so `encoding` plays no part there; `keep_tags` plays no part in
        a FASTQ file."""
        from . import sam
        if sam.is_bam(path):
            return cls.stream_bam(path, number, block_bytes=block_bytes, keep_tags=keep_tags)
        return cls.stream_fastq(path, number, encoding=encoding, block_bytes=block_bytes)

    @classmethod
    def from_bam(cls, path, exclude_flags=0x900, missing_qual=1, keep_tags=False):
        """The reads of a BAM file (aligned or not: a basecaller's unaligned BAM holds unmapped records only) as one
        resident batch, unpacked on the device (sarlacc_dev_bam_reads_index / _range / _extract, bam_reads.hip).  A record
        becomes a read unless `flag & exclude_flags` (the default drops secondary and supplementary records); a record
        stored reverse-complemented (flag 0x10) is turned back to the read as sequenced; a record without qualities gets
        `missing_qual` (0..93) at every base.  The encoding is Phred+33; `.names` is a StrList, as from_fastq leaves it.
        With `keep_tags` the batch gets `.tags`: every read's aux bytes as they lie in its record (tags.DeviceTags;
        sarlacc_dev_bam_reads_aux_range / _aux_extract), walked once on the device, so that a file with malformed tags
        fails here ("read K: malformed tags", K counted in the batch).  The tags of a record stored reverse-complemented
        are kept unchanged: its MM / ML / mv describe the stored strand.  Without `keep_tags` tags are skipped."""
        chunks = list(cls.stream_bam(path, None, exclude_flags, missing_qual, block_bytes=None, keep_tags=keep_tags))
        return chunks[0] if chunks else cls._bam_range(DevBuffer(1), 0, 0, missing_qual, keep_tags=keep_tags)

    @classmethod
    def stream_bam(cls, path, number, exclude_flags=0x900, missing_qual=1, block_bytes=256 << 20, keep_tags=False):
        """Generator over the reads of a BAM file (see from_bam) in chunks of `number` reads, each a resident batch: every
        chunk but the last holds exactly `number`, wherever the buffers end.  The header is read on the host
        (sam.read_bam_header); the records are inflated on the device, whole BGZF blocks worth `block_bytes` at a time
        (bgzf.DeviceTextStream).  A chunk that continues past the buffer carries the bytes from its first unused record
        on, on the device, into the next buffer; a buffer in which no record is complete grows.  With `keep_tags` every
        chunk carries `.tags`, read for read (see from_bam)."""
        from . import bgzf, sam
        if number is not None:      # (None: the whole file, from_bam)
            number = int(number)
            if number < 1:
                raise ValueError("'number' must be a positive integer")
        if isinstance(missing_qual, bool) or int(missing_qual) != missing_qual or not 0 <= missing_qual <= 93:
            raise ValueError("'missing_qual' must be an integer in 0..93")
        if isinstance(exclude_flags, bool) or int(exclude_flags) != exclude_flags or not 0 <= exclude_flags <= 0xffff:
            raise ValueError("'exclude_flags' must be an integer in 0..65535")
        if block_bytes is not None and int(block_bytes) < 1:
            raise ValueError("'block_bytes' must be a positive integer")
        lib = _lib.lib()
        with open(path, "rb") as fh:
            origin = sam.read_bam_header(fh)[2]
            fh.seek(origin[0])
            stream = bgzf.DeviceTextStream(fh, block_bytes, first_block=origin[1], skip=origin[2])
            record, carry, eof = 1, None, False
            while not eof:
                d_bam, nbytes, eof = stream.next(carry)
                if d_bam is None or nbytes == 0:
                    break
                nrec, used, nreads = C.c_int64(0), C.c_int64(0), C.c_int64(0)
                check(lib.sarlacc_dev_bam_reads_index(d_bam, nbytes, record, 1 if eof else 0, int(exclude_flags), C.byref(nrec),
                                                      C.byref(used), C.byref(nreads), None))
                pos, start = 0, 0
                while pos < nreads.value and (eof or number is None or nreads.value - pos >= number):
                    count = nreads.value - pos if number is None else min(number, nreads.value - pos)
                    chunk, start = cls._bam_range(d_bam, pos, count, int(missing_qual), with_next=True, keep_tags=keep_tags)
                    pos += count
                    yield chunk
                if pos == nreads.value:     # the dropped records at the end go too
                    start, taken = used.value, nrec.value
                else:                       # the chunk continues in the next buffer, from its first unused record on
                    done = C.c_int64(0)
                    check(lib.sarlacc_dev_bam_reads_records(pos, C.byref(done)))
                    taken = done.value
                record += taken
                carry = (d_bam, start, nbytes - start) if start < nbytes else None

    @classmethod
    def _bam_range(cls, d_bam, first, count, missing_qual, with_next=False, keep_tags=False):
        """The reads first .. first + count of the BAM buffer indexed last (sarlacc_dev_bam_reads_range / _extract) as a
        resident batch, with `keep_tags` with their validated tags, and with `with_next` the offset of the record behind
        them."""
        lib = _lib.lib()
        tb, tn, nxt = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        if count:
            check(lib.sarlacc_dev_bam_reads_range(first, count, C.byref(tb), C.byref(tn), C.byref(nxt)))

        def extract(seq, qual, off, names, noff):
            if count:
                check(lib.sarlacc_dev_bam_reads_extract(d_bam, first, count, missing_qual, seq, qual, off, names, noff, None))
            else:       # no reads: offsets that start at 0
                for buf in (off, noff):
                    check(lib.sarlacc_dev_upload(buf, np.zeros(1, np.int64), 8))
        out = cls._extracted(count, tb.value, tn.value, phred_encoding(), extract)
        if keep_tags:
            from .tags import DeviceTags
            if count:
                ab = C.c_int64(0)
                check(lib.sarlacc_dev_bam_reads_aux_range(first, count, C.byref(ab)))
                aux, aoff = DevBuffer(max(ab.value, 1)), DevBuffer(8 * (count + 1))
                check(lib.sarlacc_dev_bam_reads_aux_extract(d_bam, first, count, aux, aoff, None))
                out.tags = DeviceTags(aux, aoff, aoff.to_numpy(np.int64, count + 1).copy()).validate()
            else:
                out.tags = DeviceTags.empty(0)
        return (out, nxt.value) if with_next else out

    def __len__(self):
        return len(self.off_host) - 1

    def _encoding(self):
        return self.encoding if self.encoding is not None else phred_encoding()

    @property
    def total(self):
        return int(self.off_host[-1])

    @property
    def max_len(self):
        return int(np.diff(self.off_host).max()) if len(self) else 0

    def download(self):
        return (StringSet(self.seq.to_numpy(np.uint8, self.total), self.off_host.copy()),
                StringSet(self.qual.to_numpy(np.uint8, self.total), self.off_host.copy()))

    def _name_set(self):
        """`.names` as a StringSet (None: default names): a StrList hands over its flat bytes and offsets undecoded,
        a plain list of str is encoded once."""
        if self.names is None or len(self.names) == 0:   # (an empty list: default names, as in generics.write_fastq)
            return None
        from .strset import StrList
        ss = self.names.ss if isinstance(self.names, StrList) else StringSet.from_strings(list(self.names))
        if len(ss) != len(self):
            raise _lib.SarlaccError("%d read names for %d reads" % (len(ss), len(self)))
        return ss

    def _write_plan(self, block_bytes, bam=False):
        """The size pass of the device FASTQ writer (sarlacc_dev_fastq_format_size; refuses names with a line break) or,
        with `bam`, of the device BAM writer (sarlacc_dev_bam_format_size; refuses what BAM cannot hold, and leaves the
        SEQ and QUAL starts as `cuts`), and the record ranges of _record_ranges over the n + 1 record offsets `ro`.  The
        host knows every length of a FASTQ record and computes `ro` itself; the kept part of a BAM name is decided on
        the device, so there `ro` is downloaded.  Names, name offsets, record offsets and cuts stay on the device."""
        n = len(self)
        ss = self._name_set()
        names = noff = cuts = None
        if ss is not None:      # (names that are all empty: the library tells "no names" by a null pointer)
            names, noff = DevBuffer.from_numpy(ss.chars if ss.chars.size else np.zeros(1, np.uint8)), DevBuffer.from_numpy(ss.off)
        rec_off, total = DevBuffer(8 * (n + 1)), C.c_int64(0)
        if bam and self.tags is not None:
            tags = self._tags()
            cuts = DevBuffer(max(24 * n, 8))
            check(_lib.lib().sarlacc_dev_bam_format_size_aux(self.seq, self.qual, self.off, n, names, noff, 1, tags.aux, tags.off,
                                                             rec_off, cuts, C.byref(total), None))
            ro = rec_off.to_numpy(np.int64, n + 1)
            return WritePlan(_lib.lib().sarlacc_dev_bam_format_aux, names, noff, rec_off, cuts, ro, _record_ranges(ro, block_bytes),
                             3, tags)
        if bam:
            cuts = DevBuffer(max(16 * n, 8))
            check(_lib.lib().sarlacc_dev_bam_format_size(self.seq, self.qual, self.off, n, names, noff, 1, rec_off, cuts,
                                                         C.byref(total), None))
            ro = rec_off.to_numpy(np.int64, n + 1)
        else:
            check(_lib.lib().sarlacc_dev_fastq_format_size(self.off, n, names, noff, 1, rec_off, C.byref(total), None))
            if ss is not None:
                name_len = np.diff(ss.off)
            else:   # READ_<k>, k = 1 .. n
                name_len = 6 + np.searchsorted(10 ** np.arange(1, 19, dtype=np.int64), np.arange(1, n + 1, dtype=np.int64), side="right")
            ro = np.zeros(n + 1, np.int64)
            np.cumsum(name_len + 2 * np.diff(self.off_host) + 6, out=ro[1:])
        format_range = _lib.lib().sarlacc_dev_bam_format if bam else _lib.lib().sarlacc_dev_fastq_format
        return WritePlan(format_range, names, noff, rec_off, cuts, ro, _record_ranges(ro, block_bytes))

    def _blocks(self, plan, compress=False, head=None):
        """Generator over the blocks of a WritePlan: `head` (bytes that go in front as a block of their own), then every
        record range, formatted on the device (plan.format).  With `compress` a block is deflated where it lies into
        BGZF blocks (bgzf.deflate_device, with the plan's cuts as piece boundaries where it has them) and only the
        compressed bytes are downloaded.  Each block is a uint8 view of ONE reused page-locked buffer, valid until the
        next block is asked for."""
        from . import bgzf
        sizes = [int(plan.ro[b] - plan.ro[a]) for a, b in plan.ranges]
        largest = max(sizes + [0 if head is None else head.size])
        if not largest:
            return
        cap = bgzf.deflate_bound(largest)[1] if compress else largest
        d_raw, host = DevBuffer(largest), _lib.host_array(cap, np.uint8)
        d_out = DevBuffer(cap) if compress else d_raw

        def block(nbytes, **cuts):
            if compress:
                nbytes = bgzf.deflate_device(d_raw, nbytes, out=d_out, **cuts)[1]
            check(_lib.lib().sarlacc_dev_download(host, d_out, nbytes))
            return host[:nbytes]
        if head is not None:
            check(_lib.lib().sarlacc_dev_upload(d_raw, head, head.size))
            yield block(head.size)
        for (a, b), nbytes in zip(plan.ranges, sizes):
            aux = () if plan.tags is None else (plan.tags.aux, plan.tags.off)
            check(plan.format(self.seq, self.qual, self.off, plan.names, plan.noff, 1, *aux, plan.rec_off, a, b - a, d_raw, None))
            if plan.cuts is None:
                yield block(nbytes)
            else:
                yield block(nbytes, cuts=(plan.cuts.ptr.value + 8 * plan.per * a, plan.per * (b - a)), cut_origin=int(plan.ro[a]))

    def fastq_text(self, block_bytes=None):
        """The batch as 4-line FASTQ text (bytes), formatted on the device: record i is
        b"@" + name + b"\\n" + seq + b"\\n+\\n" + qual + b"\\n" -- LF only, the bytes generics.write_fastq writes for
        the same reads.  `.names` gives the names (the StrList from_fastq leaves, or a list of str); None selects READ_1,
        READ_2, ...  Sequence and quality bytes are copied as they are: `encoding` plays no part.  A name that holds a
        line break is refused ("record K: read name holds a line break").  `block_bytes` bounds the text the device
        formats at a time (see to_fastq); the result is the same.  The whole text is held on the host more than once (the
        download buffer, a copy per block, the joined result) and, with block_bytes=None, once on the device: this is for
        batches whose text fits comfortably; to_fastq is the bounded route.  Not done here: gzip output, multi-line FASTQ, a
        repeated name on the '+' line."""
        return b"".join(blk.tobytes() for blk in self._blocks(self._write_plan(block_bytes)))

    def to_fastq(self, path, append=False, block_bytes=256 << 20, compress=False):
        """Writes fastq_text() to `path` (after what is there with append=True) and returns the bytes written.  The
        text is formatted on the device in blocks of whole records of at most `block_bytes` (a single larger record
        gets a block of its own size), each downloaded into one page-locked buffer and written with one write(), so
        neither the host nor the device ever holds more than one block of text -- the bound of stream_fastq.  The file
        is opened only once the names have passed the check: a refused batch leaves it as it was.
        With compress=True the file is BGZF (what bgzip writes; from_fastq and any gzip reader take it): every block of
        text is deflated on the device where it was formatted (sarlacc_dev_bgzf_deflate: Huffman codes, a table per line
        where that is smaller), only the compressed bytes come to the host, and the 28-byte end-of-file block follows the
        last of them -- alone for an empty batch.  The count returned is that of the file's new bytes.  append=True leaves
        the end-of-file block of what was there in the middle, an empty member that BGZF permits.  Compression is never
        inferred from the name of the file."""
        from .bgzf import EOF_BLOCK
        return self._write_blocks(path, "ab" if append else "wb", self._blocks(self._write_plan(block_bytes), compress),
                                  EOF_BLOCK if compress else b"")

    @staticmethod
    def _write_blocks(path, mode, blocks, end):
        """Opens the file, writes the blocks with one write() each and `end` behind them; the bytes written."""
        written = len(end)
        with open(path, mode) as fh:
            for blk in blocks:
                fh.write(blk)
                written += blk.size
            fh.write(end)
        return written

    def to_bam(self, path, header=None, block_bytes=256 << 20):
        """Writes the batch to `path` as unaligned BAM (uBAM: what basecallers write and every long-read mapper and
        samtools take; from_bam reads it back) and returns the bytes written.  Record i is an unmapped, unpaired record
        (flag 4, no reference, no CIGAR) of read i, with the read's tags behind QUAL where the batch has `.tags` (kept by
        from_bam(keep_tags=True), made by set_tag) and without tags otherwise: SEQ packed and QUAL turned into Phred values on the device
        (sarlacc_dev_bam_format).  Its name is the read's name up to the first space or tab, as samtools import keeps it
        ('*' where nothing is left; READ_1, READ_2, ... without `.names`).  The records are formatted in ranges of whole
        records of at most `block_bytes`, as to_fastq plans its blocks; every range is deflated where it lies into BGZF
        blocks of its own (bgzf.deflate_device with the SEQ and QUAL starts as piece boundaries, so packed bases and
        qualities get a Huffman table each where that is smaller), only the compressed bytes are downloaded, into one
        reused page-locked buffer, and written with one write().  Records may straddle the BGZF blocks of a range.
        `header` is the header text (default sam.UNALIGNED_HEADER), written as given into BGZF blocks of its own in
        front of the records; one with @SQ lines is refused.  The 28-byte end-of-file block ends the file; an empty batch
        is header + end-of-file block.  There is no append: a BAM file has one header.
        Refused before the file is opened, so that it keeps what it held: an encoding other than Phred+33 (BAM stores
        Phred values), and "record K: <reason>" for the lowest record BAM cannot hold -- a kept name above 254 bytes or
        with a byte outside '!'..'~', a base that is not one of ACMGRSVTWYHKDBN, a quality byte outside 33..126, malformed
        tags, a tag that appears twice in one read.  With tags, the tag start of every record is a third piece boundary
        of the deflate.
        Not done here: @RG lines for the RG tags written (the header text is the caller's), aligned records, @SQ headers,
        paired flags, indexes."""
        from . import bgzf, sam
        from .encoding import encoding_name
        if block_bytes is not None and int(block_bytes) < 1:
            raise ValueError("'block_bytes' must be a positive integer")
        kind = encoding_name(self._encoding())
        if kind != "phred":
            raise _lib.SarlaccError("BAM stores Phred values: the batch's quality encoding is %s, not Phred+33" % kind)
        head = np.frombuffer(sam.bam_header_bytes(header), np.uint8)
        plan = self._write_plan(block_bytes, bam=True)
        return self._write_blocks(path, "wb", self._blocks(plan, compress=True, head=head), bgzf.EOF_BLOCK)

    def _tags(self):
        """`.tags`, checked against the batch."""
        if len(self.tags) != len(self):
            raise _lib.SarlaccError("tags of %d reads for %d reads" % (len(self.tags), len(self)))
        return self.tags

    def tag(self, name):
        """The values of the tag `name` ([A-Za-z][A-Za-z0-9]) and a boolean mask of the reads that hold it, found on the
        device (sarlacc_dev_bam_tags_find; the first entry of a repeated tag, as htslib's bam_aux_get).  Types A, Z and
        H give a StrList (an empty string where the tag is absent), the integer types c C s S i I -- mixed widths
        across the reads are fine -- an int64 array (0 where absent).  Strings and integers under one name are an
        error ("read K: tag XX has type T"), and so are the types f and B, which are not decoded: they are kept and
        written as they lie.  On a batch without tags, or where no read holds the tag, every read is absent and the
        values are empty strings."""
        from .tags import DeviceTags, tag_name
        name = tag_name(name)
        return (self._tags() if self.tags is not None else DeviceTags.empty(len(self))).values(name)

    def set_tag(self, name, values, present=None):
        """Sets the tag `name` on the reads where `present` (a boolean mask; None: on every read): replaced where a read
        holds it, appended behind the read's other tags where not -- one find and one splice on the device
        (sarlacc_dev_bam_tags_splice).  `values` (one per read, those outside `present` are ignored) are a StringSet, a
        StrList or a list of str, written as type Z -- a byte outside ' '..'~' is refused --, or integers within int32,
        written as type i.  A batch without `.tags` gets them."""
        from .tags import DeviceTags, present_mask, tag_column, tag_name
        name, column, mask = tag_name(name), tag_column(values, len(self)), present_mask(present, len(self))
        tags = self._tags() if self.tags is not None else DeviceTags.empty(len(self))
        self.tags = tags.set(name, column, mask)

    def drop_tags(self, names):
        """Removes every entry of the tags `names` (one name or several) from every read: what MM, ML and mv need
        after a trim or a reversal, which nothing here rewrites."""
        from .tags import tag_name
        names = [tag_name(nm) for nm in ([names] if isinstance(names, (str, bytes)) else names)]
        if self.tags is not None:
            tags = self._tags()
            for nm in names:
                tags = tags.drop(nm)
            self.tags = tags

    def _like(self, off_host):
        total = int(off_host[-1])
        return DeviceReads(DevBuffer(total), DevBuffer(total), DevBuffer.from_numpy(off_host), off_host, self.encoding)

    def front_and_back(self, tolerance):
        """.get_front_and_back (R/adaptorAlign.R:86-95) on the device.  The two window batches carry no tags."""
        if int(tolerance) < 0:
            raise _lib.SarlaccError("'tolerance' must not be negative")
        w = np.minimum(int(tolerance), np.diff(self.off_host))
        woff = np.zeros(len(self) + 1, np.int64)
        np.cumsum(w, out=woff[1:])
        out = []
        for which in (0, 1):
            d = self._like(woff.copy())
            check(_lib.lib().sarlacc_dev_windows(self.seq, self.qual, self.off, len(self), d.off, which, d.seq, d.qual, None))
            out.append(d)
        return out[0], out[1]

    def subseq(self, start, width, other=None, from_other=None):
        """XVector::subseq on the resident batch, straight to a host StringSet: element r = `width[r]` bases from the 1-based
        position `start[r]` of read r -- of `other`'s read r where `from_other[r]` (sarlacc_dev_subseq).  No tags go along."""
        n = len(self)
        st = np.ascontiguousarray(start, dtype=np.int32)
        wd = np.ascontiguousarray(np.maximum(np.asarray(width, dtype=np.int64), 0), dtype=np.int32)
        sel = None if from_other is None else np.ascontiguousarray(from_other, dtype=np.uint8)
        for what, a in (("start", st), ("width", wd), ("from_other", sel)):
            if a is not None and a.shape != (n,):
                raise _lib.SarlaccError("'%s' holds %d entries for %d reads" % (what, a.size, n))
        if other is not None and len(other) != n:
            raise _lib.SarlaccError("'other' holds %d reads, this batch %d" % (len(other), n))
        off = np.zeros(n + 1, np.int64)
        total = int(wd.sum(dtype=np.int64))
        chars = _lib.host_array(max(total, 1), np.uint8)
        o_seq, o_off = (other.seq, other.off) if other is not None else (None, None)
        check(_lib.lib().sarlacc_dev_subseq(self.seq, self.off, o_seq, o_off, sel, st, wd, n, chars, chars.size, off, None))
        return StringSet(chars, off)

    def realize(self, idx, reversed_, trim_start=None, trim_end=None):
        """Reads `idx` (0-based) of this batch, reverse-complemented where `reversed_`, cut to the
        1-based inclusive [trim_start, trim_end] of the oriented read (whole read when None):
        the device half of realizeReads (R/realizeReads.R:28-43).  `.tags` go along in `idx` order, each read's bytes
        unchanged (a splice with src): MM / ML / mv no longer fit a trimmed or reversed read -- drop_tags."""
        idx = np.ascontiguousarray(idx, dtype=np.int64)
        rev = np.ascontiguousarray(reversed_, dtype=np.uint8)
        if idx.ndim != 1 or (idx.size and (idx.min() < 0 or idx.max() >= len(self))):
            raise _lib.SarlaccError("'idx' must be a vector of read numbers in 0..%d" % (len(self) - 1))
        w = np.diff(self.off_host)[idx]
        ts = np.ones(idx.size, np.int32) if trim_start is None else np.ascontiguousarray(trim_start, dtype=np.int32)
        te = w.astype(np.int32) if trim_end is None else np.ascontiguousarray(trim_end, dtype=np.int32)
        for what, a in (("reversed_", rev), ("trim_start", ts), ("trim_end", te)):
            if a.shape != idx.shape:
                raise _lib.SarlaccError("'%s' holds %d entries for the %d reads of 'idx'" % (what, a.size, idx.size))
        if idx.size and ((ts < 1).any() or (te > w).any()):
            raise _lib.SarlaccError("trim coordinates outside the read")
        ow = np.maximum(te.astype(np.int64) - ts + 1, 0)
        ooff = np.zeros(idx.size + 1, np.int64)
        np.cumsum(ow, out=ooff[1:])
        d = self._like(ooff)
        if idx.size:
            d_idx, d_rev, d_ts = DevBuffer.from_numpy(idx), DevBuffer.from_numpy(rev), DevBuffer.from_numpy(ts)   # kept alive over the call
            check(_lib.lib().sarlacc_dev_realize(self.seq, self.qual, self.off, d_idx, d_rev, d_ts, idx.size, d.off, d.seq, d.qual, None))
        if self.tags is not None:
            d.tags = self._tags().take(idx)
        return d

    def scramble(self, seed):
        """.scramble_input (R/getAdaptorThresholds.R:68-92) on the device, deterministic in `seed`.  The result carries no tags."""
        d = self._like(self.off_host.copy())
        check(_lib.lib().sarlacc_dev_scramble(self.seq, self.qual, self.off, len(self), int(seed), d.seq, d.qual, None))
        return d

    def align_block(self, adaptor, gap_opening, gap_extension, sec_starts=(), sec_ends=()):
        """adaptor_align (src/adaptor_align.cpp:11-77) on the resident batch, results left in HBM as ONE block (DevBuffer, n,
        number of sections): scores | starts | ends | section starts | section widths (include/sarlacc_amd.h,
        sarlacc_dev_choose_strand) -- one allocation per call, and one download for whoever wants them on the host."""
        n = len(self)
        ns = np.asarray(sec_starts).size
        nsec = max(ns, 1)
        blk = DevBuffer(16 * n + 8 * n * nsec)
        base = blk.ptr.value
        device.dev_align(self.seq, self.qual, self.off, n, self.max_len, self._encoding(), gap_opening, gap_extension, adaptor,
                         True, sec_starts, sec_ends, base, base + 8 * n, base + 12 * n, base + 16 * n, base + 16 * n + 4 * n * nsec,
                         stream=None)
        return blk, n, ns

    @staticmethod
    def block_to_host(block):
        """A result block of align_block / choose_strand as (scores, starts, ends, [section starts], [section widths])."""
        blk, n, ns = block
        nsec = max(ns, 1)
        o_st, o_en, o_so, o_sw = 8 * n, 12 * n, 16 * n, 16 * n + 4 * n * nsec
        host = _lib.host_array(blk.nbytes, np.uint8)
        check(_lib.lib().sarlacc_dev_download(host, blk, blk.nbytes))
        scores = host[:o_st].view(np.float64)
        starts, ends = host[o_st:o_en].view(np.int32), host[o_en:o_so].view(np.int32)
        so_h, sw_h = host[o_so:o_sw].view(np.int32), host[o_sw:].view(np.int32)
        return (scores, starts, ends, [so_h[k * n:(k + 1) * n] for k in range(ns)], [sw_h[k * n:(k + 1) * n] for k in range(ns)])

    @staticmethod
    def choose_strand(cs, ce, rs, re):
        """.resolve_strand + the row selection of .align_AA_internal (R/adaptorAlign.R:112-122, :190-207) on four result blocks
        in HBM (sarlacc_dev_choose_strand): (rows of adaptor 1, rows of adaptor 2, reversed) on the host -- half the bytes of
        the four blocks cross PCIe and no host pass selects rows."""
        n = cs[1]
        if not (ce[1] == rs[1] == re[1] == n and cs[2] == rs[2] and ce[2] == re[2]):
            raise _lib.SarlaccError("strand choice: result blocks of different shapes")
        out1, out2, rev = DevBuffer(cs[0].nbytes), DevBuffer(ce[0].nbytes), DevBuffer(max(n, 1))
        check(_lib.lib().sarlacc_dev_choose_strand(cs[0], ce[0], rs[0], re[0], n, cs[2], ce[2], out1, out2, rev, None))
        return (DeviceReads.block_to_host((out1, n, cs[2])), DeviceReads.block_to_host((out2, n, ce[2])),
                rev.to_numpy(np.uint8, n).view(np.bool_))

    def align_map(self, adaptor, gap_opening, gap_extension, sec_starts=(), sec_ends=()):
        """adaptor_align (src/adaptor_align.cpp:11-77) on the resident batch: (scores, starts, ends,
        [section starts], [section widths]) as numpy arrays, same conventions as calls.adaptor_align."""
        ns = np.asarray(sec_starts).size
        if len(self) == 0:
            return np.zeros(0), np.zeros(0, np.int32), np.zeros(0, np.int32), [np.zeros(0, np.int32)] * ns, [np.zeros(0, np.int32)] * ns
        return self.block_to_host(self.align_block(adaptor, gap_opening, gap_extension, sec_starts, sec_ends))

    def align_scores(self, adaptor, gap_opening, gap_extension, local=True):
        """adaptor_align_score_only / barcode_align on the resident batch."""
        n = len(self)
        if n == 0:
            return np.zeros(0)
        scores = DevBuffer(8 * n)
        device.dev_align(self.seq, self.qual, self.off, n, self.max_len, self._encoding(), gap_opening, gap_extension, adaptor,
                         local, d_scores=scores, stream=None)
        return scores.to_numpy(np.float64, n)

    def barcode_panel(self, barcodes, gap_opening, gap_extension, all_scores=False):
        """calls.barcode_panel on the resident batch: only best / score / next best (20 bytes per read, whatever the panel's
        size) come back, and the score matrix when asked for."""
        from .calls import _numeric, _panel_args, _panel_result
        from .encoding import as_encoding
        chars, boff, nb = _panel_args(barcodes)
        go = _numeric(gap_opening, "gap opening penalty")
        ge = _numeric(gap_extension, "gap extension penalty")
        enc = as_encoding(self._encoding())
        n = len(self)
        best, score, nxt, matrix = _panel_result(n, nb, all_scores)
        if n:
            d_best, d_score, d_next = DevBuffer(4 * n), DevBuffer(8 * n), DevBuffer(8 * n)
            d_all = DevBuffer(8 * n * nb) if all_scores and nb else None
            check(_lib.lib().sarlacc_dev_barcode_panel(self.seq, self.qual, self.off, n, self.max_len, enc.errors, enc.names,
                                                       len(enc), go, ge, chars, boff, nb, d_best, d_score, d_next, d_all, None))
            for host, dev in ((best, d_best), (score, d_score), (nxt, d_next)):
                check(_lib.lib().sarlacc_dev_download(host, dev, host.nbytes))
            if d_all is not None:
                check(_lib.lib().sarlacc_dev_download(matrix, d_all, 8 * n * nb))
        return (best, score, nxt, matrix[:nb * n].reshape(nb, n)) if all_scores else (best, score, nxt)

    def profile(self, reference, gap_opening, gap_extension):
        """calls.profile_reads on the resident batch (sarlacc_dev_profile_reads + sarlacc_profile_fetch): the same raw arrays;
        only the scores, the edit distances and the reduced profile come back."""
        from .calls import _numeric, _profile_fetch, _string
        from .encoding import as_encoding
        rf = _string(reference, "reference sequence")
        go = _numeric(gap_opening, "gap opening penalty")
        ge = _numeric(gap_extension, "gap extension penalty")
        enc = as_encoding(self._encoding())
        n = len(self)
        d_scores, d_edits = DevBuffer(8 * max(n, 1)), DevBuffer(4 * max(n, 1))
        ni, nr, no = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        check(_lib.lib().sarlacc_dev_profile_reads(self.seq, self.qual, self.off, n, self.max_len, enc.errors, enc.names, len(enc), go, ge,
                                                   rf, len(rf), d_scores, d_edits, C.byref(ni), C.byref(nr), C.byref(no), None))
        out = _profile_fetch(len(rf), ni.value, nr.value, no.value)
        out["score"], out["edit"] = d_scores.to_numpy(np.float64, n), d_edits.to_numpy(np.int32, n)
        return out

    def sketch(self, k=13, buckets=64, canonical=True):
        """The one-permutation MinHash sketch of every read (sarlacc_dev_sketch_reads): (uint64[n, buckets]
        bucket minima of the k-mer hashes, 2^64 - 1 in an empty bucket; int32[n] numbers of k-mers), on the host."""
        from . import sketch as sk
        k, buckets, _, _ = sk.check_args(k, buckets)
        n = len(self)
        if n == 0:
            return np.zeros((0, buckets), np.uint64), np.zeros(0, np.int32)
        d_sketch, d_nk = sk.sketch_reads(self.seq, self.off, n, k, buckets, canonical)
        return d_sketch.to_numpy(np.uint64, n * buckets).copy().reshape(n, buckets), d_nk.to_numpy(np.int32, n).copy()
