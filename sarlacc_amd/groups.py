"""readGroups: per-read pre-groups from the records of sam2ranges (include/sarlacc_amd.h "pre-groups of a read batch",
csrc/read_groups.hip).  The reference's correction vignette builds the `groups` of umiGroup from a mapping -- "each set
of reads mapping to the same transcript would then be defined as a single group", with the name of the reference
sequence taken from sam2ranges() -- and leaves the join of records to reads to the user; here it is four device calls:
names matched, one record picked per read, labels by locus where asked, labels split into CSR groups."""
import ctypes as C
import numbers

import numpy as np

from . import _lib
from ._lib import check
from .strset import StringSet, StrList

BY = ("reference", "locus")
INT_MAX = 2 ** 31 - 1
COLUMNS = ("seqnames", "start", "width", "strand", "names")


def read_names(reads):
    """The names of `reads` as a StringSet: a resident.DeviceReads or generics.Reads (its .names), a StrList (handed
    over undecoded) or a list of str."""
    names = reads.names if hasattr(reads, "names") else reads
    if names is None:
        raise ValueError("reads have no names")
    if isinstance(names, StrList):
        return names.ss
    names = list(names)
    if not all(isinstance(x, str) for x in names):
        raise ValueError("read names should be strings")
    return StringSet.from_strings(names)


def check_args(ranges, by, maxgap):
    """Rule 5: everything that can be refused before a device is touched.  Returns the columns (seqnames, start, width,
    strand bytes, names as a StringSet) and the integer maxgap."""
    if by not in BY:
        raise ValueError("'by' should be one of %s" % ", ".join(repr(b) for b in BY))
    if isinstance(maxgap, (bool, np.bool_)) or not isinstance(maxgap, numbers.Integral) or not 0 <= int(maxgap) <= INT_MAX:
        raise ValueError("'maxgap' should be an integer in 0 .. 2^31 - 1")
    missing = [c for c in COLUMNS + ("seqinfo",) if c not in ranges]
    if missing:
        raise ValueError("'ranges' lacks %s: it should be what sam2ranges returns" % ", ".join(missing))
    ref = np.ascontiguousarray(ranges["seqnames"], dtype=np.int32)
    start = np.ascontiguousarray(ranges["start"], dtype=np.int32)
    width = np.ascontiguousarray(ranges["width"], dtype=np.int32)
    strand = np.asarray(ranges["strand"])
    strand = np.ascontiguousarray(strand.astype("S1").view(np.uint8) if strand.size else np.zeros(0, np.uint8))
    names = ranges["names"]
    names = names.ss if isinstance(names, StrList) else StringSet.from_strings(list(names))
    lengths = {c: int(n) for c, n in zip(COLUMNS, (ref.size, start.size, width.size, strand.size, len(names)))}
    if len(set(lengths.values())) != 1:
        raise ValueError("columns of 'ranges' differ in length: " + ", ".join("%s %d" % kv for kv in lengths.items()))
    nref = len(ranges["seqinfo"]["seqnames"])
    if ref.size and (int(ref.min()) < 0 or int(ref.max()) >= nref):
        k = int(np.flatnonzero((ref < 0) | (ref >= nref))[0])
        raise ValueError("row %d of 'ranges': seqname code %d outside the seqinfo (%d names)" % (k + 1, int(ref[k]), nref))
    if width.size and int(width.min()) < 0:
        raise ValueError("row %d of 'ranges': negative width" % (int(np.flatnonzero(width < 0)[0]) + 1))
    return (ref, start, width, strand, names), int(maxgap)


def empty_result(n, unmatched=0):
    """No read has a row: `unmatched` rows name none."""
    minus = np.full(n, -1, np.int32)
    return {"record": minus, "n.records": np.zeros(n, np.int32), "reference": minus.copy(), "group": minus.copy(),
            "groups": (np.zeros(1, np.int64), np.zeros(0, np.int32)), "unmatched.records": np.int64(unmatched)}


def _up(a, dtype):
    from .resident import DevBuffer
    a = np.ascontiguousarray(a, dtype=dtype)
    return DevBuffer.from_numpy(a if a.size else np.zeros(1, dtype))


def names_match(read_names_ss, record_names_ss):
    """sarlacc_dev_names_match on two StringSets: (device int32 read of every record, unmatched records)."""
    from .resident import DevBuffer
    n, m = len(read_names_ss), len(record_names_ss)
    out, unmatched = DevBuffer(4 * max(m, 1)), C.c_int64(0)
    check(_lib.lib().sarlacc_dev_names_match(_up(read_names_ss.chars[:max(read_names_ss.total, 1)], np.uint8), _up(read_names_ss.off, np.int64), n,
                                             _up(record_names_ss.chars[:max(record_names_ss.total, 1)], np.uint8),
                                             _up(record_names_ss.off, np.int64), m, out, C.byref(unmatched), None))
    return out, unmatched.value


def records_pick(d_read_of_record, d_width, m, n):
    """sarlacc_dev_records_pick: (device record of every read, device records per read)."""
    from .resident import DevBuffer
    rec, cnt = DevBuffer(4 * max(n, 1)), DevBuffer(4 * max(n, 1))
    check(_lib.lib().sarlacc_dev_records_pick(d_read_of_record, d_width, m, n, rec, cnt, None))
    return rec, cnt


def locus_labels(d_ref, d_strand, d_start, d_width, m, d_record_of_read, n, maxgap, ignore_strand):
    """sarlacc_dev_locus_labels: (device labels, number of groups)."""
    from .resident import DevBuffer
    label, ng = DevBuffer(4 * max(n, 1)), C.c_int64(0)
    check(_lib.lib().sarlacc_dev_locus_labels(d_ref, d_strand, d_start, d_width, m, d_record_of_read, n, maxgap,
                                              1 if ignore_strand else 0, label, C.byref(ng), None))
    return label, ng.value


def labels_csr(d_label, n):
    """sarlacc_dev_labels_csr: the CSR pair (off int64[G + 1], members int32) on the host."""
    from .resident import DevBuffer
    off, members = DevBuffer(8 * (n + 1)), DevBuffer(4 * max(n, 1))
    ng, nm = C.c_int64(0), C.c_int64(0)
    check(_lib.lib().sarlacc_dev_labels_csr(d_label, n, off, members, C.byref(ng), C.byref(nm), None))
    return off.to_numpy(np.int64, ng.value + 1).copy(), members.to_numpy(np.int32, nm.value).copy()


def read_groups(ranges, reads, by="reference", maxgap=0, ignore_strand=True):
    """generics.readGroups."""
    rnames = read_names(reads)
    (ref, start, width, strand, qnames), maxgap = check_args(ranges, by, maxgap)
    n, m = len(rnames), len(qnames)
    if n == 0 or m == 0:
        return empty_result(n, m)
    d_read_of_record, unmatched = names_match(rnames, qnames)
    d_width = _up(width, np.int32)
    d_record, d_count = records_pick(d_read_of_record, d_width, m, n)
    record = d_record.to_numpy(np.int32, n).copy()
    reference = np.where(record >= 0, ref[np.maximum(record, 0)], -1).astype(np.int32)
    if by == "reference":
        group, d_label = reference, _up(reference, np.int32)
    else:
        d_label, _ = locus_labels(_up(ref, np.int32), _up(strand, np.uint8), _up(start, np.int32), d_width, m, d_record, n,
                                  maxgap, ignore_strand)
        group = d_label.to_numpy(np.int32, n).copy()
    return {"record": record, "n.records": d_count.to_numpy(np.int32, n).copy(), "reference": reference, "group": group,
            "groups": labels_csr(d_label, n), "unmatched.records": np.int64(unmatched)}
