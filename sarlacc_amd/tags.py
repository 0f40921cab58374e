"""Tags of a resident read batch (include/sarlacc_amd.h "tags of a resident batch", csrc/bam_tags.hip): the raw aux bytes
of every read's BAM record, flat in HBM with n + 1 offsets, as names are held -- kept by DeviceReads.from_bam /
stream_bam(keep_tags=True), queried and edited on the device (DeviceReads.tag / set_tag / drop_tags), carried through
DeviceReads.realize and written by DeviceReads.to_bam.  Values of type f and B are never decoded here: they are kept
and written as they lie."""
import ctypes as C
import re

import numpy as np

from . import _lib
from ._lib import check
from .strset import StringSet, StrList

_NAME = re.compile(r"[A-Za-z][A-Za-z0-9]")
STRING_TYPES, INT_TYPES = b"AZH", b"cCsSiI"
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


def tag_name(name):
    """The two bytes of a tag name; ValueError for anything but [A-Za-z][A-Za-z0-9]."""
    if isinstance(name, bytes):
        name = name.decode("latin-1")
    if not isinstance(name, str) or not _NAME.fullmatch(name):
        raise ValueError("a tag name is two characters, [A-Za-z][A-Za-z0-9]: %r" % (name,))
    return name.encode()


def tag_column(values, n):
    """(kind, data) of the values a tag is set to on n reads: ('Z', StringSet) for a StringSet, a StrList or a list of
    str, ('i', int32 array) for integers.  ValueError for a wrong count, a byte a Z value cannot hold (outside
    ' '..'~'), an integer outside int32, or anything else."""
    if isinstance(values, StrList):
        values = values.ss
    if not isinstance(values, StringSet):
        values = list(values) if not isinstance(values, np.ndarray) else values
        if len(values) and all(isinstance(v, (str, bytes)) for v in values):
            values = StringSet.from_strings(values)
    if isinstance(values, StringSet):
        if len(values) != n:
            raise ValueError("%d tag values for %d reads" % (len(values), n))
        chars = values.chars[:values.total]
        if chars.size and (chars.min() < 32 or chars.max() > 126):
            raise ValueError("a Z tag value holds only the bytes ' '..'~'")
        return "Z", values
    arr = np.asarray(values)
    if arr.ndim != 1 or arr.dtype == np.bool_ or not (np.issubdtype(arr.dtype, np.integer) or arr.size == 0):
        raise ValueError("tag values are strings (a Z tag) or integers (an i tag)")
    if arr.size != n:
        raise ValueError("%d tag values for %d reads" % (arr.size, n))
    if arr.size and (int(arr.min()) < INT32_MIN or int(arr.max()) > INT32_MAX):
        raise ValueError("an i tag value lies in -2^31 .. 2^31 - 1")
    return "i", np.ascontiguousarray(arr, dtype=np.int32)


def present_mask(present, n):
    if present is None:
        return None
    mask = np.asarray(present)
    if mask.dtype != np.bool_ or mask.shape != (n,):
        raise ValueError("'present' is a boolean mask with one entry per read")
    return np.ascontiguousarray(mask, dtype=np.uint8)


class TagHit:
    """The result of DeviceTags.find: per read the type letter and where the value and the whole entry lie, on the
    device; how many reads hold the tag and the bytes of their string values."""

    def __init__(self, name, n):
        from .resident import DevBuffer
        self.name, self.n = name, n
        self.type = DevBuffer(max(n, 1))
        self.val_off, self.val_len, self.tag_off, self.tag_len = (DevBuffer(8 * max(n, 1)) for _ in range(4))
        self.n_present = self.string_bytes = 0


class DeviceTags:
    """aux bytes / offsets in HBM + the host copy of the offsets."""

    def __init__(self, aux, off_dev, off_host):
        self.aux, self.off, self.off_host = aux, off_dev, off_host

    def __len__(self):
        return len(self.off_host) - 1

    @property
    def total(self):
        return int(self.off_host[-1])

    @classmethod
    def empty(cls, n):
        """n reads without a tag."""
        from .resident import DevBuffer
        off = np.zeros(n + 1, np.int64)
        return cls(DevBuffer(1), DevBuffer.from_numpy(off), off)

    @classmethod
    def upload(cls, areas):
        """areas: one bytes object of BAM aux bytes per read."""
        from .resident import DevBuffer
        ss = StringSet.from_strings([bytes(a) for a in areas])
        return cls(DevBuffer.from_numpy(ss.chars), DevBuffer.from_numpy(ss.off), ss.off.copy())

    def download(self):
        """The aux bytes of every read, as a list of bytes."""
        raw = self.aux.to_numpy(np.uint8, self.total).tobytes()
        return [raw[a:b] for a, b in zip(self.off_host[:-1], self.off_host[1:])]

    def find(self, name, results=True):
        """sarlacc_dev_bam_tags_find for the two bytes `name`: a TagHit, or with results=False nothing but the walk
        over every read's tags ("read K: malformed tags")."""
        n = len(self)
        hit = TagHit(name, n) if results else None
        present, sbytes = C.c_int64(0), C.c_int64(0)
        out = (hit.type, hit.val_off, hit.val_len, hit.tag_off, hit.tag_len) if results else (None,) * 5
        check(_lib.lib().sarlacc_dev_bam_tags_find(self.aux, self.off, n, name, *out, C.byref(present), C.byref(sbytes), None))
        if results:
            hit.n_present, hit.string_bytes = present.value, sbytes.value
        return hit

    def validate(self):
        self.find(b"\0\0", results=False)
        return self

    def values(self, name):
        """What DeviceReads.tag returns."""
        from .resident import DevBuffer
        n = len(self)
        hit = self.find(name)
        types = hit.type.to_numpy(np.uint8, n)
        held = bytes(np.unique(types[types != 0]).tolist())
        for t in held:
            if t not in STRING_TYPES + INT_TYPES:
                raise _lib.SarlaccError("tag %s has type %s on read %d: float and array values are not decoded (they are kept "
                                        "and written as they lie)" % (name.decode(), chr(t), int(np.flatnonzero(types == t)[0]) + 1))
        lib = _lib.lib()
        if held and held[0] in INT_TYPES and not any(t in STRING_TYPES for t in held):
            vals, mask = DevBuffer(8 * max(n, 1)), DevBuffer(max(n, 1))
            check(lib.sarlacc_dev_bam_tags_ints(self.aux, self.off, n, name, hit.type, hit.val_off, vals, mask, None))
            return vals.to_numpy(np.int64, n).copy(), mask.to_numpy(np.uint8, n).view(np.bool_).copy()
        # strings, and the error of a batch that mixes strings and integers
        chars, soff = DevBuffer(max(hit.string_bytes, 1)), DevBuffer(8 * (n + 1))
        check(lib.sarlacc_dev_bam_tags_strings(self.aux, self.off, n, name, hit.type, hit.val_off, hit.val_len, chars, soff, None))
        raw = chars.to_numpy(np.uint8, hit.string_bytes)
        ss = StringSet(raw.copy() if raw.size else np.zeros(1, np.uint8), soff.to_numpy(np.int64, n + 1).copy())
        return StrList(ss), types != 0

    def splice(self, src=None, cut=None, name=None, column=None, mask=None):
        """sarlacc_dev_bam_tags_splice: a new DeviceTags whose read r holds the tags of read src[r] (None: r) without the
        span cut = (device offsets, host lengths) and, where mask[r] (uint8, None: everywhere), a new entry `name` from
        column = (kind, data) of tag_column.  The output offsets are computed here, from lengths the host holds."""
        from .resident import DevBuffer
        if src is not None:
            src = np.ascontiguousarray(src, dtype=np.int64)
            if src.size and (src.min() < 0 or src.max() >= len(self)):
                raise _lib.SarlaccError("tag splice: read index outside the batch")
        n_out = len(self) if src is None else src.size
        length = np.diff(self.off_host) if src is None else np.diff(self.off_host)[src]
        d_src = d_cut_off = d_cut_len = d_chars = d_coff = d_ints = d_mask = None
        if src is not None:
            d_src = DevBuffer.from_numpy(src if n_out else np.zeros(1, np.int64))
        if cut is not None:
            d_cut_off, cut_len = cut
            cut_len = np.ascontiguousarray(cut_len, dtype=np.int64)
            d_cut_len = DevBuffer.from_numpy(cut_len if cut_len.size else np.zeros(1, np.int64))
            length = length - cut_len
        kind = 0
        if column is not None:
            kind, data = column
            extra = (np.diff(data.off) + 4) if kind == "Z" else np.full(n_out, 7, np.int64)
            if mask is not None:
                extra = extra * (mask != 0)
                d_mask = DevBuffer.from_numpy(mask if mask.size else np.zeros(1, np.uint8))
            length = length + extra
            if kind == "Z":
                d_chars, d_coff = DevBuffer.from_numpy(data.chars), DevBuffer.from_numpy(data.off)
            else:
                d_ints = DevBuffer.from_numpy(data if data.size else np.zeros(1, np.int32))
            kind = ord(kind)
        ooff = np.zeros(n_out + 1, np.int64)
        np.cumsum(length, out=ooff[1:])
        out = DeviceTags(DevBuffer(max(int(ooff[-1]), 1)), DevBuffer.from_numpy(ooff), ooff)
        check(_lib.lib().sarlacc_dev_bam_tags_splice(self.aux, self.off, len(self), d_src, n_out, d_cut_off, d_cut_len, name, kind,
                                                     d_chars, d_coff, d_ints, d_mask, out.off, out.aux, None))
        return out

    def take(self, idx):
        """The tags of the reads `idx`, in that order (a splice with src)."""
        return self.splice(src=idx)

    def set(self, name, column, mask=None):
        """What DeviceReads.set_tag does to the tags, `column` and `mask` those of tag_column and present_mask: one
        find + one splice."""
        n = len(self)
        hit = self.find(name)
        cut_len = hit.tag_len.to_numpy(np.int64, n).copy()
        if mask is not None:
            cut_len[mask == 0] = 0
        return self.splice(cut=(hit.tag_off, cut_len), name=name, column=column, mask=mask)

    def drop(self, name):
        """The tags without every entry named `name`."""
        out, n = self, len(self)
        while n:
            hit = out.find(name)
            if not hit.n_present:
                break
            out = out.splice(cut=(hit.tag_off, hit.tag_len.to_numpy(np.int64, n).copy()))
        return out
