"""BAM tags on the device: sarlacc_dev_bam_tags_find / _strings / _ints / _splice, sarlacc_dev_bam_format_size_aux /
_format_aux, sarlacc_dev_bam_reads_aux_range / _aux_extract, and DeviceReads.from_bam(keep_tags=True) / tag / set_tag /
drop_tags / realize / to_bam on top of them.  Everything is compared exactly with tests/bam_tags_cases.py, the
plain-Python restatement that tests/test_bam_tags_host.py pins.

The NUL of a Z / H value is searched 16 bytes per lane, 1 024 bytes per step of the wavefront, so the Z lengths tried sit
around 16, 64 (four lanes), 1 024 and 2 048 (one and two steps) and 4 096.  Malformed inputs are ordinary refusals:
every case lies wholly inside its allocation."""
import ctypes as C
import gzip

import numpy as np
import pytest

from tests import bam_cases as B
from tests import bam_tags_cases as T
from tests import bam_write_cases as Bw
from tests.test_gpu_bam_write import GUARD, device_batch, first_difference

pytestmark = pytest.mark.gpu

Z_LENGTHS = (0, 1, 15, 16, 17, 62, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 4097)


def _lib():
    from sarlacc_amd import _lib
    return _lib


class Areas:
    """Aux areas on the device, the flat bytes `shift` bytes into their (16-byte aligned) buffer."""

    def __init__(self, areas, shift=0):
        from sarlacc_amd.resident import DevBuffer
        self.areas, self.n = areas, len(areas)
        flat = b"".join(areas)
        self.buf = DevBuffer.from_numpy(np.frombuffer(b"\xaa" * shift + flat + b"\xaa", np.uint8))
        assert self.buf.ptr.value % 16 == 0
        self.aux = C.c_void_p(self.buf.ptr.value + shift)
        self.off_host = np.zeros(self.n + 1, np.int64)
        np.cumsum([len(a) for a in areas], out=self.off_host[1:])
        self.off = DevBuffer.from_numpy(self.off_host)

    def find(self, tag, results=True):
        from sarlacc_amd.resident import DevBuffer
        n = self.n
        out = [DevBuffer.from_numpy(np.full(n + 1, 0x77, np.uint8))] + [DevBuffer.from_numpy(np.full(n + 1, -7, np.int64)) for _ in range(4)]
        present, sbytes = C.c_int64(-1), C.c_int64(-1)
        _lib().check(_lib().lib().sarlacc_dev_bam_tags_find(self.aux, self.off, n, tag, *(out if results else [None] * 5),
                                                            C.byref(present), C.byref(sbytes), None))
        host = [out[0].to_numpy(np.uint8, n + 1)] + [b.to_numpy(np.int64, n + 1) for b in out[1:]]
        if results:
            assert host[0][-1] == 0x77 and all(h[-1] == -7 for h in host[1:]), "written past n entries"
        self.hit = out
        return [h[:n] for h in host], present.value, sbytes.value

    def check_find(self, tag):
        got, present, sbytes = self.find(tag)
        want = [T.find(a, tag) for a in self.areas]
        for k, name in enumerate(("type", "value offset", "value bytes", "entry offset", "entry bytes")):
            assert got[k].tolist() == [w[k] for w in want], "%s of tag %r" % (name, tag)
        assert present == sum(1 for w in want if w[0])
        assert sbytes == sum(w[2] for w in want if w[0] and chr(w[0]) in "AZH")
        return got

    def strings(self, tag):
        from sarlacc_amd.resident import DevBuffer
        got, _, sbytes = self.find(tag)
        chars, soff = DevBuffer.from_numpy(np.full(sbytes + 16, 0xEE, np.uint8)), DevBuffer.from_numpy(np.full(self.n + 2, -7, np.int64))
        _lib().check(_lib().lib().sarlacc_dev_bam_tags_strings(self.aux, self.off, self.n, tag, self.hit[0], self.hit[1], self.hit[2],
                                                               chars, soff, None))
        off, raw = soff.to_numpy(np.int64, self.n + 2), chars.to_numpy(np.uint8, sbytes + 16)
        assert off[-1] == -7 and off[-2] == sbytes and (raw[sbytes:] == 0xEE).all()
        return [raw[a:b].tobytes() for a, b in zip(off[:-2], off[1:-1])]

    def ints(self, tag):
        from sarlacc_amd.resident import DevBuffer
        self.find(tag)
        vals, mask = DevBuffer(8 * max(self.n, 1)), DevBuffer(max(self.n, 1))
        _lib().check(_lib().lib().sarlacc_dev_bam_tags_ints(self.aux, self.off, self.n, tag, self.hit[0], self.hit[1], vals, mask, None))
        return vals.to_numpy(np.int64, self.n), mask.to_numpy(np.uint8, self.n).astype(bool)

    def splice(self, want, src=None, cuts=None, tag=None, kind=None, column=None, mask=None, shift=0):
        """The splice through the C ABI, its output offsets those of the expected areas `want`; the areas it wrote."""
        from sarlacc_amd.resident import DevBuffer
        from sarlacc_amd.strset import StringSet
        n_out = len(want)
        ooff = np.zeros(n_out + 1, np.int64)
        np.cumsum([len(w) for w in want], out=ooff[1:])
        total = int(ooff[-1])
        d_out = DevBuffer.from_numpy(np.full(2 * GUARD + shift + total, 0xEE, np.uint8))
        d_ooff = DevBuffer.from_numpy(ooff)
        d_src = None if src is None else DevBuffer.from_numpy(np.array(list(src) + [0], np.int64))
        d_co = d_cl = d_chars = d_coff = d_ints = d_mask = None
        if cuts is not None:
            d_co = DevBuffer.from_numpy(np.array([c[0] for c in cuts] + [0], np.int64))
            d_cl = DevBuffer.from_numpy(np.array([c[1] for c in cuts] + [0], np.int64))
        if kind == "Z":
            ss = StringSet.from_strings(column)
            d_chars, d_coff = DevBuffer.from_numpy(ss.chars), DevBuffer.from_numpy(ss.off)
        elif kind == "i":
            d_ints = DevBuffer.from_numpy(np.array(list(column) + [0], np.int32))
        if mask is not None:
            d_mask = DevBuffer.from_numpy(np.array(list(mask) + [0], np.uint8))
        _lib().check(_lib().lib().sarlacc_dev_bam_tags_splice(self.aux, self.off, self.n, d_src, n_out, d_co, d_cl, tag, ord(kind) if kind else 0,
                                                              d_chars, d_coff, d_ints, d_mask, d_ooff,
                                                              C.c_void_p(d_out.ptr.value + GUARD + shift), None))
        got = d_out.to_numpy(np.uint8, 2 * GUARD + shift + total)
        assert (got[:GUARD + shift] == 0xEE).all() and (got[GUARD + shift + total:] == 0xEE).all(), "bytes written outside the range"
        raw = got[GUARD + shift:GUARD + shift + total].tobytes()
        return [raw[a:b] for a, b in zip(ooff[:-1], ooff[1:])]

    def check_splice(self, shift=0, **kw):
        want = T.splice(self.areas, **kw)
        got = self.splice(want, shift=shift, **kw)
        for r, (g, w) in enumerate(zip(got, want)):
            assert g == w, "output read %d" % r
        return want


# ---- find ----------------------------------------------------------------------------------------------------------------

FIELDS = ["aA:A:x", "ac:i:-5", "aC:i:200", "as:i:-300", "aS:i:40000", "ai:i:-70000", "aI:i:3000000000", "af:f:1.5", "aZ:Z:hello tag",
          "aH:H:1AE3", "bc:B:c,-1,2", "bC:B:C,1,2,255", "bs:B:s,-300", "bS:B:S,40000,1", "bi:B:i,-70000,5,6", "bI:B:I,3000000000",
          "bf:B:f,1,2", "be:B:C"]


def every_type_areas():
    """Reads that hold every type letter and B subtype, each tag once at the first, at the last and at middle positions;
    an empty read; reads that repeat a tag."""
    entries = [B.encode_tag(f) for f in FIELDS]
    assert None not in entries and {chr(e[2]) for e in entries} == set("AcCsSiIfZHB") and {chr(e[3]) for e in entries[10:]} == set(T.SUBTYPES)
    areas = [b"".join(entries[k:] + entries[:k]) for k in range(len(entries))]
    areas += [b"", b"".join(entries[::-1]), entries[8] + entries[1] + B.encode_tag("aZ:Z:second") + entries[1], entries[3]]
    return areas


@pytest.mark.parametrize("shift", range(16))
def test_find_every_type_at_every_alignment(shift):
    A = Areas(every_type_areas(), shift)
    for tag in [f[:2].encode() for f in FIELDS] + [b"zz", b"a\0"]:
        A.check_find(tag)


def z_areas():
    """A Z value of every length of Z_LENGTHS as the last entry of a read (its NUL is the read's last byte), in front of
    another entry, and as H behind a B array."""
    areas = []
    for n in Z_LENGTHS:
        val = bytes(33 + (7 * k) % 90 for k in range(n))
        areas += [b"NMC\x01" + T.z_entry(b"zv", val), T.z_entry(b"zv", val) + b"NMC\x02", b"mvBc\x03\0\0\0\x00\x00\x00" + b"zvH" + val + b"\0" + T.z_entry(b"RG", b"r")]
    return areas


@pytest.mark.parametrize("shift", range(16))
def test_find_z_lengths_at_every_alignment(shift):
    A = Areas(z_areas(), shift)
    A.check_find(b"zv")
    A.check_find(b"NM")       # behind the long value
    if shift in (0, 5):
        want = [a[v:v + n] for a, (_, v, n, _, _) in ((a, T.find(a, b"zv")) for a in A.areas)]
        assert A.strings(b"zv") == want


def test_find_empty_areas_and_empty_batch():
    A = Areas([b""] * 300)
    got = A.check_find(b"RX")
    assert not got[0].any()
    assert A.strings(b"RX") == [b""] * 300
    vals, mask = A.ints(b"RX")
    assert not vals.any() and not mask.any()
    E = Areas([])
    assert E.find(b"RX")[1:] == (0, 0) and E.strings(b"RX") == [] and E.check_splice() == []
    assert Areas([b"", b"RXZAC\0", b""]).check_find(b"RX")[0].tolist() == [0, ord("Z"), 0]


def test_find_many_tiny_reads():
    rng = np.random.default_rng(21)
    pool = [b"RXZACGT\0", b"NMC\x05", b"BCZbc01\0", b"tpAP", b"nsi\x01\x02\x03\x04"]
    areas = [b"".join(pool[j] for j in rng.permutation(5)[:int(rng.integers(0, 3))]) for _ in range(3000)]
    for shift in (0, 11):
        A = Areas(areas, shift)
        for tag in (b"RX", b"NM", b"ns"):
            A.check_find(tag)
    assert A.strings(b"RX") == T.string_values(areas, b"RX")[0]
    vals, mask = A.ints(b"ns")
    want = T.int_values(areas, b"ns")
    assert np.array_equal(vals, want[0]) and np.array_equal(mask, want[1])


def test_strings_and_ints_of_every_type():
    A = Areas(every_type_areas(), 3)
    for tag in (b"aA", b"aZ", b"aH"):
        assert A.strings(tag) == T.string_values(A.areas, tag)[0]
    mixed = [B.encode_tag(f) for f in ("xx:i:-5", "xx:i:200", "xx:i:-300", "xx:i:40000", "xx:i:-70000", "xx:i:3000000000")] + [b"", b"NMC\x01"]
    M = Areas(mixed, 9)
    assert {chr(a[2]) for a in mixed[:6]} == set("cCsSiI")
    vals, mask = M.ints(b"xx")
    assert vals.tolist() == [-5, 200, -300, 40000, -70000, 3000000000, 0, 0] and mask.tolist() == [True] * 6 + [False] * 2
    for tag in (b"ac", b"aI"):
        vals, mask = A.ints(tag)
        want = T.int_values(A.areas, tag)
        assert np.array_equal(vals, want[0]) and np.array_equal(mask, want[1])
    SarlaccError = _lib().SarlaccError
    first = {t: next(k for k, a in enumerate(A.areas) if T.find(a, t)[0]) + 1 for t in (b"ac", b"af", b"bc", b"aZ")}
    for tag, ty in ((b"ac", "c"), (b"af", "f"), (b"bc", "B")):
        with pytest.raises(SarlaccError) as e:
            A.strings(tag)
        assert str(e.value) == "read %d: tag %s has type %s" % (first[tag], tag.decode(), ty)
    for tag, ty in ((b"aZ", "Z"), (b"af", "f"), (b"bc", "B")):
        with pytest.raises(SarlaccError) as e:
            A.ints(tag)
        assert str(e.value) == "read %d: tag %s has type %s" % (first[tag], tag.decode(), ty)


# ---- malformed -----------------------------------------------------------------------------------------------------------

GOOD_AUX = b"NMC\x01RGZrun\0"
BAD = {
    "fewer than 3 bytes": b"NMC\x01XY",
    "type letter": b"NMz\x01",
    "fixed value past the end": b"NMC\x01nsi\x01\x02\x03",
    "B header past the end": b"mvBc\x01\0\0",
    "B payload past the end": b"mvBs\x02\0\0\0\x01\x02\x03",
    "B subtype": b"mvBA\x01\0\0\0A",
    "no NUL": b"NMC\x01RGZabcdefghijklmnopqrstuvwxyz",
    "no NUL, long": b"RGZ" + b"a" * 1500,
}


def _malformed(areas, shift=0):
    want = T.first_malformed(areas)
    assert want is not None
    A = Areas(areas, shift)
    for results in (True, False):
        with pytest.raises(_lib().SarlaccError) as e:
            A.find(b"RG", results)
        assert str(e.value) == "read %d: malformed tags" % want
    return want


@pytest.mark.parametrize("rule", sorted(BAD))
def test_malformed_in_the_first_the_middle_and_the_last_read(rule):
    bad = BAD[rule]
    with pytest.raises(T.Malformed):
        T.walk(bad)
    assert _malformed([bad] + [GOOD_AUX] * 9) == 1
    assert _malformed([GOOD_AUX] * 9 + [bad], shift=7) == 10
    assert _malformed([GOOD_AUX] * 4 + [b"", bad, b""] + [GOOD_AUX] * 300, shift=13) == 6
    assert _malformed([GOOD_AUX] * 70 + [bad] + [GOOD_AUX] * 70 + [BAD["type letter"]]) == 71      # the lowest is named


def test_the_refusal_comes_from_the_bound():
    # the next read's aux starts with what an over-running scanner would take: a NUL, enough payload
    assert _malformed([GOOD_AUX, b"RGZabc", b"\0\0A\0", GOOD_AUX]) == 2
    assert _malformed([GOOD_AUX, b"RGZ" + b"a" * 40, b"\0\0A\0" + GOOD_AUX], shift=3) == 2
    assert _malformed([b"mvBc\x04\0\0\0\x01", b"\x02\x03\x04NMC\x01", GOOD_AUX]) == 1
    assert _malformed([GOOD_AUX, b"mvBi\x02\0\0\0\x01\x02\x03\x04", b"NMC\x01NMC\x01", GOOD_AUX]) == 2
    assert _malformed([b"NMi\x01", b"\x02\x03\x04", GOOD_AUX]) == 1
    # and the same bytes with the bound moved are fine
    Areas([GOOD_AUX, b"RGZabc\0", b"\0\0A\0", GOOD_AUX]).check_find(b"RG")
    Areas([b"mvBc\x04\0\0\0\x01\x02\x03\x04", b"NMC\x01", GOOD_AUX]).check_find(b"NM")


# ---- splice --------------------------------------------------------------------------------------------------------------

def splice_areas():
    rng = np.random.default_rng(31)
    areas = T.random_areas(rng, 60, empty=0.25)
    areas[7] = T.basecaller_aux(rng, 3000, 7)
    return areas


def test_splice_src():
    areas = splice_areas()
    A = Areas(areas, 6)
    rng = np.random.default_rng(32)
    A.check_splice()                                               # identity
    A.check_splice(src=rng.permutation(60).tolist(), shift=1)
    A.check_splice(src=rng.integers(0, 60, 200).tolist(), shift=9)   # with repeats
    A.check_splice(src=[7, 7, 7])
    assert A.check_splice(src=[]) == []
    empties = [k for k, a in enumerate(areas) if not a]
    assert len(empties) > 3 and A.check_splice(src=empties * 2) == [b""] * (2 * len(empties))


def test_splice_drop():
    entries = [B.encode_tag(f) for f in FIELDS]
    areas = [b"".join(entries), b"", b"".join(entries[::-1]), entries[8], entries[8] + entries[0], entries[0] + entries[8]] + splice_areas()
    A = Areas(areas, 2)
    for tag in (b"aA", b"aZ", b"be", b"bi", b"zz", b"RG"):          # first, middle, last, absent
        cuts = [T.find(a, tag)[3:] for a in areas]
        want = A.check_splice(cuts=cuts, shift=4)
        assert want == T.drop_tag(areas, tag)


@pytest.mark.parametrize("length", [0, 1, 4095, 4096, 4097])
def test_splice_append_z(length):
    areas = splice_areas()[:12]
    A = Areas(areas, 15)
    column = [bytes(32 + (k + 3 * r) % 95 for k in range(length)) for r in range(12)]
    column[5] = b""
    A.check_splice(tag=b"RX", kind="Z", column=column, shift=length % 16)
    A.check_splice(tag=b"RX", kind="Z", column=column, mask=[r % 3 != 1 for r in range(12)])


def test_splice_append_i_and_replace():
    areas = splice_areas()
    A = Areas(areas, 8)
    values = [[-2 ** 31, -1, 0, 2 ** 31 - 1][r % 4] for r in range(60)]
    want = A.check_splice(tag=b"BC", kind="i", column=values)
    assert want[0].endswith(b"BCi\x00\x00\x00\x80") and want[3].endswith(b"BCi\xff\xff\xff\x7f")
    mask = [r % 5 != 2 for r in range(60)]
    A.check_splice(tag=b"BC", kind="i", column=values, mask=mask, shift=3)
    # replace: the found entry cut, the new one appended, in one pass -- longer and shorter values, holes in the mask
    for tag in (b"RG", b"MM", b"NM"):
        for column in ([b"x" * (r % 7) for r in range(60)], [b"a much longer value than before %d" % r * 3 for r in range(60)]):
            for m in (None, mask):
                cuts = [T.find(a, tag)[3:] if m is None or m[r] else (0, 0) for r, a in enumerate(areas)]
                want = A.check_splice(cuts=cuts, tag=tag, kind="Z", column=column, mask=m, shift=11)
                assert want == T.set_tag(areas, tag, "Z", column, m)
    A.check_splice(src=list(range(59, -1, -1)), cuts=[T.find(areas[59 - r], b"RG")[3:] for r in range(60)], tag=b"RG", kind="i",
                   column=values)


def test_splice_a_long_area_between_tiny_ones_at_every_alignment():
    big = T.z_entry(b"MM", bytes(48 + k % 10 for k in range(14001 - 4 - 4))) + b"NMC\x01"
    assert len(big) == 14001
    areas = [b"tpAP", b"", b"NMC\x02", big, b"", b"tpAQ", b"RXZA\0"]
    for shift in range(16):
        A = Areas(areas, (5 * shift) % 16)
        A.check_splice(src=[6, 3, 0, 1, 3, 2], shift=shift)
        A.check_splice(cuts=[(0, 0), (0, 0), (0, 4), (0, 7001), (0, 0), (0, 0), (0, 0)], tag=b"RX", kind="Z", column=[b"ACGT"] * 7, shift=shift)


# ---- writer --------------------------------------------------------------------------------------------------------------

class SizedAux:
    """Step 1 of the writer with tags through the C ABI (tests.test_gpu_bam_write.Sized with d_aux / d_aux_off)."""

    def __init__(self, batch, areas, with_aux=True, aux_shift=0):
        from sarlacc_amd.resident import DevBuffer
        from tests import bam_reads_cases as Rd
        names, seqs, quals = batch
        n = len(seqs)
        self.dev, self.n = device_batch(None, seqs, quals), n
        nb, noff = Rd.flat(names)
        self.names, self.noff = DevBuffer.from_numpy(np.frombuffer(nb or b"\0", np.uint8)), DevBuffer.from_numpy(noff)
        self.A = Areas(areas, aux_shift) if with_aux else None
        self.aux = (self.A.aux, self.A.off) if with_aux else (None, None)
        self.rec_off = DevBuffer.from_numpy(np.full(n + 2, -7, np.int64))
        self.cuts = DevBuffer.from_numpy(np.full(3 * n + 1, -7, np.int64))
        total = C.c_int64(-1)
        _lib().check(_lib().lib().sarlacc_dev_bam_format_size_aux(self.dev.seq, self.dev.qual, self.dev.off, n, self.names, self.noff, 1,
                                                                  *self.aux, self.rec_off, self.cuts, C.byref(total), None))
        ro = self.rec_off.to_numpy(np.int64, n + 2)
        assert ro[-1] == -7 and total.value == ro[-2]
        self.ro, self.cu = ro[:-1].copy(), self.cuts.to_numpy(np.int64, 3 * n + 1)

    def format(self, first=0, count=None, shift=0):
        from sarlacc_amd.resident import DevBuffer
        count = self.n - first if count is None else count
        nbytes = int(self.ro[first + count] - self.ro[first])
        d_out = DevBuffer.from_numpy(np.full(2 * GUARD + shift + nbytes, 0xEE, np.uint8))
        _lib().check(_lib().lib().sarlacc_dev_bam_format_aux(self.dev.seq, self.dev.qual, self.dev.off, self.names, self.noff, 1, *self.aux,
                                                             self.rec_off, first, count, C.c_void_p(d_out.ptr.value + GUARD + shift), None))
        got = d_out.to_numpy(np.uint8, 2 * GUARD + shift + nbytes)
        assert (got[:GUARD + shift] == 0xEE).all() and (got[GUARD + shift + nbytes:] == 0xEE).all(), "bytes written outside the range"
        return got[GUARD + shift:GUARD + shift + nbytes].tobytes()


def batch_areas(name):
    """Tags for the reads of bam_write_cases.BATCHES[name]: basecaller-like ones whose move table follows the read's
    length, random short lists, and reads without any."""
    batch = Bw.BATCHES[name]()
    rng = np.random.default_rng(41)
    areas = []
    for k, s in enumerate(batch[1]):
        r = k % 4
        if name != "tiny" and (r == 1 or len(s) > 4000):
            areas.append(T.basecaller_aux(rng, len(s), k))
        else:
            areas.append(b"" if r == 0 else T.encode(T.random_fields(rng, 3 if name == "tiny" else 8)))
    return batch, areas


@pytest.mark.parametrize("name", ["lengths", "tiny", "span"])
def test_writer_bytes_offsets_and_cuts(name):
    batch, areas = batch_areas(name)
    S = SizedAux(batch, areas, aux_shift=5)
    off, cuts = T.layout(*batch, areas)
    assert np.array_equal(S.ro, off) and np.array_equal(S.cu[:-1], cuts) and S.cu[-1] == -7
    got, recs = S.format(shift=3), T.record_list(*batch, areas)
    assert first_difference(got, b"".join(recs)) is None
    for k in range(len(recs)):
        assert got[off[k]:off[k + 1]] == recs[k], "record %d" % (k + 1)


def test_writer_ranges_at_every_record_boundary():
    batch, areas = batch_areas("forty")
    S, want = SizedAux(batch, areas), b"".join(T.record_list(*batch, areas))
    for shift in range(16):
        assert first_difference(S.format(shift=shift), want) is None, "misaligned by %d" % shift
    for k in range(1, 40):
        got = S.format(0, k, shift=k % 16) + S.format(k, 40 - k, shift=(3 * k) % 16)
        assert first_difference(got, want) is None, "split at record %d" % k
    assert S.format(7, 0) == b""


def test_writer_without_tags_is_the_existing_pair():
    from tests.test_gpu_bam_write import sized
    batch = Bw.batch_forty()
    old = sized(batch)
    S = SizedAux(batch, None, with_aux=False)
    assert np.array_equal(S.ro, old.ro) and np.array_equal(S.cu[:80], old.cu) and (S.cu[80:] == -7).all()
    assert S.format(shift=5) == old.format() == Bw.expected_records(*batch)
    E = SizedAux(batch, [b""] * 40)      # and with tags that are all empty: the same bytes, three cuts per record
    assert np.array_equal(E.ro, old.ro) and E.format() == old.format()
    assert np.array_equal(E.cu[0:120:3], old.cu[0::2]) and np.array_equal(E.cu[1:120:3], old.cu[1::2]) and np.array_equal(E.cu[2:120:3], old.ro[1:])


def many_tags(n):
    return [b"%c%c" % (65 + k // 26, 97 + k % 26) for k in range(n)]


def test_writer_refusals():
    good = (b"name", b"ACGTN", b"!I5~+")

    def refused(reads, areas):
        names, seqs, quals = ([r[k] for r in reads] for k in range(3))
        k, why = T.first_refusal(names, seqs, quals, areas)
        with pytest.raises(_lib().SarlaccError) as e:
            SizedAux((names, seqs, quals), areas)
        assert str(e.value) == "record %d: %s" % (k, why)
        return k, why
    assert refused([good] * 3, [GOOD_AUX, BAD["no NUL"], GOOD_AUX]) == (2, T.MALFORMED)
    assert refused([good] * 3, [GOOD_AUX, GOOD_AUX, b"NMC\x01RGZa\0NMC\x02"]) == (3, "tag NM appears twice")
    assert refused([good] * 3, [b"RXZA\0RXZA\0", BAD["B subtype"], b""]) == (1, "tag RX appears twice")
    assert refused([good, (b"n", b"ACGT", b"II I"), good], [GOOD_AUX, BAD["type letter"], GOOD_AUX]) == (2, Bw.QUAL)     # quality first
    assert refused([good, (b"n", b"ACGT", b"II I")], [b"NMC\x01NMC\x01", GOOD_AUX]) == (1, "tag NM appears twice")      # the lower record
    assert refused([good] * 2, [b"", b"NMC\x01" + BAD["fewer than 3 bytes"]])[1] == T.MALFORMED                            # malformed behind a repeat: malformed wins
    # more entries than lanes: repeats among the first 64, across them, and behind them
    tags = many_tags(80)
    area = lambda ts: b"".join(t + b"C\x01" for t in ts)      # noqa: E731
    SizedAux(([b"n"], [b"A"], [b"I"]), [area(tags)])
    for ts, twice in ((tags + [tags[3]], tags[3]), (tags + [tags[70]], tags[70]), (tags[:66] + [tags[65]], tags[65]), (tags[:65] + [tags[64]], tags[64]),
                      (tags[:64] + [tags[63]], tags[63]), (tags[:64] + [tags[0]] + tags[64:], tags[0])):
        assert refused([good], [area(ts)]) == (1, "tag %s appears twice" % twice.decode())


# ---- files ---------------------------------------------------------------------------------------------------------------

def sam_lines(names, seqs, quals, areas):
    return ["\t".join([Bw.qname(nm).decode(), "4", "*", "0", "0", "*", "*", "0", "0", s.decode() or "*", q.decode() if s else "*"] + B._tags_text(a)[0])
            for nm, s, q, a in zip(names, seqs, quals, areas)]


def tagged_batch(name="file"):
    from sarlacc_amd.tags import DeviceTags
    batch, areas = batch_areas(name)
    dev = device_batch(*batch)
    dev.tags = DeviceTags.upload(areas)
    return dev, batch, areas


def test_to_bam_with_tags_and_back(tmp_path):
    from sarlacc_amd.resident import DeviceReads
    dev, batch, areas = tagged_batch()
    for block_bytes in (256 << 20, 30000):      # one range, several ranges
        path = str(tmp_path / ("t%d.bam" % block_bytes))
        written = dev.to_bam(path, block_bytes=block_bytes)
        data = open(path, "rb").read()
        assert written == len(data)
        raw = gzip.decompress(data)
        assert raw == Bw.header_bytes() + b"".join(T.record_list(*batch, areas))
        assert B.bam_to_sam(raw).decode().splitlines()[1:] == sam_lines(*batch, areas)
        back = DeviceReads.from_bam(path, keep_tags=True)
        assert back.tags.download() == areas and np.array_equal(back.tags.off_host, dev.tags.off_host)
        assert back.names.tolist() == [Bw.qname(nm).decode() for nm in batch[0]]
        assert DeviceReads.from_bam(path).tags is None
    chunks = list(DeviceReads.stream_bam(path, 7, block_bytes=20000, keep_tags=True))
    assert [len(c) for c in chunks] == [7] * 8 + [4] and [a for c in chunks for a in c.tags.download()] == areas


def test_a_batch_without_tags_writes_the_same_file(tmp_path):
    batch = Bw.batch_file()
    dev = device_batch(*batch)
    a, b = str(tmp_path / "a.bam"), str(tmp_path / "b.bam")
    dev.to_bam(a, block_bytes=30000)
    raw = gzip.decompress(open(a, "rb").read())
    assert raw == Bw.header_bytes() + Bw.expected_records(*batch)
    from sarlacc_amd.tags import DeviceTags
    dev.tags = DeviceTags.empty(len(dev))
    dev.to_bam(b, block_bytes=30000)
    assert gzip.decompress(open(b, "rb").read()) == raw


def test_stream_bam_keeps_tags_aligned_with_names(tmp_path):
    from sarlacc_amd.resident import DeviceReads
    text = B.sam_text(np.random.default_rng(51), 400, seqlen=60)
    path = str(tmp_path / "m.bam")
    open(path, "wb").write(B.bam_file(text, block=3000))
    want = []
    for ln in B.split_sam(text)[3]:
        f = ln.decode().split("\t")
        if not int(f[1]) & 0x900:
            want.append((f[0], b"".join(B.encode_tag(t) for t in f[11:])))
    assert 50 < len(want) < 400 and any(a for _, a in want) and any(not a for _, a in want)
    for number, block_bytes in ((7, 4000), (64, 9000), (1000, 4000)):
        got = [(nm, a) for c in DeviceReads.stream_bam(path, number, block_bytes=block_bytes, keep_tags=True)
               for nm, a in zip(c.names.tolist(), c.tags.download())]
        assert got == want
    whole = DeviceReads.from_bam(path, keep_tags=True)
    assert list(zip(whole.names.tolist(), whole.tags.download())) == want
    vals, present = whole.tag("NM")
    assert np.array_equal(vals, T.int_values([a for _, a in want], b"NM")[0]) and np.array_equal(present, [b"NM" in a for _, a in want])
    keep_all = DeviceReads.from_bam(path, exclude_flags=0, keep_tags=True)
    assert len(keep_all) == 400 and len(keep_all.tags) == 400


def test_a_file_with_malformed_tags_fails_at_ingest(tmp_path):
    from sarlacc_amd.resident import DeviceReads
    recs = [Bw.record(b"r%d" % k, b"ACGT", b"IIII") for k in range(5)]
    bad = T.record(b"bad", b"ACGT", b"IIII", BAD["no NUL"])
    path = str(tmp_path / "bad.bam")
    from tests.bgzf_cases import bgzf_compress
    open(path, "wb").write(bgzf_compress(Bw.header_bytes() + b"".join(recs[:3] + [bad] + recs[3:])))
    assert len(DeviceReads.from_bam(path)) == 6        # without tags nobody looks
    with pytest.raises(_lib().SarlaccError, match="read 4: malformed tags"):
        DeviceReads.from_bam(path, keep_tags=True)


def test_realize_keeps_each_reads_tags():
    dev, batch, areas = tagged_batch()
    rng = np.random.default_rng(61)
    idx = rng.permutation(60)[:45]
    lens = np.array([len(batch[1][i]) for i in idx])
    rev = rng.random(45) < 0.5
    ts = np.minimum(np.maximum(lens // 4, 1), np.maximum(lens, 1)).astype(np.int32)
    te = np.maximum(lens - lens // 5, 0).astype(np.int32)
    out = dev.realize(idx, rev, ts, te)
    assert out.tags.download() == [areas[i] for i in idx] and len(out) == 45
    plain = device_batch(*batch).realize(idx, rev, ts, te)
    assert plain.tags is None and plain.download()[0].to_strings() == out.download()[0].to_strings()
    for other in (dev.scramble(3), dev.front_and_back(10)[0]):
        assert other.tags is None


def test_tag_set_tag_and_drop_tags():
    from sarlacc_amd.strset import StrList
    dev, batch, areas = tagged_batch()
    n = len(dev)
    vals, present = dev.tag("fn")        # (fn, rn and sv are tags of basecaller_aux alone: one type each)
    want = T.string_values(areas, b"fn")
    assert isinstance(vals, StrList) and vals.tolist() == [v.decode() for v in want[0]] and np.array_equal(present, want[1])
    assert 15 <= present.sum() < n
    vals, present = dev.tag("rn")
    want = T.int_values(areas, b"rn")
    assert vals.dtype == np.int64 and np.array_equal(vals, want[0]) and np.array_equal(present, want[1]) and vals.max() > 50
    vals, present = dev.tag("zz")
    assert vals.tolist() == [""] * n and not present.any()
    plain = device_batch(*batch)
    vals, present = plain.tag("RX")
    assert vals.tolist() == [""] * n and not present.any() and plain.tags is None
    mv = next(k for k, a in enumerate(areas) if T.find(a, b"mv")[0] == ord("B")) + 1
    with pytest.raises(_lib().SarlaccError, match="tag mv has type B on read %d: float and array values are not decoded" % mv):
        dev.tag("mv")
    # set_tag: UMIs as RX:Z on the reads that have one, a count as an i tag, on a batch with tags and on one without
    umis = ["ACGT"[k % 4] * (k % 9) for k in range(n)]
    mask = np.array([k % 3 != 0 for k in range(n)])
    count = np.arange(n) * 40000 - 2 ** 31
    for d, before in ((dev, areas), (plain, [b""] * n)):
        d.set_tag("RX", umis, mask)
        after = T.set_tag(before, b"RX", "Z", [u.encode() for u in umis], mask)
        assert d.tags.download() == after
        d.set_tag("RX", StrList(umis[::-1]))                       # replaced where it is, appended where not
        after = T.set_tag(after, b"RX", "Z", [u.encode() for u in umis[::-1]])
        d.set_tag("xc", count)
        after = T.set_tag(after, b"xc", "i", count.tolist())
        assert d.tags.download() == after
        assert d.tag("RX")[0].tolist() == umis[::-1] and np.array_equal(d.tag("xc")[0], count) and d.tag("xc")[1].all()
        d.drop_tags(["MM", "ML", "mv", "zz"])
        after = T.drop_tag(T.drop_tag(T.drop_tag(after, b"MM"), b"ML"), b"mv")
        assert d.tags.download() == after
        d.drop_tags("RX")
        assert d.tags.download() == T.drop_tag(after, b"RX") and not d.tag("RX")[1].any()
    mixed = device_batch([b"a", b"b"], [b"A", b"C"], [b"I", b"I"])
    from sarlacc_amd.tags import DeviceTags
    mixed.tags = DeviceTags.upload([b"RXZAC\0", b"RXC\x05"])
    with pytest.raises(_lib().SarlaccError, match="read 2: tag RX has type C"):
        mixed.tag("RX")


def test_read_bam_and_write_bam_with_tags(tmp_path):
    from sarlacc_amd import generics as G
    names, seqs, quals = Bw.batch_forty()
    reads = G.Reads([s.decode() for s in seqs], [q.decode() for q in quals], [nm.decode() for nm in names])
    umis = ["ACGTAC"[:k % 7] for k in range(40)]
    path = str(tmp_path / "w.bam")
    G.write_bam(path, reads, tags={"RX": umis, "xn": (np.arange(40), np.arange(40) % 2 == 0)})
    areas = T.set_tag(T.set_tag([b""] * 40, b"RX", "Z", [u.encode() for u in umis]), b"xn", "i", list(range(40)), [k % 2 == 0 for k in range(40)])
    assert gzip.decompress(open(path, "rb").read()) == Bw.header_bytes() + b"".join(T.record_list(names, seqs, quals, areas))
    back, tags = G.read_bam(path, tags=("RX", "xn", "zz"))
    assert back.seq.to_strings() == reads.seq.to_strings() and tags["RX"][0].tolist() == umis and tags["RX"][1].all()
    assert tags["xn"][0].tolist() == [k if k % 2 == 0 else 0 for k in range(40)] and tags["xn"][1].tolist() == [k % 2 == 0 for k in range(40)]
    assert not tags["zz"][1].any()
    assert isinstance(G.read_bam(path), G.Reads)


def test_realize_reads_resident_keeps_tags(tmp_path):
    from sarlacc_amd import generics as G
    dev, batch, areas = tagged_batch("forty")
    path = str(tmp_path / "r.bam")
    dev.to_bam(path)
    names = [Bw.qname(nm).decode() for nm in batch[0]]
    for pick in ([2, 5, 17, 31, 38], [31, 2, 38, 5, 17]):      # in file order (one part, as it is) and not
        aligned = {"names": [names[i] for i in pick], "reversed": np.array([True, False, False, True, False]),
                   "metadata": {"filepath": path, "qual.type": "phred"}}
        for number in (1e5, 7):
            out = G.realizeReads(aligned, number=number, trim=False, resident=True, keep_tags=True)
            assert out.names == aligned["names"] and out.tags.download() == [areas[i] for i in pick]
            assert np.array_equal(np.diff(out.off_host), [len(batch[1][i]) for i in pick])
        assert G.realizeReads(aligned, trim=False, resident=True).tags is None


def test_an_empty_selection_of_a_tagged_batch(tmp_path):
    from sarlacc_amd import generics as G
    dev, batch, areas = tagged_batch("forty")
    none = dev.tags.take([])
    assert len(none) == 0 and none.total == 0 and none.download() == [] and none.off_host.tolist() == [0]
    out = dev.realize([], [])
    assert len(out) == 0 and len(out.tags) == 0 and out.tags.download() == []
    plain = device_batch(*batch).realize([], [])
    assert len(plain) == 0 and plain.tags is None
    # the call itself: nothing to write is no error, with or without src, whatever the source holds
    A = Areas(areas)
    for d_src in (None, A.off):
        _lib().check(_lib().lib().sarlacc_dev_bam_tags_splice(A.aux, A.off, A.n, d_src, 0, None, None, None, 0, None, None, None, None,
                                                              A.off, A.aux, None))
    path = str(tmp_path / "r.bam")
    dev.to_bam(path)
    aligned = {"names": [], "reversed": np.zeros(0, bool), "metadata": {"filepath": path, "qual.type": "phred"}}
    got = G.realizeReads(aligned, trim=False, resident=True, keep_tags=True)
    assert len(got) == 0 and len(got.tags) == 0
    assert G.realizeReads(aligned, trim=False, resident=True).tags is None
