"""What the four readers share (readers_host.cpp, text_lines.hip): the k-th newline of sarlacc_dev_fastq_split at the
edges of a tile and of a thread's slot, the one line index under FASTQ's two and SAM's one end sentinel, and the index
state of every reader after the workspaces were released or another buffer was indexed -- an error return, never a
launch over stale arrays.  Byte work: everything must be identical."""
import ctypes as C

import numpy as np
import pytest

from tests import bam_cases as B
from tests import bam_reads_cases as RC
from tests import sam_restated as R

pytestmark = pytest.mark.gpu

TILE, SLOT = 8192, 32          # FQ_TILE, FQ_PER_THREAD of text_lines.hpp


def _lib():
    from sarlacc_amd import _lib
    return _lib.lib()


def _dev(data, shift=0):
    """bytes -> (device buffer, address of byte 0 of the data): `shift` bytes of padding in front misalign the text."""
    from sarlacc_amd.resident import DevBuffer
    buf = DevBuffer.from_numpy(np.frombuffer(b"#" * shift + bytes(data) + b"#", np.uint8))
    return buf, buf.ptr.value + shift


# ---- 1. sarlacc_dev_fastq_split at the tile's edges ----------------------------------------------------------------------

def record_of(rng, nbytes, i):
    """One FASTQ record of exactly nbytes >= 8 bytes, final newline included: '@' name, bases, '+', qualities."""
    name = b"r" if nbytes % 2 else b"r%d" % (i % 10)      # 2 L + len(name) + 6 bytes
    L = (nbytes - 6 - len(name)) // 2
    seq = "".join(rng.choice(list("ACGTNacgt"), L)).encode()
    qual = bytes(rng.integers(33, 127, L).astype(np.uint8))
    rec = b"@" + name + b"\n" + seq + b"\n+\n" + qual + b"\n"
    assert len(rec) == nbytes
    return rec


def text_with_newline_at(rng, at, k, tail):
    """FASTQ text whose 4 k-th newline is byte `at`, followed by `tail` further records."""
    sizes = [int(s) for s in rng.integers(8, max(9, min(400, (at + 1) // k - 8)), k - 1)]
    sizes.append(at + 1 - sum(sizes))
    text = b"".join(record_of(rng, s, i) for i, s in enumerate(sizes + [int(s) for s in rng.integers(8, 300, tail)]))
    assert text[at:at + 1] == b"\n" and text[:at + 1].count(b"\n") == 4 * k
    return text


# (byte of the 4 k-th newline, k, records behind it)
SPLIT_EDGES = {
    "tile0_last_byte": (TILE - 1, 7, 30), "tile1_first_byte": (TILE, 7, 30),
    "slot_last_byte": (TILE + 5 * SLOT + SLOT - 1, 9, 30), "next_slot_first_byte": (TILE + 6 * SLOT, 9, 30),
    "slot_last_byte_tile0": (7 * SLOT + SLOT - 1, 2, 40), "text_last_byte": (10000, 11, 0),
    "text_of_one_tile": (TILE - 1, 6, 0), "text_of_two_tiles": (2 * TILE - 1, 13, 0),
}


@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("edge", sorted(SPLIT_EDGES))
def test_fastq_split_at_tile_and_slot_edges(tmp_path, edge, shift):
    from sarlacc_amd._lib import check
    from sarlacc_amd.generics import read_fastq
    from sarlacc_amd.resident import DeviceReads
    at, k, tail = SPLIT_EDGES[edge]
    text = text_with_newline_at(np.random.default_rng(at + k), at, k, tail)
    if tail == 0:
        assert len(text) == at + 1
    newlines = np.flatnonzero(np.frombuffer(text, np.uint8) == 10)
    buf, address = _dev(text, shift)
    for max_records in (1, k, k + tail + 5):
        n, used = C.c_int64(-1), C.c_int64(-1)
        check(_lib().sarlacc_dev_fastq_split(address, len(text), max_records, C.byref(n), C.byref(used), None))
        want_n = min(len(newlines) // 4, max_records)
        assert (n.value, used.value) == (want_n, int(newlines[4 * want_n - 1]) + 1)
        if max_records == k:
            assert used.value == at + 1
        path = tmp_path / ("r%d.fastq" % max_records)
        path.write_bytes(text[:used.value])
        host = read_fastq(str(path))
        dev = DeviceReads._from_device_text(address, used.value, None)
        seq, qual = dev.download()
        assert len(dev) == len(host) == want_n
        assert seq.to_strings() == host.seq.to_strings() and qual.to_strings() == host.qual.to_strings()
        assert dev.names == host.names


# ---- 2. one line index, two sentinel counts --------------------------------------------------------------------------------

SAM_HEAD = "@HD\tVN:1.6\n@SQ\tSN:chr1\tLN:100000\n"
SAM_REST = "\t16\tchr1\t%d\t60\t3S10M2D5M4H\t*\t0\t0\tACGT\t!!!!"


def line_lengths(total):
    """Lengths (a, b, c, b) of the four lines of each record, newlines not counted, that add up with one newline per
    line to `total` bytes: lines of 48 to 700 bytes, so line ends fall on both sides of tile and slot edges."""
    rng = np.random.default_rng(total)
    lens, left = [], total
    while True:
        a, b, c = (int(x) for x in rng.integers(48, 700, 3))
        size = a + 2 * b + c + 4
        if left - size < 200:       # the last record takes what is left, in its header line
            a, b, c = left - 4 - 2 * 50 - 48, 50, 48
            lens += [a, b, c, b]
            assert a >= 48 and sum(lens) + len(lens) == total
            return lens
        lens += [a, b, c, b]
        left -= size


def fastq_of(lens):
    rng = np.random.default_rng(len(lens))
    out = []
    for i in range(0, len(lens), 4):
        a, b, c = lens[i:i + 3]
        out += [b"@" + b"n" * (a - 1), "".join(rng.choice(list("ACGTN"), b)).encode(), b"+" + b"p" * (c - 1),
                bytes(rng.integers(33, 127, b).astype(np.uint8))]
    return b"".join(ln + b"\n" for ln in out)


def sam_of(lens):
    out = []
    for i, n in enumerate(lens):
        rest = SAM_REST % (i + 1)
        assert n > len(rest)
        out.append("q" * (n - len(rest)) + rest)
    return "".join(ln + "\n" for ln in out).encode()


@pytest.mark.parametrize("total", [TILE - 1, TILE, TILE + 1, 3 * TILE])
def test_one_line_index_under_two_and_one_end_sentinels(tmp_path, total):
    from sarlacc_amd import sam
    from sarlacc_amd.generics import read_fastq
    from sarlacc_amd.resident import DeviceReads
    from sarlacc_amd.strset import StrList
    lens = line_lengths(total)
    fq, body = fastq_of(lens), sam_of(lens)
    assert len(fq) == len(body) == total
    assert np.array_equal(np.flatnonzero(np.frombuffer(fq, np.uint8) == 10), np.flatnonzero(np.frombuffer(body, np.uint8) == 10))
    # FASTQ: the device sees `size` bytes; the host reader gets the same bytes as a file
    path = tmp_path / "r.fastq"
    path.write_bytes(fq)
    host = read_fastq(str(path))
    assert len(host) == len(lens) // 4
    buf, address = _dev(fq + b"\n\r\n\n")
    for size in (total, total - 1, total + 1, total + 4):      # as it is, without the final newline, with blank lines
        dev = DeviceReads._from_device_text(address, size, None)
        seq, qual = dev.download()
        assert seq.to_strings() == host.seq.to_strings() and qual.to_strings() == host.qual.to_strings()
        assert dev.names == host.names
    # SAM body: with and without the final newline
    want = R.as_table(R.sam2ranges(SAM_HEAD.encode() + body, 10, None))
    assert len(want["start"]) == len(lens)
    names, lengths = sam.parse_header([ln.encode() for ln in SAM_HEAD.split("\n")[:-1]])
    sbuf, saddress = _dev(body)
    for size in (total, total - 1):
        nlines, cols = sam._parse_block(saddress, size, 3, sam._Tables(names, None), True, 10)
        ref, start, width, lclip, rclip, strand, qn = cols
        got = {"seqnames": ref, "start": start, "end": start.astype(np.int64) + width - 1, "width": width,
               "strand": strand.view("S1").astype("<U1"), "left.clip": lclip, "right.clip": rclip, "names": StrList(qn),
               "seqinfo": {"seqnames": list(names), "seqlengths": lengths}}
        assert nlines == len(lens)
        assert R.as_table(got) == want


# ---- 3. a stale index is an error return ------------------------------------------------------------------------------------

PATTERN = 0xA5
NO_FASTQ = "sarlacc_dev_fastq_extract without a matching sarlacc_dev_fastq_index"
NO_SAM = "sarlacc_dev_sam_extract without a matching sarlacc_dev_sam_index"
NO_BAMR = "no BAM reads index on this thread"
OTHER_BAM = "not the BAM buffer indexed last on this thread"


class Outputs:
    """Device buffers for a step's outputs, filled with a pattern: a refused step must leave every byte of them alone."""

    def __init__(self, *sizes):
        from sarlacc_amd.resident import DevBuffer
        self.sizes = [max(int(s), 1) + 16 for s in sizes]
        self.bufs = [DevBuffer.from_numpy(np.full(s, PATTERN, np.uint8)) for s in self.sizes]

    def untouched(self):
        return all((b.to_numpy(np.uint8, s) == PATTERN).all() for b, s in zip(self.bufs, self.sizes))

    def bytes(self):
        return [b.to_numpy(np.uint8, s).tobytes() for b, s in zip(self.bufs, self.sizes)]


class Numbers:
    """The same for a step whose outputs are int64 values on the host."""

    def __init__(self, n):
        self.vals = [C.c_int64(-7) for _ in range(n)]

    def untouched(self):
        return all(v.value == -7 for v in self.vals)

    def bytes(self):
        return [v.value for v in self.vals]


class FastqPair:
    missing = other = NO_FASTQ

    def __init__(self, seed):
        rng = np.random.default_rng(seed)
        recs = [record_of(rng, int(s), i) for i, s in enumerate(rng.integers(8, 200, 25))]
        self.text = b"".join(recs)
        self.buf, self.address = _dev(self.text)

    def index(self):
        n, tb, tn = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        assert _lib().sarlacc_dev_fastq_index(self.address, len(self.text), C.byref(n), C.byref(tb), C.byref(tn), None) == 0
        self.sizes = (tb.value, tb.value, 8 * (n.value + 1), tn.value, 8 * (n.value + 1))

    def steps(self):
        def extract():
            out = Outputs(*self.sizes)
            return _lib().sarlacc_dev_fastq_extract(self.address, *out.bufs, None), out
        return {"extract": extract}


class SamPair:
    missing = other = NO_SAM

    def __init__(self, seed):
        from sarlacc_amd import sam
        text = B.sam_text(np.random.default_rng(seed), 30)
        head = B.header().encode()
        self.body = text[len(head):]
        names, _ = sam.parse_header([ln for ln in head.split(b"\n")[:-1]])
        self.tables = sam._Tables(names, None)
        self.buf, self.address = _dev(self.body)

    def index(self):
        t = self.tables
        nl, nk, nb = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        assert _lib().sarlacc_dev_sam_index(self.address, len(self.body), 1, t.ref, t.ref_off, t.n_ref, t.mask, t.extra, t.extra_off,
                                            t.n_extra, 1, 10, C.byref(nl), C.byref(nk), C.byref(nb), None) == 0
        assert nk.value > 0
        self.nk, self.nb = nk.value, nb.value

    extract_name = "sarlacc_dev_sam_extract"

    def steps(self):
        def extract():
            n = self.nk
            out = Outputs(4 * n, 4 * n, 4 * n, n, 4 * n, 4 * n, self.nb, 8 * (n + 1))
            return getattr(_lib(), self.extract_name)(self.address, *out.bufs, None), out
        return {"extract": extract}


class BamPair(SamPair):
    extract_name = "sarlacc_dev_bam_extract"

    def __init__(self, seed):
        self.raw = b"".join(B.sam_to_bam(B.sam_text(np.random.default_rng(seed), 30))[1])
        self.buf, self.address = _dev(self.raw)

    def index(self):
        nrec, used, nk, nb = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)
        assert _lib().sarlacc_dev_bam_index(self.address, len(self.raw), 1, 1, len(B.REFS), None, 1, 10, C.byref(nrec), C.byref(used),
                                            C.byref(nk), C.byref(nb), None) == 0
        assert nrec.value == 30 and nk.value > 0
        self.nk, self.nb = nk.value, nb.value


class BamReadsPair:
    missing, other = NO_BAMR, OTHER_BAM
    first, count = 3, 14

    def __init__(self, seed):
        rng = np.random.default_rng(seed)
        recs = [RC.read_record(b"read%d" % i, f, rng.integers(1, 16, int(n)).tolist(), rng.integers(0, 94, int(n)).tolist(),
                               tags=(b"NMC\x03" if i % 2 else b""))
                for i, (n, f) in enumerate(zip(rng.integers(1, 300, 24), [4, 16, 0] * 8))]
        self.raw = b"".join(recs)
        self.buf, self.address = _dev(self.raw)

    def index(self):
        nrec, used, nreads = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        assert _lib().sarlacc_dev_bam_reads_index(self.address, len(self.raw), 1, 1, 0x900, C.byref(nrec), C.byref(used),
                                                  C.byref(nreads), None) == 0
        assert nreads.value == 24

    def steps(self):
        lib, first, count = _lib(), self.first, self.count

        def numbers(call, n):
            out = Numbers(n)
            return call(*[C.byref(v) for v in out.vals]), out

        def extract():
            out = Outputs(60000, 60000, 8 * (count + 1), 4000, 8 * (count + 1))
            return lib.sarlacc_dev_bam_reads_extract(self.address, first, count, 1, *out.bufs, None), out

        def aux_extract():
            out = Outputs(4000, 8 * (count + 1))
            return lib.sarlacc_dev_bam_reads_aux_extract(self.address, first, count, *out.bufs, None), out

        return {"range": lambda: numbers(lambda *v: lib.sarlacc_dev_bam_reads_range(first, count, *v), 3),
                "records": lambda: numbers(lambda *v: lib.sarlacc_dev_bam_reads_records(first, *v), 1),
                "extract": extract,
                "aux_range": lambda: numbers(lambda *v: lib.sarlacc_dev_bam_reads_aux_range(first, count, *v), 1),
                "aux_extract": aux_extract}


STEPS = [(FastqPair, "extract"), (SamPair, "extract"), (BamPair, "extract")] + \
        [(BamReadsPair, s) for s in ("range", "records", "extract", "aux_range", "aux_extract")]
STEP_IDS = ["%s-%s" % (p.__name__, s) for p, s in STEPS]


def last_error():
    return _lib().sarlacc_last_error().decode()


@pytest.mark.parametrize("pair,step", STEPS, ids=STEP_IDS)
def test_a_step_after_a_workspace_release_is_refused(pair, step):
    a = pair(1)
    a.index()
    _lib().sarlacc_release_workspace()
    rc, out = a.steps()[step]()
    assert rc != 0 and a.missing in last_error()
    assert out.untouched()
    a.index()                               # usable again
    assert a.steps()[step]()[0] == 0


# (the range, records and aux_range steps of BAM reads name no buffer: they answer for the index made last)
@pytest.mark.parametrize("pair,step", [ps for ps in STEPS if "range" not in ps[1] and ps[1] != "records"],
                         ids=[i for i in STEP_IDS if "range" not in i and "records" not in i])
def test_a_step_on_the_buffer_indexed_before_the_last_is_refused(pair, step):
    a, b = pair(1), pair(2)
    a.index()
    b.index()
    rc, out = a.steps()[step]()
    assert rc != 0 and a.other in last_error()
    assert out.untouched()


@pytest.mark.parametrize("pair,step", STEPS, ids=STEP_IDS)
def test_a_release_of_other_workspaces_leaves_the_index_alone(pair, step):
    a = pair(1)
    a.index()
    rc, out = a.steps()[step]()
    assert rc == 0
    want = out.bytes()
    a.index()
    _lib().sarlacc_release_umi_workspace()
    rc, out = a.steps()[step]()
    assert rc == 0, last_error()
    assert out.bytes() == want and not out.untouched()
