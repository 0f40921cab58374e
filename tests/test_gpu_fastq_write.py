"""Device FASTQ writer (DeviceReads.fastq_text / .to_fastq, sarlacc_dev_fastq_format_size / _format): the text formatted
on the GPU against the host loop of generics.write_fastq on host Reads, or against a literal.  Byte work: every
comparison is byte for byte, and the expected text never comes from the code under test."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

A1 = "ACGATCAGC" + "N" * 12 + "GTCAGTCAG"
A2 = "CACACTGAGCAGCGACTAGACA"
_BASES = np.frombuffer(b"ACGTN", dtype=np.uint8)
_NAME_CHARS = np.frombuffer(b"abcXYZ019 /_:=.", dtype=np.uint8)


def draw(rng, lengths, name_lengths=None):
    """(names, seqs, quals) as lists of str: one read per length; names "read_<i> some description/<i>" or, with
    name_lengths, of exactly those lengths (spaces and '/' among their characters)."""
    names, seqs, quals = [], [], []
    for i, L in enumerate(lengths):
        L = int(L)
        seqs.append(_BASES[rng.choice(5, L, p=[0.24, 0.24, 0.24, 0.24, 0.04])].tobytes().decode())
        quals.append(rng.integers(33, 127, L).astype(np.uint8).tobytes().decode())
        if name_lengths is None:
            names.append("read_%d some description/%d" % (i + 1, i))
        else:
            names.append(_NAME_CHARS[rng.integers(0, _NAME_CHARS.size, int(name_lengths[i]))].tobytes().decode())
    return names, seqs, quals


def fastq_text(names, seqs, quals, eol="\n", lower=False, final_eol=True):
    recs = ["@%s%s%s%s+%s%s" % (nm, eol, s.lower() if lower and i % 3 == 0 else s, eol, eol, q)
            for i, (nm, s, q) in enumerate(zip(names, seqs, quals))]
    return (eol.join(recs) + (eol if final_eol and recs else "")).encode()


def host_text(tmp_path, reads, tag="host"):
    """What the host loop of generics.write_fastq writes for host Reads."""
    from sarlacc_amd import generics as G
    assert isinstance(reads, G.Reads)
    path = tmp_path / ("%s.fastq" % tag)
    G.write_fastq(str(path), reads)
    return path.read_bytes()


def resident(reads):
    from sarlacc_amd.resident import DeviceReads
    dev = DeviceReads.upload(reads)
    dev.names = reads.names
    return dev


def abi_text(dev, first_index, first=0, count=None, shift=0, names=(None, None)):
    """Text of records [first, first + count) straight through the C ABI, written `shift` bytes into a buffer (so that the
    destination is not 16-byte aligned), with default names or with `names` (device buffers of the name bytes and their
    offsets); also returns the record offsets."""
    from sarlacc_amd import _lib
    from sarlacc_amd._lib import check
    from sarlacc_amd.resident import DevBuffer
    lib, n = _lib.lib(), len(dev)
    count = n - first if count is None else count
    rec_off, total = DevBuffer(8 * (n + 1)), C.c_int64(-1)
    names, name_off = (b and b.ptr for b in names)
    check(lib.sarlacc_dev_fastq_format_size(dev.off.ptr, C.c_int64(n), names, name_off, C.c_int64(first_index), rec_off.ptr,
                                            C.byref(total), None))
    ro = rec_off.to_numpy(np.int64, n + 1)
    assert total.value == ro[-1]
    nbytes = int(ro[first + count] - ro[first])
    guard = np.full(nbytes + shift + 32, 0xEE, np.uint8)
    d_text = DevBuffer.from_numpy(guard)
    check(lib.sarlacc_dev_fastq_format(dev.seq.ptr, dev.qual.ptr, dev.off.ptr, names, name_off, C.c_int64(first_index), rec_off.ptr,
                                       C.c_int64(first), C.c_int64(count), C.c_void_p(d_text.ptr.value + shift), None))
    got = d_text.to_numpy(np.uint8, guard.size)
    assert (got[:shift] == 0xEE).all() and (got[shift + nbytes:] == 0xEE).all(), "bytes written outside the range"
    return got[shift:shift + nbytes].tobytes(), ro


def test_identity_with_the_host_writer(tmp_path):
    """300 records of 0 - 700 bases, names with spaces and '/': once uploaded from Reads with a list of names, once parsed
    from text on the device (names: the device-extracted StrList)."""
    from sarlacc_amd import generics as G
    from sarlacc_amd.resident import DeviceReads
    from sarlacc_amd.strset import StrList
    rng = np.random.default_rng(11)
    names, seqs, quals = draw(rng, rng.integers(0, 701, 300))
    assert min(map(len, seqs)) == 0
    reads = G.Reads(seqs, quals, names)
    want = host_text(tmp_path, reads)
    dev = resident(reads)
    assert isinstance(dev.names, list)
    assert dev.fastq_text() == want
    path = tmp_path / "dev.fastq"
    assert dev.to_fastq(str(path)) == len(want) and path.read_bytes() == want
    parsed = DeviceReads.from_fastq(fastq_text(names, seqs, quals))
    assert isinstance(parsed.names, StrList)
    assert parsed.fastq_text() == want
    assert G.write_fastq(str(path), parsed) == len(want) and path.read_bytes() == want


def test_default_names(tmp_path):
    """names = None: READ_<i>, 1-based and unpadded, across 9/10, 99/100 and 999/1000; through the C ABI also numbered
    from 999 999 998, which crosses from 9 to 10 digits."""
    from sarlacc_amd import generics as G
    from sarlacc_amd.resident import DeviceReads
    rng = np.random.default_rng(12)
    _, seqs, quals = draw(rng, rng.integers(0, 41, 1005))
    reads = G.Reads(seqs, quals)
    want = host_text(tmp_path, reads)
    assert b"@READ_9\n" in want and b"@READ_10\n" in want and b"@READ_1000\n" in want and b"@READ_1005\n" in want
    dev = DeviceReads.upload(reads)
    assert dev.names is None
    assert dev.fastq_text() == want
    path = tmp_path / "dev.fastq"
    assert dev.to_fastq(str(path), block_bytes=1000) == len(want) and path.read_bytes() == want
    got, _ = abi_text(dev, 1)
    assert got == want
    start = 999999998
    literal = b"".join(b"@READ_%d\n%s\n+\n%s\n" % (start + i, s.encode(), q.encode()) for i, (s, q) in enumerate(zip(seqs, quals)))
    assert b"@READ_999999999\n" in literal and b"@READ_1000000000\n" in literal
    got, ro = abi_text(dev, start)
    assert got == literal
    # a range of records, into a destination that is not 16-byte aligned
    got, _ = abi_text(dev, start, first=1, count=700, shift=5)
    assert got == literal[int(ro[1]):int(ro[701])]


def test_given_names_at_every_record_boundary_and_misalignment(tmp_path):
    """40 records of 0 - 70 bases with given names of 0 - 40 bytes, through the C ABI into a guarded buffer: the whole
    batch at every misalignment 0 .. 15 of the destination, and split at every record boundary with both parts misaligned
    (with default names a piece never lies inside a name, and only test_default_names misaligns the destination).  The
    expected bytes are the host writer's."""
    from sarlacc_amd import generics as G
    from sarlacc_amd.resident import DevBuffer, DeviceReads
    from sarlacc_amd.strset import StringSet
    rng = np.random.default_rng(23)
    lengths, name_lengths = rng.integers(0, 71, 40), rng.integers(0, 41, 40)
    lengths[[3, 20]], name_lengths[[3, 21]] = (0, 70), (0, 40)
    names, seqs, quals = draw(rng, lengths, name_lengths)
    reads = G.Reads(seqs, quals, names)
    want = host_text(tmp_path, reads)
    ss = StringSet.from_strings(names)
    dev, given = DeviceReads.upload(reads), (DevBuffer.from_numpy(ss.chars), DevBuffer.from_numpy(ss.off))
    for shift in range(16):
        assert abi_text(dev, 1, shift=shift, names=given)[0] == want, "misaligned by %d" % shift
    for k in range(1, 40):
        got = abi_text(dev, 1, 0, k, shift=k % 16, names=given)[0] + abi_text(dev, 1, k, 40 - k, shift=(3 * k) % 16, names=given)[0]
        assert got == want, "split at record %d" % k
    assert b"".join(abi_text(dev, 1, k, 1, shift=(5 * k) % 16, names=given)[0] for k in range(40)) == want


def test_round_trip(tmp_path):
    from sarlacc_amd import generics as G
    from sarlacc_amd.resident import DeviceReads
    rng = np.random.default_rng(13)
    names, seqs, quals = draw(rng, rng.integers(0, 701, 300))
    text = fastq_text(names, seqs, quals)
    assert DeviceReads.from_fastq(text).fastq_text() == text
    crlf = tmp_path / "crlf.fastq"
    crlf.write_bytes(fastq_text(names, seqs, quals, eol="\r\n", lower=True))
    want = host_text(tmp_path, G.read_fastq(str(crlf)))
    assert b"\r" not in want and want == text
    assert DeviceReads.from_fastq(str(crlf)).fastq_text() == want


@pytest.fixture(scope="module")
def mixed(tmp_path_factory):
    """40 records of 5 000 - 30 000 bases, one of 70 000 (beyond 65 535) and records of 1, 15, 16, 17, 63, 64 and 65 bases
    (head and tail handling meets every alignment), names of 1 - 40 characters in front so that the destination alignment
    changes from record to record: (Reads, the host writer's text)."""
    from sarlacc_amd import generics as G
    rng = np.random.default_rng(14)
    lengths = np.concatenate([rng.integers(5000, 30001, 40), [70000], [1, 15, 16, 17, 63, 64, 65]])
    lengths = lengths[rng.permutation(lengths.size)]
    names, seqs, quals = draw(rng, lengths, 1 + np.arange(lengths.size) % 40)
    reads = G.Reads(seqs, quals, names)
    return reads, host_text(tmp_path_factory.mktemp("mixed"), reads)


def test_long_and_mixed_lengths(mixed):
    reads, want = mixed
    assert int(reads.width().max()) == 70000 and len(reads) == 48
    assert resident(reads).fastq_text() == want


def test_blocks(mixed, tmp_path):
    """block_bytes below one long record, between, and the default give the same file; append keeps what is there."""
    reads, want = mixed
    dev = resident(reads)
    path = tmp_path / "blocks.fastq"
    for block_bytes in (4096, 100000):
        assert dev.to_fastq(str(path), block_bytes=block_bytes) == len(want)
        assert path.read_bytes() == want, block_bytes
        assert dev.fastq_text(block_bytes=block_bytes) == want
    assert dev.to_fastq(str(path)) == len(want) and path.read_bytes() == want
    before = b"@x\nAC\n+\nII\n"
    path.write_bytes(before)
    assert dev.to_fastq(str(path), append=True, block_bytes=100000) == len(want)
    assert path.read_bytes() == before + want


def test_empty_cases(tmp_path):
    from sarlacc_amd import generics as G
    from sarlacc_amd.resident import DeviceReads
    path = tmp_path / "empty.fastq"
    for dev in (DeviceReads.upload(G.Reads([], [])), DeviceReads.from_fastq(b"")):
        path.write_bytes(b"old")
        assert len(dev) == 0 and dev.to_fastq(str(path)) == 0 and path.read_bytes() == b""
        assert dev.fastq_text() == b""
    names = ["a", "b c", "read/3"]
    dev = resident(G.Reads(["", "", ""], ["", "", ""], names))
    want = b"@a\n\n+\n\n@b c\n\n+\n\n@read/3\n\n+\n\n"
    assert dev.fastq_text() == want
    assert dev.to_fastq(str(path)) == len(want) and path.read_bytes() == want


def test_other_encodings(tmp_path):
    """Quality bytes are copied, not interpreted: a table whose names lie at and above byte 128, and the same text whatever
    `encoding` says."""
    from sarlacc_amd import generics as G
    from sarlacc_amd.encoding import phred_encoding
    from tests.encodings import BY_NAME, draw_quals
    table = BY_NAME["n128_high"]
    rng = np.random.default_rng(17)
    lengths = rng.integers(0, 201, 60)
    names, seqs, _ = draw(rng, lengths)
    quals = draw_quals(table, lengths, 17)
    flat = np.frombuffer(b"".join(quals), dtype=np.uint8)
    assert (flat >= 128).any() and flat.max() == 255 and not np.isin(flat, (10, 13)).any()
    want = b"".join(b"@" + nm.encode() + b"\n" + s.encode() + b"\n+\n" + q + b"\n" for nm, s, q in zip(names, seqs, quals))
    dev = resident(G.Reads(seqs, quals, names, encoding=table.enc))
    path = tmp_path / "high.fastq"
    for enc in (table.enc, None, phred_encoding()):
        dev.encoding = enc
        assert dev.fastq_text() == want
        assert dev.to_fastq(str(path)) == len(want) and path.read_bytes() == want


def test_realize_reads_to_fastq(tmp_path):
    """FASTQ -> device -> oriented and trimmed -> FASTQ: write_fastq of realizeReads(resident=True) writes the file that
    write_fastq of the host Reads of realizeReads writes, for one chunk and for several."""
    from sarlacc_amd import generics as G
    from sarlacc_amd.mock import mock_reads
    from sarlacc_amd.resident import DeviceReads
    sim = mock_reads(A1, A2, nmolecules=15, nreads=6, seqlen=300, seed=7)
    reads = G.Reads(sim["reads"], sim["quals"], ["READ_%d" % (i + 1) for i in range(len(sim["reads"]))])
    src = tmp_path / "mock.fastq"
    G.write_fastq(str(src), reads)
    filt = G.filterReads(G.adaptorAlign(A1, A2, str(src), tolerance=120), 6, 6)
    rev = np.asarray(filt["reversed"], dtype=bool)
    assert rev.any() and not rev.all() and (np.asarray(filt["trim.start"]) > 1).any()
    for number in (1e5, 25):
        assert (number < len(reads)) == (number == 25)
        p1, p2 = tmp_path / ("dev_%d.fastq" % number), tmp_path / ("host_%d.fastq" % number)
        res = G.realizeReads(filt, number=number, resident=True)
        assert isinstance(res, DeviceReads)
        written = G.write_fastq(str(p1), res)
        G.write_fastq(str(p2), G.realizeReads(filt, number=number))
        want = p2.read_bytes()
        assert want.count(b"\n") == 4 * len(filt["names"]) > 0
        assert p1.read_bytes() == want and written == len(want)


def test_refusal(tmp_path):
    """A name with a line break cannot be read back: the lowest such record is the error, and nothing is written."""
    from sarlacc_amd import generics as G
    from sarlacc_amd._lib import SarlaccError
    rng = np.random.default_rng(19)
    names, seqs, quals = draw(rng, rng.integers(0, 50, 10))
    names[2], names[6] = "a\nb", "x\ry"
    dev = resident(G.Reads(seqs, quals, names))
    path = tmp_path / "bad.fastq"
    with pytest.raises(SarlaccError, match="record 3: read name holds a line break"):
        dev.to_fastq(str(path))
    assert not path.exists()
    path.write_bytes(b"@x\nAC\n+\nII\n")
    with pytest.raises(SarlaccError, match="record 3: read name holds a line break"):
        dev.to_fastq(str(path), append=True)
    assert path.read_bytes() == b"@x\nAC\n+\nII\n"
    with pytest.raises(SarlaccError, match="record 3: read name holds a line break"):
        dev.fastq_text()
    dev.names = names[:6] + ["x\ry"] + names[7:]
    dev.names[2] = "ab"
    with pytest.raises(SarlaccError, match="record 7: read name holds a line break"):
        dev.fastq_text()


def test_host_plan_agrees_with_the_size_pass(mixed):
    """The host plans the blocks from the lengths it already has; the device formats from the offsets of its size pass.
    The two must be the same numbers, for given names and for the default ones."""
    from sarlacc_amd import generics as G
    from sarlacc_amd.resident import DeviceReads
    reads, _ = mixed
    rng = np.random.default_rng(21)
    _, seqs, quals = draw(rng, rng.integers(0, 41, 1005))
    for dev in (resident(reads), DeviceReads.upload(G.Reads(seqs, quals))):
        plan = dev._write_plan(100000)
        rec_off, ro, ranges = plan.rec_off, plan.ro, plan.ranges
        assert np.array_equal(rec_off.to_numpy(np.int64, len(dev) + 1), ro)
        assert ranges[0][0] == 0 and ranges[-1][1] == len(dev) and all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))
        assert all(ro[b] - ro[a] <= 100000 or b == a + 1 for a, b in ranges)
