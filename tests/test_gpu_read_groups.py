"""readGroups on the device (csrc/read_groups.hip: sarlacc_dev_names_match / _records_pick / _locus_labels /
_labels_csr, sarlacc_amd/groups.py, generics.readGroups), compared exactly with tests/read_groups_cases.py, the
plain-Python restatement that tests/test_read_groups_host.py pins.  Everything is integers: no tolerance.

The name kernels take 64 bytes of a name per step of the wavefront, so the key lengths tried sit around 16, 64, 128 and
beyond; every buffer is uploaded at its exact size, the longest name last."""
import numpy as np
import pytest

from tests import read_groups_cases as G

pytestmark = pytest.mark.gpu


def _read_groups(rows, names, nref=None, **kwargs):
    from sarlacc_amd import generics
    return generics.readGroups(G.make_ranges(rows, nref), names, **kwargs)


def _check(rows, names, what, nref=None, **kwargs):
    ranges = G.make_ranges(rows, nref)
    from sarlacc_amd import generics
    got = generics.readGroups(ranges, names, **kwargs)
    G.same(got, G.expected(ranges, names, **kwargs), what)
    return got


# ---- name match ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 5000])
def test_name_match(n):
    rows, names = G.name_case(n, seed=n)
    got = _check(rows, names, "n = %d" % n, nref=7)
    _check(rows, names, "n = %d, by locus" % n, nref=7, by="locus", maxgap=1, ignore_strand=False)
    if n >= 63:
        assert (got["record"] < 0).any() and got["unmatched.records"] > 0 and got["n.records"].max() == 6


def test_name_match_takes_reads_of_every_kind():
    from sarlacc_amd import generics
    from sarlacc_amd.strset import StrList
    rows, names = G.name_case(130, seed=3)
    ranges = G.make_ranges(rows, 7)
    want = G.expected(ranges, names)
    reads = generics.Reads(["ACGT"] * len(names), ["IIII"] * len(names), names=names)
    for r in (names, StrList(names), reads):
        G.same(generics.readGroups(ranges, r), want, type(r).__name__)


@pytest.mark.parametrize("bits", [1, 2, 8])
def test_collisions_change_nothing(bits):
    """names_hash_bits keeps 1, 2 or 8 bits of the hash: every probe walks chains of unequal keys with equal tags, and
    only the byte comparison tells them apart."""
    from sarlacc_amd import calls
    cases = [G.name_case(n, seed=n) for n in (2, 65, 700)]
    default = [_read_groups(rows, names, nref=7, by="locus") for rows, names in cases]
    try:
        calls.set_option("names_hash_bits", bits)
        for (rows, names), before in zip(cases, default):
            got = _check(rows, names, "names_hash_bits = %d, n = %d" % (bits, len(names)), nref=7, by="locus")
            G.same(got, before, "names_hash_bits = %d against the default" % bits)
    finally:
        calls.set_option("names_hash_bits", 0)


# ---- duplicate keys --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("whole", [True, False], ids=["equal names", "equal after the cut"])
@pytest.mark.parametrize("copies", [2, 3, 4])
def test_duplicate_keys_are_refused(copies, whole):
    """Rule 1: (J, K) of the message are the first read of the key and the lowest read that is not the first of its key,
    whatever order the wavefronts arrive in: five runs, one message."""
    from sarlacc_amd._lib import SarlaccError
    rows, names = G.name_case(900, seed=copies)
    at = [811, 37, 480, 122][:copies]                      # a second, later duplicate pair must not win
    key = G.key_of(names[at[0]])
    for k, i in enumerate(at):
        names[i] = key if whole else key + (" copy %d" % k, "\tcopy %d" % k, "", " ")[k]
    names[899] = names[700]
    with pytest.raises(G.DuplicateKey) as want:
        G.expected(G.make_ranges(rows, 7), names)
    assert (want.value.j, want.value.k) == (sorted(at)[0] + 1, sorted(at)[1] + 1)
    for _ in range(5):
        with pytest.raises(SarlaccError) as got:
            _read_groups(rows, names, nref=7)
        assert str(got.value) == str(want.value)


# ---- pick ------------------------------------------------------------------------------------------------------------------
def test_pick():
    rows = [("r1", 0, 1, 7, "+"),
            ("r2", 1, 1, 5, "+"), ("r2", 2, 2, 5, "-"),                                # equal widths: the first wins
            ("r3", 0, 1, 1, "+"), ("r3", 1, 1, 2, "+"), ("r3", 2, 1, 3, "+"),          # the widest is last
            ("r4", 3, 9, 0, "+"), ("r4", 4, 9, 0, "+"), ("r4", 5, 9, 0, "+"), ("r4", 6, 9, 0, "+"),      # width 0
            ("r5", 0, 1, 4, "+"), ("r5", 1, 1, 9, "+"), ("r5", 2, 1, 9, "+"), ("r5", 3, 1, 2, "+"), ("r5", 4, 1, 9, "+"),
            ("r6", 6, 1, 3, "+"), ("r6", 5, 1, 3, "+"), ("r6", 4, 1, 2, "+"), ("r6", 3, 1, 3, "+"), ("r6", 2, 1, 1, "+"), ("r6", 1, 1, 3, "+")]
    names = ["r6", "r5", "r4", "r3", "r2", "r1", "r0"]
    got = _check(rows, names, "pick", nref=7)
    assert got["record"].tolist() == [15, 11, 6, 5, 1, 0, -1] and got["n.records"].tolist() == [6, 5, 4, 3, 2, 1, 0]
    back = rows[::-1]
    got = _check(back, names, "pick, rows reversed", nref=7)
    assert got["record"].tolist() == [0, 6, 11, 15, 18, 20, -1]


# ---- locus -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", G.LITERAL, ids=[c[0] for c in G.LITERAL])
def test_literal_cases(case):
    what, rows, names, kwargs, want = case
    from sarlacc_amd import generics
    G.same(generics.readGroups(G.make_ranges(rows), names, **kwargs), G.literal_expected(want), what)


@pytest.fixture(scope="module")
def locus_case():
    return G.locus_case(3000, 7, seed=1)


@pytest.mark.parametrize("ignore_strand", [True, False])
@pytest.mark.parametrize("maxgap", [0, 1, 50])
def test_locus_random_ranges(locus_case, maxgap, ignore_strand):
    rows, names = locus_case
    got = _check(rows, names, "maxgap %d, ignore_strand %s" % (maxgap, ignore_strand), nref=7, by="locus", maxgap=maxgap,
                 ignore_strand=ignore_strand)
    on3 = got["group"][got["reference"] == 3]
    assert np.unique(on3).size > 5          # the long range of reference 2 does not reach into reference 3


# ---- labels -> CSR ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("labels", [
    [3, -1, 0, 3, 7, 0], [-1, -1, -1], [-1], [5], [4, 4, 4, 4], [2 ** 31 - 1, 0, -1, 2 ** 31 - 1],
    list(np.random.default_rng(5).integers(-1, 40, 3001)), list(np.random.default_rng(6).integers(-1, 2, 700) * 1000),
], ids=["missing labels", "all -1", "one -1", "one item", "one group", "the largest label", "3001 items", "two far labels"])
def test_labels_csr(labels):
    from sarlacc_amd import groups
    from sarlacc_amd.resident import DevBuffer
    labels = np.array(labels, np.int32)
    off, members = groups.labels_csr(DevBuffer.from_numpy(labels), labels.size)
    want = G.split_labels(labels)
    assert off.dtype == np.int64 and members.dtype == np.int32
    assert np.array_equal(off, want[0]) and np.array_equal(members, want[1])


# ---- end to end ------------------------------------------------------------------------------------------------------------
def test_from_sam_to_umi_groups_and_profiles(tmp_path):
    """SAM text -> sam2ranges -> readGroups -> umiGroup(groups=) and profileReads(assignment=), the reads a DeviceReads that
    went through write_bam."""
    from sarlacc_amd import generics
    from sarlacc_amd.resident import DeviceReads
    from sarlacc_amd.strset import lists_from_csr
    rng = np.random.default_rng(11)
    refs = ["".join("ACGT"[k] for k in rng.integers(0, 4, 300)) for _ in range(3)]
    n = 400
    names, seqs, umis, lines = [], [], [], []
    for i in range(n):
        key = "%08x-read-%d" % (int(rng.integers(0, 2 ** 31)), i)
        names.append(key + ("", " ch=%d" % i, "\tst=%d" % i)[i % 3])
        t, pos = int(rng.integers(0, 3)), int(rng.integers(0, 220))
        seq = refs[t][pos:pos + 60]
        seqs.append(seq)
        umis.append("".join("ACGT"[k] for k in rng.integers(0, 4, 12)) if i % 4 or i == 0 else umis[i - 1])
        if i % 10 == 9:                                    # unmapped: no row
            lines.append("%s\t4\t*\t0\t0\t*\t*\t0\t0\t%s\t%s" % (key, seq, "I" * 60))
            continue
        lines.append("%s\t0\tT%d\t%d\t60\t60M\t*\t0\t0\t%s\t%s" % (key, t, pos + 1, seq, "I" * 60))
        if i % 6 == 0:                                     # a shorter supplementary row elsewhere
            lines.append("%s\t2048\tT%d\t%d\t60\t20M40S\t*\t0\t0\t%s\t%s" % (key, (t + 1) % 3, 5, seq, "I" * 60))
    order = rng.permutation(len(lines))
    sam = tmp_path / "mapped.sam"
    sam.write_text("@HD\tVN:1.6\n" + "".join("@SQ\tSN:T%d\tLN:300\n" % t for t in range(3)) + "".join(lines[j] + "\n" for j in order))
    bam = tmp_path / "reads.bam"
    generics.write_bam(str(bam), generics.Reads(seqs, ["I" * 60] * n, names=names))
    dev = DeviceReads.from_bam(str(bam))
    assert len(dev) == n and list(dev.names) == [G.key_of(s) for s in names]

    ranges = generics.sam2ranges(str(sam))
    out = generics.readGroups(ranges, dev, by="reference")
    want = G.expected(ranges, names, by="reference")
    G.same(out, want, "end to end")
    assert (out["record"] < 0).sum() == n // 10 and out["n.records"].max() == 2 and out["unmatched.records"] == 0
    got_groups = lists_from_csr(*out["groups"])
    clusters = generics.umiGroup(umis, threshold1=1, groups=got_groups)
    expected = generics.umiGroup(umis, threshold1=1, groups=lists_from_csr(*want["groups"]))
    assert [c.tolist() for c in clusters] == [c.tolist() for c in expected] and len(clusters) > 3
    aligned = generics.multiReadAlign(generics.Reads(seqs), [got_groups[0][:5]])
    assert len(aligned["alignments"]) == 1
    profiles = generics.profileReads(dev, refs, assignment=out["reference"])
    assert len(profiles) == 3 and all(len(p["score"]) == int((out["reference"] == k).sum()) for k, p in enumerate(profiles))
