"""sequenceGroups without a device: the plain-Python restatement of its rules (tests/sketch_cases.py) is pinned on
literals worked out by hand, the argument checks raise before the library is touched, no reads return the empty result
without one, and on the mock reads that the device test uses the restatement alone finds one group per transcript."""
import numpy as np
import pytest

from sarlacc_amd import generics
from sarlacc_amd.strset import lists_from_csr
from tests import sketch_cases as S


@pytest.fixture
def no_library(monkeypatch):
    """Any touch of the native library fails the test."""
    from sarlacc_amd import _lib

    def refuse():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", refuse)


# ---- rules 1 to 3 ----------------------------------------------------------------------------------------------------------
def test_fmix64_literals():
    """MurmurHash3's 64-bit finaliser: 0 is its fixed point; the value at 1 is the published one.  By hand for 1:
    1 ^ 1 >> 33 = 1; * 0xff51afd7ed558ccd = 0xff51afd7ed558ccd; ^ >> 33 (0x7fa8d7eb) = 0xff51afd792fd5b26; ..."""
    assert S.fmix64(0) == 0
    assert S.fmix64(1) == 0xb456bcfc34c2cb2c
    assert 0xff51afd7ed558ccd ^ (0xff51afd7ed558ccd >> 33) == 0xff51afd792fd5b26
    assert S.fmix64(2) == 0x3abf2a20650683e7
    xs = list(range(1, 2000)) + [S.M64, 1 << 63, (1 << 62) - 1]
    assert len(set(S.fmix64(x) for x in xs)) == len(xs)


def test_plane_value_and_reverse_complement_of_ACGTT():
    """A 0, C 1, G 2, T 3.  ACGTT: low code bits 0 1 0 1 1 -> lo = 2 + 8 + 16 = 26, high code bits 0 0 1 1 1 -> hi = 4 + 8 +
    16 = 28.  Its reverse complement is AACGT: low bits 0 0 1 0 1 -> 4 + 16 = 20, high bits 0 0 0 1 1 -> 8 + 16 = 24; by the
    planes: ~26 = 00101b in five bits, reversed 10100b = 20; ~28 = 00011b, reversed 11000b = 24."""
    x = S.kmer_value("ACGTT")
    assert x == 26 | (28 << 32)
    assert S.revcomp_value(x, 5) == 20 | (24 << 32) == S.kmer_value("AACGT")
    assert S.revcomp_value(S.revcomp_value(x, 5), 5) == x
    assert S.read_hashes("ACGTT", 5, canonical=True) == [S.fmix64(20 | (24 << 32))]      # the smaller of the two values
    assert S.read_hashes("ACGTT", 5, canonical=False) == [S.fmix64(26 | (28 << 32))]
    assert S.read_hashes("AACGT", 5, canonical=True) == S.read_hashes("ACGTT", 5, canonical=True)


def test_even_k_palindrome_is_its_own_reverse_complement():
    """AACGTT: low bits 0 0 1 0 1 1 -> 4 + 16 + 32 = 52, high bits 0 0 0 1 1 1 -> 56."""
    x = S.kmer_value("AACGTT")
    assert x == 52 | (56 << 32) and S.revcomp_value(x, 6) == x
    assert S.read_hashes("AACGTT", 6, True) == S.read_hashes("AACGTT", 6, False) == [S.fmix64(x)]


def test_every_other_byte_breaks_a_kmer():
    assert len(S.read_hashes("ACGTACGTAC", 5)) == 6
    for bad in ("N", "a", "t", "-", "\x80", "\xff", "\x00"):
        assert len(S.read_hashes("ACGTA" + bad + "CGTAC", 5)) == 2, bad       # one k-mer either side
        assert len(S.read_hashes("ACGT" + bad + "ACGT", 5)) == 0
    assert S.read_hashes("ACGT", 5) == [] and S.read_hashes("", 5) == []


def test_the_numpy_restatement_is_the_scalar_one():
    rng = np.random.default_rng(0)
    reads = [S.random_bases(rng, n) for n in (0, 4, 5, 31, 64, 300)] + [b"ACGTNACGTACGTacgtACGTACGTACGTACGTACGTACGTAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAACCCCCGT\xff"]
    for s in reads:
        for k in (5, 6, 13, 16, 31):
            for canonical in (True, False):
                assert S.read_hashes_np(s, k, canonical).tolist() == S.read_hashes(s, k, canonical), (len(s), k, canonical)


def test_sketch_keeps_the_minimum_of_every_bucket():
    top = 1 << 60                                           # 16 buckets: the top four bits
    hashes = [3 * top + 5, 3 * top + 2, 15 * top + 9, 7, 3 * top + 2]
    sk, nk = S.sketch_of(hashes, 16)
    assert nk == 5 and sk.dtype == np.uint64
    assert sk.tolist() == [7, S.EMPTY, S.EMPTY, 3 * top + 2] + [S.EMPTY] * 11 + [15 * top + 9]
    sk, nk = S.sketch_of([], 64)
    assert nk == 0 and (sk == np.uint64(S.EMPTY)).all()
    sk, nk = S.sketches([b"ACGTACGTAC", b"ACG", b""], 5, 16)
    assert sk.shape == (3, 16) and nk.tolist() == [6, 0, 0] and (sk[1:] == np.uint64(S.EMPTY)).all()


# ---- rules 5 to 7 ----------------------------------------------------------------------------------------------------------
def test_three_reads_written_out():
    """Sorted entries: (10, 0) (10, 1) (11, 2) (20, 0) (20, 1) (30, 1) (30, 2) (40, 0) (40, 2).  Pairs: 0-1 by hash 10, 0-1 by 20,
    1-2 by 30, 0-2 by 40."""
    assert S.shared_counts(S.THREE_READS, 8) == S.THREE_SHARED == {(0, 1): 2, (1, 2): 1, (0, 2): 1}
    links, npairs, nlinks = S.links_of(S.THREE_READS, 8, 2)
    assert links.tolist() == [(0 << 32) | 1] and (npairs, nlinks) == (3, 1)
    assert S.components_of(links, 3).tolist() == [0, 0, 1]
    links, npairs, nlinks = S.links_of(S.THREE_READS, 8, 1)
    assert links.tolist() == [1, 2, (1 << 32) | 2] and (npairs, nlinks) == (3, 3)
    assert S.components_of(links, 3).tolist() == [0, 0, 0]
    assert S.links_of(S.THREE_READS, 8, 3)[1:] == (3, 0)
    assert S.components_of([], 3).tolist() == [0, 1, 2]
    assert S.components_of(S.links_of(S.THREE_READS, 8, 2)[0], 3, nkmers=[4, 0, 2]).tolist() == [0, -1, 1]


def test_a_long_run_gives_a_band_of_pairs():
    sk = S.hand_sketches([[0, 1, 2, 3]])
    assert sorted(S.shared_counts(sk, 2)) == [(0, 1), (0, 2), (1, 2), (1, 3), (2, 3)]          # 0-3 lies at distance 3
    assert len(S.shared_counts(sk, 3)) == 6 and sorted(S.shared_counts(sk, 1)) == [(0, 1), (1, 2), (2, 3)]


def test_labels_ascend_by_lowest_member():
    links = [(5 << 32) | 6, (2 << 32) | 4, (4 << 32) | 5, (1 << 32) | 3]
    assert S.components_of(links, 8).tolist() == [0, 1, 2, 1, 2, 2, 2, 3]
    assert S.components_of(links, 8, nkmers=[0, 1, 1, 1, 1, 1, 1, 1]).tolist() == [-1, 0, 1, 0, 1, 1, 1, 2]


@pytest.mark.parametrize("seed", S.SEEDS)
def test_mock_reads_give_one_group_per_transcript(seed):
    """12 transcripts x 10 reads of 600 bases, mock.mutate's defaults (5 % substitutions, 1 % indels), shuffled, half of them
    reverse-complemented: the defaults return exactly one group per transcript."""
    reads, transcript = S.mock_set(seed)
    assert len(reads) == 120 and sorted(np.bincount(transcript).tolist()) == [10] * 12
    want = S.expected(reads)
    assert S.one_group_per_transcript(want["group"], transcript)
    assert want["groups"][0].tolist() == list(range(0, 121, 10)) and sorted(want["groups"][1].tolist()) == list(range(1, 121))
    assert int(want["n.links"]) <= 12 * 45 <= int(want["n.pairs"]) and (want["n.kmers"] > 500).all()
    unflipped = S.expected(S.mock_set(seed, flip=False)[0], canonical=False)
    assert S.one_group_per_transcript(unflipped["group"], transcript)
    assert not S.one_group_per_transcript(S.expected(reads, canonical=False)["group"], transcript)     # strands apart without it


# ---- argument handling ---------------------------------------------------------------------------------------------------
READS = generics.Reads(["ACGTACGTACGTACGTACGT", "ACGTACGTACGTACGTACGA"])


@pytest.mark.parametrize("kwargs, message", [
    (dict(k=4), "'k' should be an integer in 5 .. 31"),
    (dict(k=32), "'k' should be an integer in 5 .. 31"),
    (dict(k=13.0), "'k' should be an integer in 5 .. 31"),
    (dict(k=True), "'k' should be an integer in 5 .. 31"),
    (dict(buckets=48), "'buckets' should be a power of two in 16 .. 256"),
    (dict(buckets=512), "'buckets' should be a power of two in 16 .. 256"),
    (dict(buckets=8), "'buckets' should be a power of two in 16 .. 256"),
    (dict(window=0), "'window' should be an integer in 1 .. 64"),
    (dict(window=65), "'window' should be an integer in 1 .. 64"),
    (dict(min_shared=0), "'min_shared' should be an integer in 1 .. buckets"),
    (dict(min_shared=65), "'min_shared' should be an integer in 1 .. buckets"),
    (dict(buckets=16, min_shared=17), "'min_shared' should be an integer in 1 .. buckets"),
    (dict(min_shared=None), "'min_shared' should be an integer in 1 .. buckets"),
])
def test_bad_arguments_raise_before_the_library(no_library, kwargs, message):
    with pytest.raises(ValueError, match=message):
        generics.sequenceGroups(READS, **kwargs)
    with pytest.raises(ValueError, match=message):
        generics.sequenceGroups(generics.Reads([]), **kwargs)


def test_reads_of_another_kind_are_refused(no_library):
    with pytest.raises(ValueError, match="'reads' should be a resident.DeviceReads or a Reads"):
        generics.sequenceGroups(["ACGT"])


def test_empty_input_needs_no_device(no_library):
    got = generics.sequenceGroups(generics.Reads([]))
    S.same(got, S.expected([]), "no reads")
    assert got["group"].size == 0 and got["groups"][0].tolist() == [0] and got["groups"][1].size == 0
    assert got["n.kmers"].size == 0 and got["n.pairs"] == 0 and got["n.links"] == 0
    assert lists_from_csr(*got["groups"]) == []


def test_the_largest_min_shared_is_accepted(no_library):
    from sarlacc_amd import sketch
    assert sketch.check_args(31, 256, 64, 256) == (31, 256, 64, 256) and sketch.check_args(5, 16, 1, 1) == (5, 16, 1, 1)
    assert sketch.check_args(np.int64(13), np.int32(64), np.int8(8), np.int16(3)) == (13, 64, 8, 3)
