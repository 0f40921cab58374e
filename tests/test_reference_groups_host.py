"""The restatement of generics.referenceGroups (tests/reference_groups_cases.py) pinned on literals worked
out by hand, rule by rule, generics.read_fasta, and every refusal that comes before a device is touched.  Needs neither
the library nor a device."""
import gzip

import numpy as np
import pytest

from tests import links_verify_cases as V
from tests import reference_groups_cases as R

# two references and three reads for M4 / M5: the reads are reference 0 with one substitution, the
# reverse complement of reference 1 with two, and a sequence that is neither
REF0 = b"ACGTACGTTGCAGGCTAACGTTAGCCATGCAAGT"
REF1 = b"TTGACCATGGCATCAAGTCCGATTGCAGTACGGA"
READ0 = REF0[:10] + b"A" + REF0[11:]                       # C -> A at base 10
FLIPPED1 = V.rc(REF1[:6] + b"T" + REF1[7:20] + b"A" + REF1[21:])      # A -> T at base 6, G -> A at base 20, then flipped
READ2 = b"GGGGGGGGGGCCCCCCCCCCAAAAAAAAAATTTT"


@pytest.fixture
def no_library(monkeypatch):
    """Any touch of the native library fails the test."""
    from sarlacc_amd import _lib

    def refuse():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", refuse)


def test_m2_hits_by_bucket():
    shared, nhits = R.hits_of(R.HAND_REFS, R.HAND_READS)
    assert shared == R.HAND_SHARED and nhits == R.HAND_HITS == 3 + 1 + 1 + 2
    # an empty bucket on both sides is no hit, and equal hashes in different buckets are none
    assert R.hits_of([[R.E, 5]], [[R.E, 6], [5, R.E]]) == ({}, 0)
    # no window: every reference that holds the hash counts
    assert R.hits_of([[7]] * 5, [[7]]) == ({(0, f): 1 for f in range(5)}, 5)


def test_m3_candidates_ranked_and_cut():
    ref, shared, n = R.candidates_of(R.HAND_SHARED, 3, 1, 2)
    assert ref.tolist() == [[0, 1], [1, 0], [-1, -1]] and shared.tolist() == [[3, 1], [2, 1], [0, 0]] and n.tolist() == [2, 2, 0]
    assert ref.dtype == shared.dtype == n.dtype == np.int32
    ref, shared, n = R.candidates_of(R.HAND_SHARED, 3, 2, 2)            # min_shared 2 drops the single hits
    assert ref.tolist() == [[0, -1], [1, -1], [-1, -1]] and shared.tolist() == [[3, 0], [2, 0], [0, 0]] and n.tolist() == [1, 1, 0]
    ref, shared, n = R.candidates_of(R.HAND_SHARED, 3, 1, 1)            # max_candidates 1 keeps rank 0
    assert ref.tolist() == [[0], [1], [-1]] and n.tolist() == [1, 1, 0]
    # equal shared: the lower reference first, and the cut falls on the higher ones
    ref, shared, n = R.candidates_of({(0, 4): 2, (0, 1): 2, (0, 3): 5, (0, 0): 2}, 1, 1, 3)
    assert ref.tolist() == [[3, 0, 1]] and shared.tolist() == [[5, 2, 2]] and n.tolist() == [3]


def test_m4_check_of_every_slot():
    assert REF1[6:7] == b"A" and REF1[20:21] == b"G" and REF0[10:11] == b"C" and len(REF0) == len(REF1) == len(READ2) == 34
    reads, refs = [READ0, FLIPPED1, READ2], [REF0, REF1]
    cand = [[0, 1], [0, 1], [1, -1]]
    ppm = V.max_diff_ppm(0.9)                                           # t = 100000 * 34 // 10^6 = 3
    assert V.threshold(ppm, 34, 34) == 3
    dist, strand, checked = R.check_slots(refs, reads, cand, ppm, 10)
    assert dist.tolist() == [[1, -1], [-1, 2], [-1, -1]] and strand.tolist() == [[0, 0], [0, 1], [0, 0]] and checked == 5
    assert dist.dtype == np.int32 and strand.dtype == np.uint8
    dist, strand, checked = R.check_slots(refs, reads, cand, ppm, 10, both_strands=False)
    assert dist.tolist() == [[1, -1], [-1, -1], [-1, -1]] and strand.sum() == 0 and checked == 5
    # t = 1: the read with two differences fails
    dist, _, _ = R.check_slots(refs, reads, cand, V.max_diff_ppm(0.96), 10)
    assert V.threshold(V.max_diff_ppm(0.96), 34, 34) == 1 and dist.tolist() == [[1, -1], [-1, -1], [-1, -1]]


def test_m5_choice():
    cand_ref, cand_shared = [[0, 1], [0, 1], [-1, -1]], [[3, 1], [2, 2], [0, 0]]
    # smallest distance wins over the rank; equal distances go to the lower rank; nothing passing gives -1
    ref, strand, dist, shared = R.choose(cand_ref, cand_shared, [[4, 2], [5, 5], [-1, -1]], [[0, 1], [1, 0], [0, 0]])
    assert ref.tolist() == [1, 0, -1] and strand.tolist() == [1, 1, 0] and dist.tolist() == [2, 5, -1] and shared.tolist() == [1, 2, 0]
    ref, strand, dist, shared = R.choose(cand_ref, cand_shared, [[-1, -1], [-1, 0], [-1, -1]], [[0, 0], [0, 0], [0, 0]])
    assert ref.tolist() == [-1, 1, -1] and dist.tolist() == [-1, 0, -1] and shared.tolist() == [0, 2, 0]
    # identity=None: rank 0, dist -1, strand 0
    ref, strand, dist, shared = R.choose(cand_ref, cand_shared)
    assert ref.tolist() == [0, 0, -1] and strand.tolist() == [0, 0, 0] and dist.tolist() == [-1, -1, -1] and shared.tolist() == [3, 2, 0]
    assert ref.dtype == dist.dtype == shared.dtype == np.int32 and strand.dtype == np.uint8


def test_m1_to_m6_on_reads():
    """Sequences of 34 bases at k = 5: the read with one substitution and the flipped read with two reach their
    references, the third read has no candidate."""
    out = R.expected([READ0, FLIPPED1, READ2], [REF0, REF1], k=5, buckets=16, min_shared=1, identity=0.9, bandwidth=10)
    assert out["reference"].tolist() == [0, 1, -1] and out["strand"].tolist() == [0, 1, 0] and out["dist"].tolist() == [1, 2, -1]
    assert out["group"].tolist() == [0, 1, -1] and out["groups"][0].tolist() == [0, 1, 2] and out["groups"][1].tolist() == [1, 2]
    assert out["n.kmers"].tolist() == [30, 30, 30] and out["ref.n.kmers"].tolist() == [30, 30]
    assert out["shared"][2] == 0 and (out["shared"][:2] > 0).all() and int(out["n.checked"]) == int(out["n.candidates"].sum())
    plain = R.expected([READ0, FLIPPED1, READ2], [REF0, REF1], k=5, buckets=16, min_shared=1, identity=None)
    assert "n.checked" not in plain and plain["dist"].tolist() == [-1, -1, -1] and plain["strand"].tolist() == [0, 0, 0]
    # stranded sketches and no second strand: the flipped read is lost
    one = R.expected([READ0, FLIPPED1, READ2], [REF0, REF1], k=5, buckets=16, min_shared=1, identity=0.9, bandwidth=10, both_strands=False)
    assert one["reference"].tolist() == [0, -1, -1]


def test_planted_set_is_links_verify_cases_own():
    reads, transcript, refs = R.planted_set(2, 0.05, 0.01)
    same_reads, same_transcript = V.planted_set(2, 0.05, 0.01)
    assert reads == same_reads and np.array_equal(transcript, same_transcript)
    assert len(refs) == 8 and all(len(f) == 300 for f in refs) and refs[1][200:300] == refs[0][200:300] and refs[2][200:300] != refs[1][200:300]


def test_in_bucket():
    sk = R.in_bucket([[3, 4, R.E]] + [[R.E] * 3], 16)
    assert sk[0].tolist() == [3, (1 << 60) | 4, R.E] and sk.dtype == np.uint64


def test_read_fasta(tmp_path):
    from sarlacc_amd import generics
    text = b">one first record\nacgtn\nACGT\n\n>two\ttabbed\r\nGGCC\r\n>\nAC\n>empty\n>last\nT"
    plain, zipped = tmp_path / "refs.fa", tmp_path / "refs.fa.gz"
    plain.write_bytes(text)
    with gzip.open(zipped, "wb") as fh:
        fh.write(text)
    for path in (plain, zipped):
        got = generics.read_fasta(str(path))
        assert got.names == ["one", "two", "", "empty", "last"]
        assert got.seq.to_strings() == ["ACGTNACGT", "GGCC", "AC", "", "T"] and got.qual is None and len(got) == 5
    (tmp_path / "none.fa").write_bytes(b"")
    assert len(generics.read_fasta(str(tmp_path / "none.fa"))) == 0
    (tmp_path / "bad.fa").write_bytes(b"\nACGT\n>x\nAC\n")
    with pytest.raises(ValueError, match="line 2: sequence before the first"):
        generics.read_fasta(str(tmp_path / "bad.fa"))


@pytest.mark.parametrize("kwargs, message", [
    (dict(k=4), "'k'"), (dict(k=32), "'k'"), (dict(k=13.0), "'k'"), (dict(k=True), "'k'"),
    (dict(buckets=48), "'buckets'"), (dict(buckets=512), "'buckets'"), (dict(buckets=8), "'buckets'"),
    (dict(min_shared=0), "'min_shared'"), (dict(min_shared=65), "'min_shared'"), (dict(buckets=16, min_shared=17), "'min_shared'"),
    (dict(max_candidates=0), "'max_candidates'"), (dict(max_candidates=17), "'max_candidates'"), (dict(max_candidates=2.0), "'max_candidates'"),
    (dict(identity=0.0), "'identity'"), (dict(identity=1.5), "'identity'"), (dict(identity="0.8"), "'identity'"), (dict(identity=True), "'identity'"),
    (dict(bandwidth=-1), "'bandwidth'"), (dict(bandwidth=128), "'bandwidth'"), (dict(identity=None, bandwidth=128), "'bandwidth'"),
], ids=str)
def test_bad_arguments_are_refused_before_a_device(no_library, kwargs, message):
    from sarlacc_amd import generics
    reads = generics.Reads(["ACGTACGTACGTACGT"])
    with pytest.raises(ValueError, match=message):
        generics.referenceGroups(reads, ["ACGTACGTACGTACGT"], **kwargs)


@pytest.mark.parametrize("reads, references, message", [
    (["ACGT"], ["ACGT"], "'reads'"), (None, ["ACGT"], "'reads'"),
    ("Reads", "ACGT", "'references'"), ("Reads", [b"ACGT"], "'references'"), ("Reads", ["ACGT", 5], "'references'"),
], ids=str)
def test_bad_inputs_are_refused_before_a_device(no_library, reads, references, message):
    from sarlacc_amd import generics
    reads = generics.Reads(["ACGTACGTACGTACGT"]) if reads == "Reads" else reads
    with pytest.raises(ValueError, match=message):
        generics.referenceGroups(reads, references)


@pytest.mark.parametrize("identity", [0.8, None])
def test_no_reads_or_no_references_need_no_device(no_library, identity):
    from sarlacc_amd import generics
    two = [b"ACGTACGTACGTACGTAA", b"TTGACCATGGCATCAAGT"]
    for reads, refs in (([], two), (two, []), ([], [])):
        got = generics.referenceGroups(generics.Reads([s.decode() for s in reads]), [s.decode() for s in refs], identity=identity)
        R.same(got, R.expected(reads, refs, identity=identity), "%d reads, %d references" % (len(reads), len(refs)))
        assert (got["reference"] == -1).all() and len(got["reference"]) == len(reads) and len(got["ref.n.kmers"]) == len(refs)
        assert ("n.checked" in got) == (identity is not None) and got["groups"][0].tolist() == [0]
