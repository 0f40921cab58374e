"""Rule 6a of DESIGN §4.19 -- the alignment check of sequenceGroups' links -- without a device: the plain-numpy
restatement (tests/links_verify_cases.py) is held to an unbanded Levenshtein distance and pinned on literals worked out
by hand, the new arguments are refused before the library is touched, the header declares the call and _lib binds it,
and on the planted sets of the device test the restatement alone separates what the sketch cannot."""
import os
import re

import numpy as np
import pytest

from sarlacc_amd import generics, sketch
from tests import links_verify_cases as V
from tests import sketch_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def no_library(monkeypatch):
    """Any touch of the native library fails the test."""
    from sarlacc_amd import _lib

    def refuse():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", refuse)


# ---- the banded distance ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [0, 1, 3, 8])
def test_the_banded_distance_against_the_unbanded_one(w):
    """Equal whenever the true distance is at most w (a path of cost d stays within d diagonals of the main one), never
    below it otherwise; infinite exactly when the lengths differ by more than w."""
    rng = np.random.default_rng(100 + w)
    xs, ys = [], []
    for _ in range(400):
        x = bytearray(S.random_bases(rng, int(rng.integers(0, 25))))
        y = bytearray(x)
        for _ in range(int(rng.integers(0, 5))):
            p, kind = int(rng.integers(0, len(y) + 1)), int(rng.integers(0, 3))
            if kind == 0 and p < len(y):
                y[p] = b"ACGTNa"[int(rng.integers(0, 6))]
            elif kind == 1 and p < len(y):
                del y[p]
            else:
                y.insert(p, b"ACGT"[int(rng.integers(0, 4))])
        if rng.random() < 0.2:
            y = bytearray(S.random_bases(rng, int(rng.integers(0, 25))))
        xs.append(bytes(x))
        ys.append(bytes(y))
    got = V.banded_many(xs, ys, w)
    equal = 0
    for x, y, d in zip(xs, ys, got):
        true = V.levenshtein(x, y)
        assert (d is None) == (abs(len(x) - len(y)) > w), (x, y, w, d)
        if true <= w:
            assert d == true, (x, y, w, d, true)
            equal += 1
        elif d is not None:
            assert d >= true, (x, y, w, d, true)
    assert equal >= 40


def test_distances_worked_out_by_hand():
    # G-ATTACA / GCAT-GCA: insert C, delete a T, substitute A by G
    assert V.levenshtein("GATTACA", "GCATGCA") == 3 and V.levenshtein("ACGT", "ACGT") == 0 and V.levenshtein("", "ACG") == 3
    assert V.banded("ACGT", "ACGT", 0) == 0 and V.banded("ACGT", "AGGT", 0) == 1
    # ACGT -> CGTA: delete A in front, append A behind: 2, off the main diagonal; the diagonal alone sees four mismatches
    assert V.levenshtein("ACGT", "CGTA") == 2 and V.banded("ACGT", "CGTA", 1) == 2 and V.banded("ACGT", "CGTA", 0) == 4
    assert V.banded("ACGT", "ACG", 0) is None and V.banded("ACGT", "ACG", 1) == 1
    assert V.banded("", "", 0) == 0 and V.banded("", "AC", 2) == 2 and V.banded("AC", "", 1) is None


def test_only_upper_case_bases_match():
    """N against N and a against A are mismatches, like every byte that is no base against itself."""
    assert V.banded("ACNGT", "ACNGT", 3) == 1 and V.levenshtein("ACNGT", "ACNGT") == 1
    assert V.banded("ACaGT", "ACAGT", 3) == 1 and V.banded("ACaGT", "ACaGT", 3) == 1
    for bad in (b"N", b"a", b"t", b"-", b"\x80", b"\xff", b"\x00"):
        assert V.banded(b"AC" + bad + b"GT", b"AC" + bad + b"GT", 2) == 1, bad
    assert V.banded("NNNN", "NNNN", 4) == 4


def test_the_reverse_complement_rule():
    assert V.rc("AACGT") == b"ACGTT" and V.rc("") == b""
    assert V.rc("ANcG-") == b"-CcNT"                       # every other byte stays, lower case too
    assert V.rc(V.rc("ACGTNNacgt")) == b"ACGTNNacgt"


def test_the_threshold_is_integer_arithmetic():
    assert V.max_diff_ppm(0.8) == 200000 and V.max_diff_ppm(1.0) == 0 and V.max_diff_ppm(0.7) == 300000
    assert V.threshold(V.max_diff_ppm(0.8), 7, 5) == 1          # 200000 * 7 = 1400000 div 10^6
    assert V.threshold(V.max_diff_ppm(0.8), 5, 7) == 1 and V.threshold(V.max_diff_ppm(0.8), 4, 4) == 0 and V.threshold(V.max_diff_ppm(0.8), 5, 5) == 1
    assert V.threshold(V.max_diff_ppm(1.0), 7, 7) == 0 and V.threshold(999999, 10 ** 6, 1) == 999999
    assert sketch.check_verify_args(0.8, 100) == (200000, 100) and sketch.check_verify_args(1.0, 0) == (0, 0)


def test_the_decision_on_literals():
    """Reads of 10 bases at identity 0.8: t = 2."""
    ppm = V.max_diff_ppm(0.8)
    a = b"AACCGGTTAC"
    one, three = b"AACCGGTTAG", b"TACCGCTTAG"                     # 1 and 3 substitutions
    seqs = [a, one, three, V.rc(one), b"ACGTACGT" + b"AC", b"ACGTACGT" + b"GT"]
    links = V.links_between([(0, 1), (0, 2), (0, 3), (4, 5), (1, 3)])
    kept, dist, strand = V.verify(seqs, links, ppm, 5)
    assert dist.tolist() == [1, -1, 1, 2, 0] and strand.tolist() == [0, 0, 1, 0, 1]
    assert kept.tolist() == links[[0, 2, 3, 4]].tolist()
    kept, dist, strand = V.verify(seqs, links, ppm, 5, both_strands=False)
    assert dist.tolist() == [1, -1, -1, 2, -1] and strand.tolist() == [0, 0, 0, 0, 0] and kept.size == 2


def test_forward_is_chosen_when_both_orientations_pass():
    """Q = ACGGTCATGC GCATGACCGT is its own reverse complement (20 bases, t = 4).  a = Q with base 2 substituted; b = rc(a) is
    Q with the mirrored base 17 substituted: forward the two differ in two places, reverse in none.  Both pass; the
    forward result is the one reported."""
    q = b"ACGGTCATGC" + V.rc(b"ACGGTCATGC")
    assert q == b"ACGGTCATGCGCATGACCGT" == V.rc(q)
    a = b"ACTGTCATGCGCATGACCGT"
    b = V.rc(a)
    assert b == b"ACGGTCATGCGCATGACAGT" and V.banded(a, b, 5) == 2 and V.banded(a, V.rc(b), 5) == 0
    seqs = [a, b, q, q]
    _, dist, strand = V.verify(seqs, V.links_between([(0, 1), (2, 3), (0, 2)]), V.max_diff_ppm(0.8), 5)
    assert dist.tolist() == [2, 0, 1] and strand.tolist() == [0, 0, 0]


def test_a_read_whose_links_all_fail_is_a_group_of_one():
    rng = np.random.default_rng(2)
    a, b = S.random_bases(rng, 200), S.random_bases(rng, 200)
    seqs = [a, a[:100] + b[100:], b]                         # the middle read shares half with either neighbour
    assert S.expected(seqs, min_shared=1)["group"].tolist() == [0, 0, 0]
    want = V.expected(seqs, min_shared=1, identity=0.8)
    assert want["group"].tolist() == [0, 1, 2] and int(want["n.links"]) == 2 and int(want["n.verified"]) == 0


@pytest.mark.parametrize("seed", S.SEEDS)
@pytest.mark.parametrize("rates, min_shared, identity", V.PLANTED)
def test_planted_sets_need_the_alignment(seed, rates, min_shared, identity):
    """Neighbouring transcripts share 100 of 300 bases: the sketch chains each such pair into one group (4 groups), the
    sketch and the alignment return the 8 transcripts."""
    seqs, transcript = V.planted_set(seed, *rates)
    assert len(seqs) == 48 and sorted(np.bincount(transcript).tolist()) == [6] * 8
    plain = S.expected(seqs, min_shared=min_shared)
    assert not S.one_group_per_transcript(plain["group"], transcript) and plain["group"].max() + 1 == 4
    want = V.expected(seqs, min_shared=min_shared, identity=identity)
    assert S.one_group_per_transcript(want["group"], transcript)
    assert int(want["n.verified"]) < int(want["n.links"]) == int(plain["n.links"])


# ---- argument handling ---------------------------------------------------------------------------------------------------
READS = generics.Reads(["ACGTACGTACGTACGTACGT", "ACGTACGTACGTACGTACGA"])


@pytest.mark.parametrize("kwargs, message", [
    (dict(identity=0), "'identity' should be a number in \\(0, 1\\]"),
    (dict(identity=0.0), "'identity' should be a number in \\(0, 1\\]"),
    (dict(identity=-0.5), "'identity' should be a number in \\(0, 1\\]"),
    (dict(identity=1.01), "'identity' should be a number in \\(0, 1\\]"),
    (dict(identity=float("nan")), "'identity' should be a number in \\(0, 1\\]"),
    (dict(identity=True), "'identity' should be a number in \\(0, 1\\]"),
    (dict(identity="0.8"), "'identity' should be a number in \\(0, 1\\]"),
    (dict(identity=0.8 + 0j), "'identity' should be a number in \\(0, 1\\]"),
    (dict(identity=1e-9), "'identity' should be a number in \\(0, 1\\]"),
    (dict(identity=0.8, bandwidth=-1), "'bandwidth' should be an integer in 0 .. 127"),
    (dict(identity=0.8, bandwidth=128), "'bandwidth' should be an integer in 0 .. 127"),
    (dict(identity=0.8, bandwidth=100.0), "'bandwidth' should be an integer in 0 .. 127"),
    (dict(identity=0.8, bandwidth=True), "'bandwidth' should be an integer in 0 .. 127"),
    (dict(identity=0.8, bandwidth=None), "'bandwidth' should be an integer in 0 .. 127"),
])
def test_bad_arguments_raise_before_the_library(no_library, kwargs, message):
    with pytest.raises(ValueError, match=message):
        generics.sequenceGroups(READS, **kwargs)
    with pytest.raises(ValueError, match=message):
        generics.sequenceGroups(generics.Reads([]), **kwargs)
    with pytest.raises(ValueError, match=message):
        sketch.verify_links(None, None, 2, None, 1, kwargs["identity"], kwargs.get("bandwidth", 100))


def test_the_edges_of_the_ranges_are_accepted(no_library):
    assert sketch.check_verify_args(1, 127) == (0, 127) and sketch.check_verify_args(np.float32(0.5), np.int8(0)) == (500000, 0)
    assert sketch.check_verify_args(1e-6, 100) == (999999, 100)
    got = generics.sequenceGroups(generics.Reads([]), identity=0.8)
    assert int(got["n.verified"]) == 0 and isinstance(got["n.verified"], np.int64) and got["group"].size == 0
    assert "n.verified" not in generics.sequenceGroups(generics.Reads([]))


def test_the_header_declares_the_call_and_the_table_binds_it():
    import ctypes as C

    from sarlacc_amd import _lib
    with open(os.path.join(ROOT, "include", "sarlacc_amd.h")) as fh:
        header = re.sub(r"\s+", " ", fh.read())
    assert ("int sarlacc_dev_links_verify(const uint8_t* d_seq, const int64_t* d_off, int64_t n, const uint64_t* d_links, int64_t n_links, "
            "int bandwidth, int64_t max_diff_ppm, int both_strands, int32_t* d_dist, uint8_t* d_strand, uint64_t* d_kept, int64_t* n_kept, "
            "void* stream);") in header
    restype, argtypes = _lib._prototypes()["sarlacc_dev_links_verify"]
    p = _lib.Pointer
    assert restype is C.c_int and argtypes == [p, p, C.c_int64, p, C.c_int64, C.c_int, C.c_int64, C.c_int, p, p, p, p, p]
