"""Oracle for the alignment-profiling routines (find_homopolymers, match_homopolymers, find_errors)
against independent restatements of the checkers the reference's tests carry -- FINDCHECK and MATCHCHECK of
tests/testthat/test-homopolymer.R:4-126 and CHECKFUN of tests/testthat/test-error.R:4-36 -- on the literal
alignment strings of those tests (DNAString upper-cases its input, so the literals are upper-cased here)."""
import numpy as np
import pytest

from tests.profile_cases import ERROR_CASES, FIND_SEQS, MATCH_CASES, checkfun, findcheck, matchcheck
from tests.profile_walk_cases import EDGE_LENGTHS, RANDOM_TOTALS, by_reference, coverage, family, random_pairs


def test_find_homopolymers_literals(oracle):
    got = oracle.find_homopolymers(FIND_SEQS)
    want = findcheck(FIND_SEQS)
    assert [np.asarray(x).tolist() for x in got[:3]] == [want[0], want[1], want[2]] and got[3] == want[3]
    assert [np.asarray(x).tolist() if not isinstance(x, list) else x for x in oracle.find_homopolymers([])] == [[], [], [], []]
    # all test sequences spell the same molecule: same homopolymers whatever the gaps
    by_seq = {}
    for i, p, s, b in zip(*[np.asarray(x).tolist() if not isinstance(x, list) else x for x in got]):
        by_seq.setdefault(i, []).append((p, s, b))
    assert by_seq[0] == by_seq[1] == by_seq[2] == by_seq[4] == by_seq[5] == [(3, 4, "G"), (7, 2, "C"), (10, 3, "T"), (13, 2, "A")]
    assert by_seq[3] == [(3, 4, "G"), (7, 2, "C"), (10, 3, "T"), (13, 4, "A")]


@pytest.mark.parametrize("k", range(len(MATCH_CASES)))
def test_match_homopolymers_literals(oracle, k):
    reads, refs = MATCH_CASES[k]
    for rd, rf in zip(reads, refs):
        got = oracle.match_homopolymers([rf], [rd])
        pos, rlen = matchcheck(rf, rd)
        assert np.asarray(got[0]).tolist() == [0] * len(pos)
        assert np.asarray(got[1]).tolist() == pos and np.asarray(got[2]).tolist() == rlen, (rd, rf)


@pytest.mark.parametrize("k", range(len(ERROR_CASES)))
def test_find_errors_literals(oracle, k):
    reads, refs = ERROR_CASES[k]
    for rd, rf in zip(reads, refs):
        got = oracle.find_errors([rf], [rd])
        want = checkfun([rf], [rd])
        assert got[0] == want[0]
        for a, b in zip(got[1:6], want[1:6]):
            assert np.asarray(a).tolist() == b, (rd, rf)
        ins = {}
        for p, l in zip(np.asarray(got[6]).tolist(), np.asarray(got[7]).tolist()):
            ins.setdefault(p, []).append(l)
        assert {p: sorted(v) for p, v in ins.items()} == want[6], (rd, rf)


def test_find_errors_many_alignments_and_errors(oracle):
    ref = "GGAAAC-GATCAGCTACGAACACT"
    refs = [ref, ref.replace("-", ""), "GG-AAACGATCAGCTACGAACACT--"]
    reads = ["GGAAACTGATCAGCTACGAACACT", "GGAAACGATCAGCTACGAACAC-", "GGTAAACGA-CAGCTACGAACACTAA"]
    got = oracle.find_errors(refs, reads)
    want = checkfun(refs, reads)
    assert got[0] == want[0] and [np.asarray(x).tolist() for x in got[1:6]] == list(want[1:6])
    with pytest.raises(oracle.OracleError, match="lengths of alignment vectors should match up"):
        oracle.find_errors(refs, reads[:2])
    with pytest.raises(oracle.OracleError, match="equal length"):
        oracle.find_errors(["ACGT"], ["ACG"])
    with pytest.raises(oracle.OracleError, match="same for all alignments"):
        oracle.find_errors(["ACGT", "ACGTA"], ["ACGT", "ACGTA"])
    with pytest.raises(oracle.OracleError, match="unknown character 'N'"):
        oracle.find_errors(["ACGT"], ["ACNT"])
    with pytest.raises(oracle.OracleError, match="lengths of alignment vectors should match up"):
        oracle.match_homopolymers(["AACC"], [])
    with pytest.raises(oracle.OracleError, match="equal length"):
        oracle.match_homopolymers(["AACC"], ["AAC"])


# ---- the structured family (tests/profile_walk_cases.py): features of 1 .. 193 characters at every phase of a 64-character step
def _l(xs):
    return [x if isinstance(x, (list, str)) else np.asarray(x).tolist() for x in xs]


def _insertions(pos, lens):
    ins = {}
    for p, l in zip(np.asarray(pos).tolist(), np.asarray(lens).tolist()):
        ins.setdefault(p, []).append(l)
    return {p: sorted(v) for p, v in ins.items()}


def _same_errors(got, want):
    assert got[0] == want[0] and _l(got[1:6]) == list(want[1:6])
    assert _insertions(got[6], got[7]) == want[6]


@pytest.fixture(scope="module")
def walk_pairs():
    return [(rf, rd) for _, rf, rd in family()] + list(random_pairs())


def test_family_covers_the_step_carries():
    fam = family()
    refs = sorted({rf for _, rf, _ in fam})
    reads = sorted({rd for _, _, rd in fam})
    for strings in (refs, reads, [rf for rf, _ in random_pairs()]):
        c = coverage(strings)
        counts = {k: v for k, v in c.items() if not isinstance(v, set)}
        print(counts)
        assert all(v > 0 for v in counts.values()), counts
    c = coverage(refs)
    assert c["longest_gap_run"] >= 193 and c["longest_run"] >= 193
    assert set(EDGE_LENGTHS) <= c["gap_run_lengths"] and set(EDGE_LENGTHS) <= c["run_lengths"]
    assert set(EDGE_LENGTHS) <= coverage(reads)["run_lengths"]
    # every kind and variant is there, none with a gap opposite a gap
    assert {n.split(":")[0] for n, _, _ in fam} >= set("abcdfe") and {n.split(":")[-1] for n, _, _ in fam} >= {"i", "ii", "iii", "iv", "v", "vi"}
    assert all(len(rf) == len(rd) and not any(x == y == "-" for x, y in zip(rf, rd)) for _, rf, rd in fam)
    assert {len(rf) for rf, _ in random_pairs()} == set(RANDOM_TOTALS) and 250 <= len(random_pairs()) <= 350
    # the count itself, on strings small enough to check by eye
    c = coverage(["-" * 64 + "A" + "-" * 63 + "-" * 10, "AC" + "G" * 62 + "G" * 64 + "GT", "T" * 64 + "AA"])
    assert (c["all_gap_steps"], c["no_start_steps"], c["starts_at_lane_0"], c["ends_at_lane_63"]) == (1, 1, 4, 1)
    assert (c["longest_gap_run"], c["longest_run"]) == (73, 127) and c["gap_run_lengths"] == {64, 73} and c["run_lengths"] == {1, 2, 64, 127}


def test_find_homopolymers_family(oracle, walk_pairs):
    for seqs in ([rf for rf, _ in walk_pairs], [rd for _, rd in walk_pairs]):
        assert _l(oracle.find_homopolymers(seqs)) == _l(findcheck(seqs))


def test_match_homopolymers_family(oracle, walk_pairs):
    refs, reads = [rf for rf, _ in walk_pairs], [rd for _, rd in walk_pairs]
    idx, pos, rlen = [], [], []
    for i, (rf, rd) in enumerate(walk_pairs):
        p, l = matchcheck(rf, rd)
        idx += [i] * len(p); pos += p; rlen += l
    assert _l(oracle.match_homopolymers(refs, reads)) == [idx, pos, rlen]
    # references without a base have no run to match
    for rf, rd in (("", ""), ("-", "A"), ("-" * 64, "G" * 64), ("-" * 129, "N" * 129)):
        assert matchcheck(rf, rd) == ([], []) and _l(oracle.match_homopolymers([rf], [rd])) == [[], [], []]
    # the read's run in the extension only counts 0, with one base of the run proper all of it
    for name, rf, rd in family():
        variant = name.split(":")[-1]
        if name[0] in "df" and variant in ("iv", "v"):
            F = name.split(":")[2]
            assert matchcheck(rf, rd) == ([rf.replace("-", "").index("GG") + 1], [0 if variant == "iv" else int(F) + 1]), name


def test_find_errors_family(oracle, walk_pairs):
    for rf, rd in walk_pairs:
        _same_errors(oracle.find_errors([rf], [rd]), checkfun([rf], [rd]))
    groups = by_reference(walk_pairs)
    assert max(len(g[0]) for g in groups.values()) >= 30
    for refs, reads in groups.values():
        got = oracle.find_errors(refs, reads)
        _same_errors(got, checkfun(refs, reads))
        # the list itself: alignment by alignment, left to right
        pos, lens = [], []
        for rf, rd in zip(refs, reads):
            one = oracle.find_errors([rf], [rd])
            pos += np.asarray(one[6]).tolist(); lens += np.asarray(one[7]).tolist()
        assert _l(got[6:8]) == [pos, lens]
    # N opposite reference gaps only is no error; opposite a base it is
    assert any(n.endswith(":vi") for n, _, _ in family())
    with pytest.raises(oracle.OracleError, match="unknown character 'N'"):
        oracle.find_errors(["G" + "-" * 64 + "A"], ["G" + "N" * 64 + "N"])
