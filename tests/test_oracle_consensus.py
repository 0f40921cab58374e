"""Pins the consensus oracle (oracle/consensus.c) and the MSA spec oracle without a GPU.

Follows tests/testthat/test-consensus.R of the reference: BASICFUN / QUALFUN /
errorToPhred are restated here in numpy (they stand in for Biostrings'
consensusMatrix), the literal alignments test.align / n.align are the reference's,
and the known answer AAAAGTAGTAAAAAGA is asserted.
"""
import math

import numpy as np
import pytest

TEST_ALIGN = ["AAAAGAAAAA-AAATAAAA", "ACACA-AAAA--AAT-AGA", "GA-AG-C-A-T-AAT-AAA",
              "AT-AG-T-AGTAAGA-AGA", "-AAAGAT-AGTCAGA-AGA", "AGAAAAT-AGAAATA-AGA"]
N_ALIGN = ["NAAAAANNN", "NNAANA---", "NNNANNN--", "NNNN--NN-"]
NUC = "ACGT"


def basicfun(aln, min_cov, pseudo):
    mat = np.array([list(r) for r in aln])
    counts = np.array([(mat == b).sum(0) for b in NUC + "N"])
    keep = counts.sum(0) >= min_cov * len(aln)
    x = counts[:4, keep].T
    best = x.argmax(1)                         # ties.method = "first"
    cons = "".join(NUC[b] for b in best)
    chosen = x[np.arange(len(best)), best]
    err = 1 - (chosen + pseudo / 4) / (x.sum(1) + pseudo)
    return cons, np.log(err)


def error_to_phred(lerr):
    score = np.round(np.asarray(lerr) / math.log(10) * -10)
    score = np.clip(score, 0, 93)
    return "".join(chr(int(s) + 33) for s in score)


def phred_roundtrip(p):
    """numeric error -> PhredQuality char -> numeric (loss of precision as in QUALFUN)."""
    q = int(np.clip(np.round(-10 * math.log10(p)), 0, 93)) if p > 0 else 93
    return chr(q + 33), 10 ** (-q / 10)


def qualfun(aln, quals_num, min_cov):
    mat = np.array([list(r) for r in aln])
    qm = np.full(mat.shape, np.nan)
    for i in range(mat.shape[0]):
        qm[i, mat[i] != "-"] = quals_num[i]
    keep = (mat != "-").sum(0) / mat.shape[0] >= min_cov
    mat, qm = mat[:, keep], qm[:, keep]
    cons, errs = [], []
    for c in range(mat.shape[1]):
        col, q = mat[:, c], qm[:, c]
        ok = np.isin(col, list(NUC))
        col, q = col[ok], np.clip(q[ok], 1e-8, 0.99999999)
        correct, incorrect = np.log1p(-q), np.log(q / 3)
        lp = np.array([correct[col == b].sum() + incorrect[col != b].sum() for b in NUC])
        p = np.exp(lp - lp.max())
        p /= p.sum()
        ch = int(p.argmax())
        cons.append(NUC[ch])
        errs.append(math.log(np.delete(p, ch).sum()))
    return "".join(cons), np.array(errs)


@pytest.mark.parametrize("aln", [TEST_ALIGN, N_ALIGN])
@pytest.mark.parametrize("cov,pc", [(0.6, 1), (0.6, 2), (0.2, 2), (0.9, 1), (0.0, 0.5), (1.0, 1)])
def test_basic_matches_consensus_matrix(oracle, aln, cov, pc):
    cons, lerr = oracle.create_consensus_basic(aln, cov, pc)
    wc, we = basicfun(aln, cov, pc)
    assert cons == wc
    assert np.allclose(lerr, we, rtol=0, atol=1e-12)


def test_basic_known_answer_and_empty(oracle):
    assert oracle.create_consensus_basic(TEST_ALIGN, 0.6, 1)[0] == "AAAAGTAGTAAAAAGA"
    cons, lerr = oracle.create_consensus_basic([], 0.6, 1)
    assert cons == "" and lerr.size == 0
    with pytest.raises(oracle.OracleError, match="same length"):
        oracle.create_consensus_basic(["AAA", "AA"], 0.6, 1)
    with pytest.raises(oracle.OracleError, match="unknown character 'X'"):
        oracle.create_consensus_basic(["AXA", "AAA"], 0.6, 1)


def test_basic_loop_is_per_call_plus_phred(oracle):
    cons, quals = oracle.create_consensus_basic_loop([N_ALIGN, TEST_ALIGN], 0.6, 1)
    r1 = oracle.create_consensus_basic(N_ALIGN, 0.6, 1)
    r2 = oracle.create_consensus_basic(TEST_ALIGN, 0.6, 1)
    assert cons == [r1[0], r2[0]]
    assert quals == [error_to_phred(r1[1]), error_to_phred(r2[1])]


@pytest.mark.parametrize("aln", [TEST_ALIGN, N_ALIGN])
@pytest.mark.parametrize("upper", [0.01, 0.1, 0.5, 1.0])
def test_quality_matches_qualfun(oracle, oenc, aln, upper):
    rng = np.random.default_rng(int(upper * 1000) + len(aln))
    qchars, qnum = [], []
    for row in aln:
        ps = rng.random(len(row.replace("-", ""))) * upper
        pairs = [phred_roundtrip(p) for p in ps]
        qchars.append("".join(c for c, _ in pairs))
        qnum.append(np.array([v for _, v in pairs]))
    for cov in (0.6, 0.2, 0.9):
        cons, lerr = oracle.create_consensus_quality(aln, cov, qchars, oenc)
        wc, we = qualfun(aln, qnum, cov)
        assert cons == wc
        assert np.allclose(lerr, we, rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("name", ["solexa", "n128_high", "n150_wrap", "zero_tail"])
@pytest.mark.parametrize("aln", [TEST_ALIGN, N_ALIGN])
def test_quality_matches_qualfun_under_other_tables(oracle, name, aln):
    """The same restatement of the quality vote under tables other than Phred+33, qualities drawn from the first name to
    six past the last (those take the last entry's probability)."""
    from tests.encodings import BY_NAME, draw_quals
    from tests.test_oracle_align import table_errs
    table = BY_NAME[name]
    last = table.first + len(table) - 1
    total = sum(len(r.replace("-", "")) for r in aln)
    # the whole table; then its last 40 entries and the characters past them (not fewer: probabilities below 1e-8 are
    # raised to 1e-8, and a column of equal weights is an exact tie that the two summation orders may break differently)
    for lo in (None, max(0, len(table) - 40)):
        qbytes = draw_quals(table, [len(r.replace("-", "")) for r in aln], len(name) + len(aln), lo=lo)
        qnum = [np.array(table_errs(table, q)) for q in qbytes]
        if lo is not None and last < 127 and total >= 46:
            assert max((b - 256 if b >= 128 else b) for q in qbytes for b in q) > last
        for cov in (0.6, 0.2, 0.9):
            cons, lerr = oracle.create_consensus_quality(aln, cov, qbytes, table.oenc)
            wc, we = qualfun(aln, qnum, cov)
            assert cons == wc
            assert np.allclose(lerr, we, rtol=1e-9, atol=1e-9)


def test_quality_errors_and_loop(oracle, oenc):
    cons, lerr = oracle.create_consensus_quality([], 0.6, [], oenc)
    assert cons == "" and lerr.size == 0
    with pytest.raises(oracle.OracleError, match="different numbers of entries"):
        oracle.create_consensus_quality(N_ALIGN[:1], 0.6, [], oenc)
    with pytest.raises(oracle.OracleError, match="quality vector is shorter than the alignment sequence"):
        oracle.create_consensus_quality(N_ALIGN[:1], 0.6, ["I"], oenc)
    with pytest.raises(oracle.OracleError, match="quality vector is longer than the alignment sequence"):
        oracle.create_consensus_quality(N_ALIGN[:1], 0.6, ["I" * 1000], oenc)
    stuff = [TEST_ALIGN, N_ALIGN]
    quals = [["5" * len(r.replace("-", "")) for r in a] for a in stuff]
    cons, ph = oracle.create_consensus_quality_loop(stuff, 0.6, quals, oenc)
    for k in range(2):
        c, e = oracle.create_consensus_quality(stuff[k], 0.6, quals[k], oenc)
        assert cons[k] == c and ph[k] == error_to_phred(e)


def test_phred_string_caps(oracle):
    assert oracle.errors_to_string([0.0, -1e9, math.log(0.1), math.log(1e-5)]) == "!~+S"


# ---------------------------------------------------------------------------
# MSA spec v1 (own algorithm, parity with the reference unpinned): structural contract only
def test_msa_contract(oracle):
    rng = np.random.default_rng(3)
    from sarlacc_amd.mock import mutate, NUC as NUCB
    for trial in range(6):
        truth = NUCB[rng.integers(0, 4, 300)]
        reads = [mutate(truth, rng).tobytes().decode() for _ in range(int(rng.integers(2, 9)))]
        groups = [list(range(1, len(reads) + 1))]
        rows = oracle.quick_msa(groups, reads, 0, -1, -5, -1, 100)[0]
        assert len(rows) == len(reads)
        assert len({len(r) for r in rows}) == 1
        for row, read in zip(rows, reads):
            assert row.replace("-", "") == read
        assert not any(all(r[c] == "-" for r in rows) for c in range(len(rows[0])))
        # consensus of the alignment recovers most of the molecule
        cons, _ = oracle.create_consensus_basic(rows, 0.6, 1)
        if len(reads) >= 6:
            from tests.test_oracle_umi import lev2
            assert lev2(cons, truth.tobytes().decode()) / 2 <= 0.03 * len(truth)
    # singletons verbatim, empty groups empty, non-ACGT shown as N
    out = oracle.quick_msa([[2], [], [1, 3]], ["ACGRT", "acgt", "ACGT"], 0, -1, -5, -1, 100)
    assert out[0] == ["acgt"] and out[1] == [] and out[2] in (["ACGNT", "ACG-T"], ["ACGNT", "AC-GT"])
    # Rd example of the reference (man/multiReadAlign.Rd:72-77): one-base deletion
    out = oracle.quick_msa([[1, 2]], ["ACACTGGTTCAGGT", "ACACGGTTCAGGT"], 0, -1, -5, -1, 100)[0]
    assert out[0] == "ACACTGGTTCAGGT" and out[1].replace("-", "") == "ACACGGTTCAGGT" and len(out[1]) == 14


def test_msa_band_cap_rule(oracle):
    """orc_msa_pairwise's band cap: |lc - lr| >= 1024 -> diagonal alignment; otherwise the bandwidth shrinks
    to what fits into 1024 diagonals, so an enormous `bandwidth` equals the largest one that fits."""
    rng = np.random.default_rng(3)
    a = "".join(rng.choice(list("ACGT"), 1500))
    b = a[:300]
    for spec in (1, 2):
        rows = oracle.quick_msa([[1, 2]], [a, b], 0, -1, -5, -1, 100, spec=spec)[0]
        assert rows[0] == a and rows[1] == b + "-" * 1200          # position p opposite position p
        rows = oracle.quick_msa([[1, 2]], [b, a], 0, -1, -5, -1, 100, spec=spec)[0]
        assert rows[1] == a and rows[0] == b + "-" * 1200
    c = a[:200] + a[260:900]                                        # 60-base deletion, 900 vs 840 bases
    big = oracle.quick_msa([[1, 2]], [a[:900], c], 0, -1, -5, -1, 10 ** 6, spec=1)[0]
    fit = oracle.quick_msa([[1, 2]], [a[:900], c], 0, -1, -5, -1, (1023 - 60) // 2, spec=1)[0]
    assert big == fit and big[1].replace("-", "") == c
