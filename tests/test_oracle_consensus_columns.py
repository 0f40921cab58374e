"""The builders of tests/consensus_columns.py against the oracle: the columns lie where the builders say -- next to
the rounding boundaries of every Phred level, on tied sums, on the coverage products -- so that
tests/test_gpu_consensus_columns.py, which only compares strings, cannot quietly lose its teeth.  Also here: under the
default MSA scores the oracle's MSA returns the gap-free alignments of the fused routes unchanged, so the vote on the
alignment IS the vote on the oracle's MSA rows."""
import numpy as np
import pytest

from tests import consensus_columns as K


def _realised(oracle, n, delta, odd):
    """distance of every engineered column's Phred value (from the oracle's log errors) from its k + 0.5"""
    rows, quals, enc, levels, cols = K.boundary_alignment(n, delta, odd)
    cons, lerr = oracle.create_consensus_quality(rows, 0.6, quals, enc)
    assert len(cons) == len(rows[0])
    return K.phred_values(lerr)[cols] - (np.array(levels) + 0.5)


@pytest.mark.parametrize("odd", [False, True])
def test_engineered_boundaries_lie_where_asked(oracle, odd):
    """Family A: for |delta| >= 1e-8 every column lies at 0.5 .. 2 |delta| from its boundary on the side asked for, for
    |delta| <= 3e-10 inside the 1e-9 window of the host re-evaluation; the row counts together reach k = 1 .. 92."""
    reached = set()
    for n in (K.A_ROWS_ODD if odd else K.A_ROWS):
        for delta in K.DELTAS:
            levels = K.boundary_table(n, delta, odd)[0]
            reached |= set(levels)
            d = _realised(oracle, n, delta, odd)
            if abs(delta) >= 1e-8:
                ratio = d / delta
                assert ratio.min() >= 0.5 and ratio.max() <= 2.0, (n, delta, ratio.min(), ratio.max())
            else:
                assert np.abs(d).max() < 1e-9, (n, delta, np.abs(d).max())
    assert reached == set(range(1, 93))
    if not odd:
        assert K.boundary_table(1, 0.0)[0] == tuple(range(1, 80))          # the clamp at 1e-8 ends one row's levels
        assert K.boundary_table(64, 0.0)[0] == tuple(range(10, 93))        # an error of 0.74 starts those of 64 rows


def test_engineered_boundaries_basic_vote(oracle):
    """Family A, basic vote.  The reference evaluates log1p(-p) with p = (n + pc / 4) / (n + pc) next to 1: the two
    roundings of p (quotient, 1 - p) are 2^-53 each against 1 - p = 10^(-x/10), i.e. 2 * (10 / ln 10) * 2^-53 *
    10^(x/10) in the Phred value (6e-10 at level 60).  Every column lies within that of k + 0.5 + delta; for
    |delta| >= 1e-8 that is inside 0.5 .. 2 |delta| on the side asked for."""
    levels = [k for _, k in K.BASIC_PAIRS]
    assert min(levels) == 2 and max(levels) == 60 and len(K.BASIC_PAIRS) >= 12
    for n, k in K.BASIC_PAIRS:
        noise = 2 * (10 / np.log(10)) * 2.0 ** -53 * 10 ** ((k + 1) / 10) + 1e-13
        assert noise < 2e-9
        for delta in K.DELTAS:
            pc = K.basic_pseudo_count(n, k + 0.5 + delta)
            assert pc > 0
            aln = K.basic_alignment(n)
            cons, lerr = oracle.create_consensus_basic(aln, 0.6, pc)
            assert cons == aln[0]
            d = K.phred_values(lerr) - (k + 0.5)
            assert np.abs(d - delta).max() <= noise, (n, k, delta, np.abs(d - delta).max())
            if abs(delta) >= 1e-8:
                assert (d / delta).min() >= 0.5 and (d / delta).max() <= 2.0


def _msa_unchanged(oracle, alns):
    reads = [r for a in alns for r in a]
    groups, at = [], 1
    for a in alns:
        groups.append(list(range(at, at + len(a))))
        at += len(a)
    assert oracle.quick_msa(groups, reads, *K.DEFAULT_SCORES) == [list(a) for a in alns]


@pytest.mark.parametrize("n,odd", [(n, False) for n in K.A_ROWS] + [(n, True) for n in K.A_ROWS_ODD])
def test_engineered_alignments_pass_the_msa_unchanged(oracle, n, odd):
    """(the bases of boundary_alignment depend on (n, odd) only, so one offset stands for all)"""
    rows = K.boundary_alignment(n, 0.0, odd)[0]
    assert all(K.boundary_alignment(n, d, odd)[0] == rows for d in (1e-3, -1e-8))
    _msa_unchanged(oracle, [rows])


@pytest.mark.parametrize("n", K.B_ROWS)
def test_searched_boundaries(oracle, n):
    """Family B: at least 200 columns within 1e-3 of a boundary and 50 within 4e-4, by the oracle's own log errors"""
    alns, quals = K.searched_alignments(n)
    enc = K.phred_table()
    x = np.concatenate([K.phred_values(oracle.create_consensus_quality(a, 0.6, q, enc)[1]) for a, q in zip(alns, quals)])
    assert x.size == K.searched_columns(n)[2].size
    d = np.abs(K.boundary_distance(x))
    assert x.max() < 93.4 and d.max() < 1e-3 + 1e-9
    assert x.size >= 200 and int((d < 4e-4).sum()) >= 50, (n, x.size, int((d < 4e-4).sum()))
    assert all(len(a[0]) <= K.B_WIDTH for a in alns)
    _msa_unchanged(oracle, K.searched_fused(n)[0])


def test_near_ties(oracle):
    """Family C: in at least 30 % of the columns the base changes when the rows are added in reverse or even rows first,
    at least 20 % are exact ties in row order; the oracle's base is the first maximum of the sums in row order."""
    changes, ties = [], []
    errors, _ = K.phred_table()
    for n in K.C_ROWS:
        c, t = K.tie_statistics(n)
        changes.append(c)
        ties.append(t)
        rows, quals = K.tie_alignment(n)
        cons, lerr = oracle.create_consensus_quality(rows, 0.6, quals, K.phred_table())
        s = K.column_sums(*K.tie_columns(n), errors)
        assert cons == "".join(K.BASES[b] for b in np.argmax(s, axis=0)), n
        assert np.allclose(K.phred_values(lerr), K.chain_phred(s), rtol=0, atol=1e-9)
    changes, ties = np.concatenate(changes), np.concatenate(ties)
    assert changes.mean() >= 0.30 and ties.mean() >= 0.20, (changes.mean(), ties.mean())
    alns, _ = K.tie_fused()
    assert max(len(a) for a in alns) == 64 and all(len(a[0]) == 10 * (1 + K.FILL) for a in alns)
    _msa_unchanged(oracle, alns)


def test_coverage_products(oracle):
    """Family D: every alignment realises every incidence count and has columns of N alone; the oracle keeps a column
    exactly when !(incidence < nrows * mincov) in fp64.  The family holds products that round off the integer they stand
    for: 25 * 0.28 and 41 * (7 / 41) exceed 7, so a column with exactly 7 is dropped; 22 * (15 / 22) stays below 15.
    (5 * 0.6 and 10 * 0.3 are exactly 3 in fp64.)"""
    assert 25 * 0.28 > 7 and 0.28 in K.coverage_values(25) and 41 * (7 / 41) > 7 and 22 * (15 / 22) < 15
    assert 5 * 0.6 == 3 and 10 * 0.3 == 3
    above = [(n, v, round(n * v)) for n in K.D_ROWS for v in K.coverage_values(n) if 0 < round(n * v) < n * v < round(n * v) + 1e-9]
    below = [(n, v) for n in K.D_ROWS for v in K.coverage_values(n) if round(n * v) - 1e-9 < n * v < round(n * v)]
    assert len(above) >= 30 and len(below) >= 30
    for n, v, j in above:
        rows, quals = K.coverage_alignment(n)
        inc = (np.array([list(r) for r in rows]) != "-").sum(axis=0)
        assert len(oracle.create_consensus_basic(rows, v, 1.0)[0]) == int((inc > j).sum()) < int((inc >= j).sum())
    enc = K.phred_table()
    for n in K.D_ROWS:
        rows, quals = K.coverage_alignment(n)
        grid = np.array([list(r) for r in rows])
        inc = (grid != "-").sum(axis=0)
        assert set(inc.tolist()) == set(range(n + 1))
        only_n = ((grid == "N") | (grid == "-")).all(axis=0) & (inc > 0)
        assert only_n.sum() >= 1
        plain = np.array([list(r) for r in K.coverage_alignment(n, False)[0]])
        assert not (plain == "N").any() and set((plain != "-").sum(axis=0).tolist()) == set(range(n + 1))
        vals = K.coverage_values(n)
        assert {j / n for j in range(n + 1)} <= set(vals) and {1 / 3, 2 / 3, 0.35, 0.6, 1.0000001, -0.1, 0.0, 1.0} <= set(vals)
        for v in vals if n <= 16 or n == 257 else vals[::7]:
            kept = int((~(inc < n * v)).sum())
            assert len(oracle.create_consensus_quality(rows, v, quals, enc)[0]) == kept, (n, v)
            assert len(oracle.create_consensus_basic(rows, v, 1.0)[0]) == kept, (n, v)
    batches = K.coverage_batches()
    assert sum(len(v) for v in batches.values()) == sum(len(K.coverage_values(n)) for n in K.D_ROWS)
    # the reads of the fused routes: the MSA stage's rows have gaps
    for n in (2, 7, 64):
        reads, _ = K.coverage_reads(n)
        rows = oracle.quick_msa([list(range(1, n + 1))], reads, *K.DEFAULT_SCORES)[0]
        assert any("-" in r for r in rows)


def test_boundary_floods(oracle):
    """Family E: every one of the 6 000 columns lies within 1e-9 of its boundary, so each is an entry of the list"""
    rows, pc = K.flood_basic()
    x = K.phred_values(oracle.create_consensus_basic(rows, 0.6, pc)[1])
    assert x.size == K.E_COLUMNS > 4096 and np.abs(x - 20.5).max() < 1e-9
    rows, quals, enc = K.flood_quality()
    x = K.phred_values(oracle.create_consensus_quality(rows, 0.6, quals, enc)[1])
    assert x.size == K.E_COLUMNS and np.abs(x - 25.5).max() < 1e-9
    alns, qs = K.split_groups(rows, quals)
    assert len(alns) == K.E_GROUPS and sum(len(a[0]) for a in alns) == K.E_COLUMNS
    # an N in the last column leaves the other columns on the boundary
    x = K.phred_values(oracle.create_consensus_quality(K.with_n(alns[0]), 0.6, qs[0], enc)[1])
    assert (np.abs(x - 25.5) < 1e-9).sum() == len(alns[0][0]) - 1
    _msa_unchanged(oracle, [rows])
