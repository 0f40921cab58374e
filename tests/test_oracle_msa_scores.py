"""The oracle's banded affine pairwise DP (oracle/msa.c orc_msa_pairwise, shared by both MSA specs) against an independent
full-matrix DP in 64-bit integers, under every scoring set the GPU tests use (tests/msa_score_cases.py).

For groups of two reads the rows of oracle.quick_msa ARE the pairwise alignment (spec v1: the read against the centre;
spec v2: every aligned pair is a library edge of positive weight, so the heaviest chain keeps them all), so their score
under the scheme must equal the optimum inside the band.  The score is compared, not the path: ties are the oracle's to
break.  Also here: the stated scoring domain and spec v2's weight guard, as the oracle states them."""
import numpy as np
import pytest

from tests import msa_score_cases as K

NEG = -(1 << 60)


def banded_optimum(r, c, ma, mm, ge, go, bandwidth):
    """Optimal score of a global alignment of r (rows) against c (columns) with moves confined to the diagonals
    j - i in [min(0, lc - lr) - bw, max(0, lc - lr) + bw]; a gap of length k scores go + (k - 1) ge.  Anti-diagonal sweep
    over full (lr + 2) x (lc + 2) matrices (one row and column of padding), int64."""
    lr, lc = len(r), len(c)
    bw = K.pair_bandwidth(bandwidth, lr, lc)
    assert bw >= 0
    dlo, dhi = min(0, lc - lr) - bw, max(0, lc - lr) + bw
    rb = np.frombuffer(K.dna5(r).encode(), np.uint8) if lr else np.zeros(0, np.uint8)
    cb = np.frombuffer(K.dna5(c).encode(), np.uint8) if lc else np.zeros(0, np.uint8)
    H = np.full((lr + 2, lc + 2), NEG, np.int64)
    E = H.copy()
    F = H.copy()
    H[1, 1] = 0
    for t in range(1, lr + lc + 1):
        i = np.arange(max(0, t - lc), min(lr, t) + 1)
        j = t - i
        keep = (j - i >= dlo) & (j - i <= dhi)
        i, j = i[keep], j[keep]
        if i.size == 0:
            continue
        e = np.maximum(H[i, j + 1] + go, E[i, j + 1] + ge)        # from (i - 1, j)
        f = np.maximum(H[i + 1, j] + go, F[i + 1, j] + ge)        # from (i, j - 1)
        same = rb[np.maximum(i - 1, 0)] == cb[np.maximum(j - 1, 0)] if lr and lc else np.zeros(i.size, bool)
        d = H[i, j] + np.where(same, ma, mm)                      # from (i - 1, j - 1); padding where i or j is 0
        e, f, d = np.maximum(e, NEG), np.maximum(f, NEG), np.maximum(d, NEG)
        E[i + 1, j + 1] = e
        F[i + 1, j + 1] = f
        H[i + 1, j + 1] = np.maximum(d, np.maximum(e, f))
    return int(H[lr + 1, lc + 1])


def rows_score(ra, rb, ma, mm, ge, go, bandwidth):
    """Score of two gapped rows under the recurrences of DESIGN.md section 5, the read of `ra` as rows i, that of `rb`
    as columns j.  A gap of length k scores go + (k - 1) ge -- unless opening is cheaper than extending (the default
    scores as the aligner sees them: open -1, extend -5): the recurrence E = max(H + go, E + ge) may open again from an
    H that is itself the end of a gap, so every further character of a run costs max(ge, go).
    Gap columns of both kinds between two aligned columns: the merging of either spec writes them in its own order
    (spec v1: a read's insertions before the centre's position; spec v2: the first child's columns first), whatever
    order the pairwise path took them in.  Such a block scores as its best ordering INSIDE the band -- the orderings are
    all alignments of the same bases, and the optimum is over all of them.  (What this gives up: had the oracle's own
    path taken such a block in a worse order than the best one, the rows -- its only output -- would not show it.)"""
    assert len(ra) == len(rb)
    lr, lc = len(ra.replace("-", "")), len(rb.replace("-", ""))
    bw = K.pair_bandwidth(bandwidth, lr, lc)
    dlo, dhi = min(0, lc - lr) - bw, max(0, lc - lr) + bw
    cont = max(ge, go)

    def block(p, q, diag):
        """best score of p row-only and q column-only steps from diagonal `diag`, every cell inside the band"""
        if p == 0 or q == 0:
            n = p + q
            end = diag - p + q
            assert dlo <= min(diag, end) and max(diag, end) <= dhi, "the rows leave the band"
            return go + (n - 1) * cont if n else 0
        best = {(0, 0, 0): 0}   # (u, v, last): last 1 = row step, 2 = column step
        for u in range(p + 1):
            for v in range(q + 1):
                for last in (0, 1, 2):
                    s = best.get((u, v, last))
                    if s is None:
                        continue
                    if u < p and dlo <= diag - (u + 1) + v:
                        k = (u + 1, v, 1)
                        best[k] = max(best.get(k, NEG), s + (cont if last == 1 else go))
                    if v < q and diag - u + (v + 1) <= dhi:
                        k = (u, v + 1, 2)
                        best[k] = max(best.get(k, NEG), s + (cont if last == 2 else go))
        ends = [best[k] for k in ((p, q, 1), (p, q, 2)) if k in best]
        assert ends, "the rows leave the band"
        return max(ends)

    score, i, j, p, q = 0, 0, 0, 0, 0
    for x, y in list(zip(ra, rb)) + [("$", "$")]:
        assert x != "-" or y != "-", "a column of two gaps"
        if y == "-":
            p += 1
        elif x == "-":
            q += 1
        else:
            score += block(p, q, j - i)
            i, j, p, q = i + p, j + q, 0, 0
            assert dlo <= j - i <= dhi, "the rows leave the band"
            if x != "$":
                score += ma if x == y else mm
                i, j = i + 1, j + 1
    return score


def test_independent_dp_known_answers():
    """The checker itself on alignments small enough to do by hand."""
    assert banded_optimum("ACGT", "ACGT", 1, -1, -1, -2, 3) == 4
    assert banded_optimum("ACGT", "AGT", 1, -1, -1, -2, 3) == 1            # three matches, one gap opened
    assert banded_optimum("AAAA", "AA", 0, -1, -5, -1, 3) == -2            # open -1, extension -5: two gaps of one
    assert banded_optimum("AAAA", "AA", 0, -1, -1, -5, 3) == -6
    assert banded_optimum("ACGT", "TGCA", 0, -1, -1, -1, 0) == -4           # bandwidth 0: the diagonal only
    assert banded_optimum("AC", "", 0, -1, -2, -3, 5) == -5
    assert rows_score("AC-GT", "ACCG-", 1, -1, -1, -2, 3) == 1 + 1 - 2 + 1 - 2
    assert rows_score("A--CT", "AGG-T", 1, -1, 1, -5, 0) == 1 - 5 - 5 - 5 + 1    # band [0, 1]: the block has to alternate
    assert rows_score("A--CT", "AGG-T", 1, -1, 1, -5, 1) == 1 - 5 + 1 - 5 + 1


def _pairs():
    rng = np.random.default_rng(20260)
    out = []
    for bw in (0, 3, 20, 100):
        for diff in sorted({0, 1, bw - 1, bw + 1} - {-1}):
            out.append((bw, *K.related_pair(rng, 80, diff)))
    out.append((100, *K.related_pair(rng, 300, 5)))
    out.append((20, *K.related_pair(rng, 40, 2)))
    out.append((600, *K.related_pair(rng, 60, 4)))                      # the band cap shrinks this pair's bandwidth
    out.append((20, K.random_read(rng, 120), K.random_read(rng, 110)))   # unrelated
    out.append((3, K.random_read(rng, 70), K.random_read(rng, 72)))
    out.append((20, "A" * 50, "A" * 47))
    out.append((3, "A" * 60, "C" * 60))
    out.append((20, "AAAAACCCCCGGGGGTTTTT" * 3, "AAAACCCCCCGGGGTTTTTT" * 3))
    return out


PAIRS = _pairs()


@pytest.mark.parametrize("name", list(K.SETS) + ["fractional"])
def test_oracle_pairwise_score_is_the_banded_optimum(oracle, name):
    scores = K.FRACTIONAL[0] if name == "fractional" else K.SETS[name]
    ma, mm, ge, go = (int(v) for v in scores)
    for bw, a, b in PAIRS:
        best = banded_optimum(b, a, ma, mm, ge, go, bw)
        assert best == banded_optimum(a, b, ma, mm, ge, go, bw)           # (the band is symmetric under exchanging the reads)
        for spec in (1, 2):
            rows = oracle.quick_msa([[1, 2]], [a, b], *scores, bw, spec=spec)[0]
            assert [r.replace("-", "") for r in rows] == [K.dna5(a), K.dna5(b)]
            got = rows_score(rows[0], rows[1], ma, mm, ge, go, bw)
            assert got == best, (name, spec, bw, len(a), len(b), got, best)
            if name == "fractional":
                assert rows == oracle.quick_msa([[1, 2]], [a, b], *K.FRACTIONAL[1], bw, spec=spec)[0]


def test_oracle_scoring_domain(oracle):
    """max |score| * (2 * longest read + 2) < 2^27, on truncated scores, over the reads of the call's groups."""
    reads = ["ACGT" * 375, "ACGA" * 375, "ACGT"]
    inside = ((1 << 27) - 1) // (2 * 1500 + 2)
    assert inside * 3002 < (1 << 27) <= (inside + 1) * 3002
    for spec in (1, 2):
        oracle.quick_msa([[1, 2]], reads, 0, -inside, -inside, -inside, 10, spec=spec)
        oracle.quick_msa([[1, 2]], reads, 0, -1, -inside - 0.9, -1, 10, spec=spec)            # truncated toward zero
        for bad in [(0, -inside - 1, -1, -1), (0, -1, -1, -inside - 1), (inside + 1, -1, -1, -1), (0, -100000, -100000, -100000),
                    (0, -1, float("nan"), -1), (0, float("-inf"), -1, -1), (0, -1, -1, -3e9)]:
            with pytest.raises(oracle.OracleError, match="scoring domain"):
                oracle.quick_msa([[1, 2]], reads, *bad, 10, spec=spec)
        # the longest read of the GROUPS decides, not of the read vector
        oracle.quick_msa([[3]], reads, 0, -100000, -100000, -100000, 10, spec=spec)


def test_oracle_weight_guard_never_acts_on_unit_weights(oracle):
    """Spec v2's guard (16-bit record weights, 32-bit row weights and chain sums) as a function of group size, longest read
    and W = max(match, mismatch, 1): W = 1 fits for every group spec v2 takes; the stated corner values."""
    for n in range(1, 65):
        for longest in (0, 1, 60, 2000, 30000, 65471):
            assert oracle.msa2_weights_fit(n, longest, 0, -1)
            assert oracle.msa2_weights_fit(n, longest, 1, 1)
            assert oracle.msa2_weights_fit(n, longest, 1.9, -2.9)
    assert oracle.msa2_weights_fit(64, 60, 1040, -1040) and not oracle.msa2_weights_fit(64, 60, 1041, -1041)   # 63 * 1040 = 65 520
    assert oracle.msa2_weights_fit(64, 64, 1040, -1040) and not oracle.msa2_weights_fit(64, 66, 1040, -1040)   # the chain sum
    assert not oracle.msa2_weights_fit(16, 60, 5000, -5000) and not oracle.msa2_weights_fit(33, 60, 5000, -5000)
    assert oracle.msa2_weights_fit(14, 60, 5000, -5000)                                                        # 13 * 5000 = 65 000
    assert oracle.msa2_weights_fit(2, 65471, 65535, 0) and not oracle.msa2_weights_fit(2, 65471, 65536, 0)
    assert not oracle.msa2_weights_fit(8, 400, 1, 70000)                                                       # mismatch above match counts
