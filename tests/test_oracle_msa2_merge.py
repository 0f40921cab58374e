"""What tests/test_gpu_msa_merge.py rests on, asserted on the CPU statement of MSA spec v2 alone (oracle/msa2.c; no GPU): the
inputs of tests/msa_merge_cases.py do reach the paths they are built for -- matches further behind the front of the chain than
the product's ring holds, joins without a single match, profiles exactly as wide as the first-pass capacity and one column
wider, and groups on the class boundaries of the merge in which both row rules act -- and every row still spells its read.

The reach statistics (max_row_reach, max_reach_ahead, joins_reach_certain, joins_reach_possible; msa2.c MSA2_RING_REACH) are
checked here against a restatement in Python on a match list small enough to follow by hand."""
import pytest

from tests import msa_merge_cases as M


def stats_of(oracle, key, read_groups, params):
    rows, st = M.reference(oracle, key, read_groups, params)
    reads, groups = M.flatten(read_groups)
    M.rows_spell(rows, reads, groups)
    return rows, st


def test_split_reaches_behind_the_ring(oracle):
    """split(600): in the join of [V | U] with U + V every row has a match 600 columns behind the front -- certainly beyond
    the ring; the four-read variant has two such joins (the second child is then a profile of two members)."""
    rows, st = stats_of(oracle, "split600", [M.split(600)], M.DEFAULT)
    assert st["joins"] == 2 and st["joins_reach_certain"] >= 1
    assert st["max_row_reach"] >= 600 and st["max_reach_ahead"] >= st["max_row_reach"]
    assert st["joins_reach_possible"] >= st["joins_reach_certain"]
    rows4, st4 = stats_of(oracle, "split600x", [M.split(600, extra=1)], M.DEFAULT)
    assert st4["joins"] == 3 and st4["joins_reach_certain"] >= 1
    assert len(rows4[0]) == 4 and rows4[0][2] == rows4[0][3]


def test_split_behind_a_prefix_reaches_back_late_in_the_join(oracle):
    """split(560, prefix=330): the last join is [P + V | P + U] with P + U + V, and its first 330 rows are the columns of P,
    matched on the diagonal -- the alignment starts with 330 columns without a gap, the same base in every row -- before the rows
    whose matches lie 560 columns apart."""
    read_groups = [M.split(560, prefix=330)]
    rows, st = stats_of(oracle, "split560p", read_groups, M.DEFAULT)
    assert oracle.msa2_tree(read_groups[0], *M.DEFAULT)[0].tolist() == [[0, 1], [3, 2]]
    assert all(rows[0][0][c] != "-" and rows[0][0][c] == rows[0][1][c] == rows[0][2][c] for c in range(330))
    assert st["joins_reach_certain"] == 1 == st["joins_reach_possible"] and st["max_row_reach"] >= 560


@pytest.mark.parametrize("extra", [22, 31])
def test_split_with_many_copies_still_reaches_behind_the_ring(oracle, extra):
    """groups of 25 and 34 reads (the multi-wavefront classes of the merge) keep a join with matches 600 columns apart"""
    _, st = stats_of(oracle, ("split600", extra), [M.split(600, extra=extra)], M.DEFAULT)
    assert st["joins"] == extra + 2 and st["joins_reach_certain"] >= 1 and st["max_row_reach"] >= 600


def test_split_400_stays_inside_the_ring(oracle):
    """split(400): the same shape with every match inside the ring, also with the 63 rows of look-ahead a block of the kernel
    can add (measured: 416 columns over the rows up to a row, 471 with the look-ahead, against 510)."""
    _, st = stats_of(oracle, "split400", [M.split(400)], M.DEFAULT)
    assert st["joins_reach_possible"] == 0 and st["joins_reach_certain"] == 0
    assert 400 <= st["max_row_reach"] <= st["max_reach_ahead"] < M.RING_REACH
    _, st = stats_of(oracle, "ordinary", [M.ordinary(1), M.ordinary(2)], M.DEFAULT)
    assert st["joins_reach_possible"] == 0 and st["max_reach_ahead"] < 150


@pytest.mark.parametrize("L", [60, 64, 65, 100])
def test_homopolymers_never_pair(oracle, L):
    rows, st = stats_of(oracle, ("homopolymers", L), [M.homopolymers(L)], M.GAPS_ONLY)
    assert len(rows[0][0]) == 4 * L
    assert st["joins"] == 3 and st["entries_kept"] == 0 and st["entries_before_filter"] == 0 and st["candidates"] == 0
    assert st["max_row_reach"] == 0 and st["joins_reach_possible"] == 0
    # the first-pass capacity of a four-read group is min(sum of lengths, 3 L + 64): met at L = 64, exceeded by one column at 65
    assert (4 * L <= 3 * L + 64) == (L <= 64)


def test_six_read_variant_outgrows_the_first_pass(oracle):
    rows, st = stats_of(oracle, "six", [M.six_read_overflow()], M.GAPS_ONLY)
    assert len(rows[0][0]) > 3 * 100 + 64
    assert st["joins"] == 5 and 0 < st["entries_kept"] <= 5 * 100
    # (and with ordinary clusters around it, as the GPU test calls it)
    rows3, _ = stats_of(oracle, "six+ordinary", [M.ordinary(3), M.six_read_overflow(), M.ordinary(4)], M.GAPS_ONLY)
    assert rows3[1] == rows[0]


@pytest.mark.parametrize("sizes", M.SWEEP_CALLS, ids=lambda s: "-".join(map(str, s)))
def test_sweep_rows_and_rules(oracle, sizes):
    """The boundary sweep: rows spell their reads at every size and molecule length (reads of 0 and 1 bases among them); from
    11 reads on, the groups of two molecules make the row cap and the noise filter act."""
    for size in sizes:
        sw = M.sweep(size)
        assert [len(g) for _, _, g in sw] == [size] * (2 * len(M.SWEEP_LENGTHS))
        _, st = stats_of(oracle, ("sweep", size), [g for _, _, g in sw], M.DEFAULT)
        assert st["joins"] == (size - 1) * len(sw)
        assert st["entries_kept"] == st["entries_before_filter"] - st["entries_filtered"]
        assert st["joins_reach_possible"] == 0
        if size >= 11:
            _, st2 = stats_of(oracle, ("sweep2", size), [g for _, nmol, g in sw if nmol == 2], M.DEFAULT)
            assert st2["rows_capped"] > 0 and st2["entries_filtered"] > 0
            assert st["rows_capped"] >= st2["rows_capped"] and st["entries_filtered"] >= st2["entries_filtered"]


def test_sweep_holds_empty_reads():
    reads = [r for size in M.SWEEP_SIZES for _, _, g in M.sweep(size) for r in g]
    assert len(reads) == 4032 and sum(1 for r in reads if not r) >= 1 and sum(1 for r in reads if len(r) == 1) >= 100


def reach_restated(matches):
    """(max_row_reach, max_reach_ahead) of a match list [(row, column)] in row-major order, from the definition: over the rows
    that have matches, the largest column among the rows up to r (up to the 63rd row with matches after r) minus r's smallest"""
    rows = sorted({i for i, _ in matches})
    reach = ahead = 0
    for k, r in enumerate(rows):
        jmin = min(j for i, j in matches if i == r)
        reach = max(reach, max(j for i, j in matches if i <= r) - jmin)
        ahead = max(ahead, max(j for i, j in matches if i <= rows[min(k + 63, len(rows) - 1)]) - jmin)
    return reach, ahead


def test_reach_statistics_follow_their_definition(oracle):
    """Two reads: the match list of the only join is the pairwise alignment itself (one match per aligned pair, no third read),
    which the rows give back -- the statistics against their definition restated above.  V against U + V with a wide band
    aligns V to the second half: column i + S of the second child is matched from row i on, so the look-ahead of 63 rows
    reaches 63 columns further than the rows up to a row do."""
    for key, pair, params in [("pairA", [M.split(300)[0], M.split(300)[2]], (0, -1, -5, -1, 400)),
                              ("pairB", M.ordinary(5, n=2, length=200), M.DEFAULT)]:
        rows, st = stats_of(oracle, key, [pair], params)
        a, b = rows[0]
        matches, i, j = [], 0, 0
        for x, y in zip(a, b):
            if x != "-" and y != "-":
                matches.append((i, j))
            i += x != "-"
            j += y != "-"
        assert st["joins"] == 1 and st["entries_kept"] == len(matches) > 100
        assert (st["max_row_reach"], st["max_reach_ahead"]) == reach_restated(matches)
        assert st["max_row_reach"] == 0 and st["max_reach_ahead"] >= 63
        assert st["joins_reach_certain"] == 0 and st["joins_reach_possible"] == 0
