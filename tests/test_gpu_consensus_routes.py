"""Which kernels a consensus call ran, read from the library's own counters: "consensus_route" (0 k_consensus<false>,
1 k_consensus<true>, 2 k_consensus_q4, 3 k_consensus_qf followed by k_consensus_q4 on what it flagged, 4 k_consensus_code)
and "consensus_vote_passes" (1 + the runs repeated for a longer boundary list).  Every case is the smallest input that
takes its route; strings are compared with the oracle as in tests/test_gpu_consensus.py."""
import numpy as np
import pytest

from tests.encodings import BY_NAME, draw_quals

pytestmark = pytest.mark.gpu

SCORES = (0, -1, -5, -1, 100)


def _route():
    from sarlacc_amd import _lib
    return int(_lib.stage_count("consensus_route")), int(_lib.stage_count("consensus_vote_passes"))


def _same(got, want):
    assert list(got[0]) == list(want[0]), "consensus strings differ"
    assert list(got[1]) == list(want[1]), "Phred strings differ"


def _clean_groups(table, seed=31, ngroups=2, nrows=3, width=8):
    """Gap-free groups of A, C, G, T with qualities inside the table: nothing k_consensus_qf would flag."""
    rng = np.random.default_rng(seed)
    alns = [["".join(rng.choice(list("ACGT"), width)) for _ in range(nrows)] for _ in range(ngroups)]
    quals = [draw_quals(table, [width] * nrows, seed + g, hi=len(table) - 1) for g in range(ngroups)]
    return alns, quals


def _quality_loop(oracle, table, alns, quals, generic=0):
    from sarlacc_amd import calls
    try:
        calls.set_option("consensus_generic", generic)
        got = calls.create_consensus_quality_loop(alns, 0.6, quals, table.enc)
        route = _route()
    finally:
        calls.set_option("consensus_generic", 0)
    _same(got, oracle.create_consensus_quality_loop(alns, 0.6, quals, table.oenc))
    return route


def test_basic_loop(oracle):
    from sarlacc_amd import calls
    aln = [["ACG", "AGG"]]
    _same(calls.create_consensus_basic_loop(aln, 0.6, 1.0), oracle.create_consensus_basic_loop(aln, 0.6, 1.0))
    assert _route() == (0, 1)


def test_quality_with_log_errors(oracle):
    """The one-column kernel is the only one that returns the per-column log errors."""
    from sarlacc_amd import calls
    table = BY_NAME["phred"]
    alns, quals = _clean_groups(table)
    got = calls.create_consensus_quality(alns[0], 0.6, quals[0], table.enc)
    want = oracle.create_consensus_quality(alns[0], 0.6, quals[0], table.oenc)
    assert _route() == (1, 1)
    assert got[0] == want[0] and np.allclose(got[1], want[1], rtol=1e-11, atol=1e-300)


def test_quality_loop_fast_and_generic(oracle):
    table = BY_NAME["phred"]
    alns, quals = _clean_groups(table)
    assert _quality_loop(oracle, table, alns, quals) == (3, 1)
    assert _quality_loop(oracle, table, alns, quals, generic=1) == (2, 1)


@pytest.mark.parametrize("name", ["n60_high", "n128_high"])
def test_quality_loop_tables_the_fast_kernel_cannot_index(oracle, name):
    """k_consensus_qf takes the first name and the first name + entries as bytes 0..255 and at most 127 entries: a table
    whose names start at or above byte 128 (n60_high: short enough otherwise) or that is longer goes to k_consensus_q4."""
    table = BY_NAME[name]
    alns, quals = _clean_groups(table)
    assert _quality_loop(oracle, table, alns, quals) == (2, 1)


def test_row_count_at_the_lds_limit_of_q4(oracle):
    """k_consensus_q4 keeps its 32-byte vectors (5 n + 1 of them) and four alignments' row records (4 x 28 bytes a row)
    in 48 KB of LDS: the deepest alignment that fits takes it (after k_consensus_qf has flagged it: more than 64 rows),
    one row more takes the one-column kernel."""
    table = BY_NAME["phred"]
    r = (49152 - 16 - 32 * (5 * len(table) + 1)) // 112
    assert r > 64
    for nrows, want in ((r, 3), (r + 1, 1)):
        alns, quals = _clean_groups(table, seed=37, ngroups=1, nrows=nrows, width=5)
        assert _quality_loop(oracle, table, alns, quals) == (want, 1), nrows


def _fused_case(table, seed=41):
    rng = np.random.default_rng(seed)
    reads, groups = [], []
    for g in range(2):
        truth = rng.choice(list("ACGT"), 20)
        for _ in range(3):
            r = truth.copy()
            r[int(rng.integers(20))] = rng.choice(list("ACGT"))
            reads.append("".join(r))
        groups.append([3 * g + 1, 3 * g + 2, 3 * g + 3])
    return reads, groups, draw_quals(table, [20] * 6, seed, hi=len(table) - 1)


def _fused(oracle, table, chars=0):
    from sarlacc_amd import calls
    from sarlacc_amd.strset import csr_from_lists
    reads, groups, quals = _fused_case(table)
    goff, gvals = csr_from_lists(groups)
    try:
        calls.set_option("consensus_chars", chars)
        got = calls.msa_consensus_flat(goff, gvals, reads, *SCORES, 0.6, quals=quals, encoding=table.enc)
        route = _route()
    finally:
        calls.set_option("consensus_chars", 0)
    rows = oracle.quick_msa(groups, reads, *SCORES)
    want = oracle.create_consensus_quality_loop(rows, 0.6, [[quals[i - 1] for i in g] for g in groups], table.oenc)
    _same([got[0].to_strings(), got[1].to_strings()], want)
    return route


def test_fused_call_votes_on_codes(oracle):
    table = BY_NAME["phred"]
    assert _fused(oracle, table) == (4, 1)
    assert _fused(oracle, table, chars=1) == (3, 1)


@pytest.mark.parametrize("name,want", [("n149_wrap", 4), ("n150_wrap", 2), ("n256", 2)])
def test_fused_call_tables_past_byte_255(oracle, name, want):
    """Tables whose first name + entries exceeds 255 when the names are read as bytes (200 + 149, 200 + 150, 128 + 256).
    The library reads the first name as the reference does, as a signed char (-56, -56, -128), and a table that passes
    the reference's check never exceeds 255 that way; what keeps a table from the vote codes is its strip table in LDS
    (1 KB per entry and a zero row, at most 150 KB): 149 entries take k_consensus_code, 150 and 256 the characters --
    and there, longer than 127 entries, k_consensus_q4."""
    assert _fused(oracle, BY_NAME[name]) == (want, 1)


def test_alignment_too_deep_for_the_kernel():
    """The one-column kernel keeps 28 bytes per row of the deepest alignment in LDS: 28 x 5 851 + 16 > 160 KB is refused
    before anything is launched."""
    from sarlacc_amd import SarlaccError, calls
    with pytest.raises(SarlaccError, match="does not fit the consensus kernel"):
        calls.create_consensus_basic_loop([["AC"] * 5851], 0.6, 1.0)
