"""GPU parity of the consensus vote where its floating-point decisions are close: the families of
tests/consensus_columns.py through every route, against the oracle.  Consensus and Phred strings must be identical; the
log errors of the one route that returns them within 1e-11 relative.

Routes: (1) create_consensus_quality -- k_consensus<true>; (2) create_consensus_quality_loop -- k_consensus_qf, with
groups it hands to k_consensus_q4 in the same call; (3) the same with consensus_generic = 1 -- k_consensus_q4 alone;
(4) msa_consensus_flat -- k_consensus_code; (5) the same with consensus_chars = 1; (6) create_consensus_basic and
_basic_loop -- k_consensus<false>.  The alignments of routes 4 and 5 are gap-free reads that the oracle's MSA returns
unchanged (asserted in tests/test_oracle_consensus_columns.py), so the expected value is the oracle's vote on them."""
import numpy as np
import pytest

from tests import consensus_columns as K

pytestmark = pytest.mark.gpu


def _first_difference(got, want):
    for g, (a, b) in enumerate(zip(got, want)):
        if a != b:
            at = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
            return "group %d, column %d: got %r, want %r (lengths %d, %d)" % (g, at, a[at:at + 1], b[at:at + 1], len(a), len(b))
    return "%d groups against %d" % (len(got), len(want))


def _same(got, want, what):
    got, want = [list(got[0]), list(got[1])], [list(want[0]), list(want[1])]
    assert got[0] == want[0], "%s: consensus strings differ: %s" % (what, _first_difference(got[0], want[0]))
    assert got[1] == want[1], "%s: Phred strings differ: %s" % (what, _first_difference(got[1], want[1]))


def _vote_passes(passes, what):
    """passes (None: not checked): how often the vote of the last call ran -- 1 + the runs repeated for a longer boundary list"""
    from sarlacc_amd import _lib
    if passes is not None:
        assert _lib.stage_count("consensus_vote_passes") == passes, what


def quality_routes(oracle, alns, quals, table, mincov=0.6, single=True, handover=True, fused=None, what="", passes=None):
    """Routes 1 to 5 on the alignments `alns` under the encoding table (errors, names).  handover: two more groups in
    the loop calls that k_consensus_qf hands to k_consensus_q4.  fused: (alignments, qualities) of gap-free rows for
    routes 4 and 5.  passes: the vote passes every one of the calls must have taken."""
    from sarlacc_amd import calls
    from sarlacc_amd.encoding import Encoding
    enc = Encoding(*table)
    if single:
        for g, (a, q) in enumerate(zip(alns, quals)):
            want = oracle.create_consensus_quality(a, mincov, q, table)
            got = calls.create_consensus_quality(a, mincov, q, enc)
            _vote_passes(passes, "%s route 1, group %d" % (what, g))
            assert got[0] == want[0], "%s route 1, group %d: %s" % (what, g, _first_difference([got[0]], [want[0]]))
            assert np.allclose(got[1], want[1], rtol=1e-11, atol=1e-300), (what, g)
    alns, quals = list(alns), list(quals)
    if handover:
        ea, eq = K.handover_extras(alns[0], quals[0])
        alns, quals = alns[:1] + ea[:1] + alns[1:] + ea[1:], quals[:1] + eq[:1] + quals[1:] + eq[1:]
    want = oracle.create_consensus_quality_loop(alns, mincov, quals, table)
    try:
        for generic in (0, 1):
            calls.set_option("consensus_generic", generic)
            _same(calls.create_consensus_quality_loop(alns, mincov, quals, enc), want, "%s route %d" % (what, 2 + generic))
            _vote_passes(passes, "%s route %d" % (what, 2 + generic))
        calls.set_option("consensus_generic", 0)
        if fused is not None:
            want = oracle.create_consensus_quality_loop(fused[0], mincov, fused[1], table)
            goff, gvals, reads = K.flat_groups(fused[0])
            rquals = [q for qs in fused[1] for q in qs]
            for chars in (0, 1):
                calls.set_option("consensus_chars", chars)
                got = calls.msa_consensus_flat(goff, gvals, reads, *K.DEFAULT_SCORES, mincov, quals=rquals, encoding=enc)
                _vote_passes(passes, "%s route %d" % (what, 4 + chars))
                _same([got[0].to_strings(), got[1].to_strings()], want, "%s route %d" % (what, 4 + chars))
    finally:
        calls.set_option("consensus_generic", 0)
        calls.set_option("consensus_chars", 0)


# ---------------------------------------------------------------------------
# Family A

@pytest.mark.parametrize("n,odd", [(n, False) for n in K.A_ROWS] + [(n, True) for n in K.A_ROWS_ODD])
def test_engineered_boundaries(oracle, n, odd):
    """Every Phred level's boundary at every offset: both sides of the host window (1e-9) and of the windows inside
    which k_consensus_q4 (2e-4) and k_consensus_qf / k_consensus_code (4e-4) leave their fp32 estimate."""
    for delta in K.DELTAS:
        rows, quals, table, _, _ = K.boundary_alignment(n, delta, odd)
        quality_routes(oracle, [rows], [quals], table, fused=([rows], [quals]), what="n %d odd %d delta %g" % (n, odd, delta))


def test_engineered_boundaries_basic(oracle):
    from sarlacc_amd import calls
    for n, k in K.BASIC_PAIRS:
        aln = K.basic_alignment(n)
        other = K.basic_alignment(n + 1, 23)
        for delta in K.DELTAS:
            pc = K.basic_pseudo_count(n, k + 0.5 + delta)
            want = oracle.create_consensus_basic(aln, 0.6, pc)
            got = calls.create_consensus_basic(aln, 0.6, pc)
            assert got[0] == want[0]
            assert np.allclose(got[1], want[1], rtol=1e-11, atol=0), (n, k, delta)
            _same(calls.create_consensus_basic_loop([aln, other], 0.6, pc), oracle.create_consensus_basic_loop([aln, other], 0.6, pc),
                  "basic n %d level %d delta %g" % (n, k, delta))


# ---------------------------------------------------------------------------
# Family B

@pytest.mark.parametrize("n", K.B_ROWS)
def test_searched_boundaries(oracle, n):
    alns, quals = K.searched_alignments(n)
    quality_routes(oracle, alns, quals, K.phred_table(), fused=K.searched_fused(n), what="searched, %d rows" % n)


# ---------------------------------------------------------------------------
# Family C

@pytest.mark.parametrize("n", K.C_ROWS)
def test_near_ties(oracle, n):
    """The base of a column whose two largest sums hold the same addends: the order of the additions and the
    first-maximum rule decide.  More than 64 rows: k_consensus_q4 inside the default call; 400 rows: the one-column
    kernel (the call's deepest alignment decides)."""
    rows, quals = K.tie_alignment(n)
    quality_routes(oracle, [rows], [quals], K.phred_table(), handover=n <= 64, what="ties, %d rows" % n)


def test_near_ties_fused(oracle):
    alns, quals = K.tie_fused()
    quality_routes(oracle, alns, quals, K.phred_table(), single=False, fused=(alns, quals), what="ties, fused", passes=1)


# ---------------------------------------------------------------------------
# Family D

@pytest.fixture(scope="module")
def coverage_expected(oracle):
    """(rows, minimum coverage) -> the oracle's (consensus, Phred string) of the quality vote and of the basic vote"""
    table = K.phred_table()
    out = {}
    for n in K.D_ROWS:
        rows, quals = K.coverage_alignment(n)
        for v in K.coverage_values(n):
            cq, eq = oracle.create_consensus_quality(rows, v, quals, table)
            cb, eb = oracle.create_consensus_basic(rows, v, 1.0)
            out[n, v] = (cq, eq, oracle.errors_to_string(eq)), (cb, eb, oracle.errors_to_string(eb))
    return out


@pytest.mark.parametrize("route", ["quality", "basic"])
def test_coverage_products_single(coverage_expected, enc, route):
    """routes 1 and 6 (single alignment): one call per (rows, minimum coverage)"""
    from sarlacc_amd import calls
    for (n, v), (wq, wb) in coverage_expected.items():
        rows, quals = K.coverage_alignment(n)
        if route == "quality":
            got, want = calls.create_consensus_quality(rows, v, quals, enc), wq
        else:
            got, want = calls.create_consensus_basic(rows, v, 1.0), wb
        assert got[0] == want[0], (route, n, v)
        assert np.allclose(got[1], want[1], rtol=1e-11, atol=1e-300), (route, n, v)


@pytest.mark.parametrize("route", ["qf", "qf_to_q4", "q4", "basic"])
def test_coverage_products_loop(oracle, oenc, coverage_expected, enc, route):
    """routes 2, 3 and 6 (loop): one call per minimum coverage, with every row count whose set holds it.  qf: the
    alignments without their columns of N, so that k_consensus_qf keeps the groups of up to 64 rows; qf_to_q4: with
    them, every group handed over."""
    from sarlacc_amd import calls
    try:
        calls.set_option("consensus_generic", int(route == "q4"))
        for v, ns in K.coverage_batches().items():
            alns = [K.coverage_alignment(n)[0] for n in ns]
            if route == "qf":
                alns, quals = [K.coverage_alignment(n, False)[0] for n in ns], [K.coverage_alignment(n, False)[1] for n in ns]
                got = calls.create_consensus_quality_loop(alns, v, quals, enc)
                want = oracle.create_consensus_quality_loop(alns, v, quals, oenc)
            elif route == "basic":
                got = calls.create_consensus_basic_loop(alns, v, 1.0)
                want = [[coverage_expected[n, v][1][0] for n in ns], [coverage_expected[n, v][1][2] for n in ns]]
            else:
                got = calls.create_consensus_quality_loop(alns, v, [K.coverage_alignment(n)[1] for n in ns], enc)
                want = [[coverage_expected[n, v][0][0] for n in ns], [coverage_expected[n, v][0][2] for n in ns]]
            _same(got, want, "coverage %r, %s, rows %r" % (v, route, ns))
    finally:
        calls.set_option("consensus_generic", 0)


@pytest.fixture(scope="module")
def coverage_msa_rows(oracle):
    """rows -> (the oracle's MSA rows of coverage_reads(rows), the reads' qualities)"""
    rows = {}
    for n in K.D_ROWS:
        if n <= 64:
            reads, quals = K.coverage_reads(n)
            rows[n] = oracle.quick_msa([list(range(1, n + 1))], reads, *K.DEFAULT_SCORES)[0], quals
    return rows


@pytest.mark.parametrize("part", range(4))
@pytest.mark.parametrize("chars", [0, 1])
def test_coverage_products_fused(oracle, oenc, enc, coverage_msa_rows, chars, part):
    """routes 4 and 5: reads whose MSA rows have gaps, up to 64 per group; expected: the oracle's vote on the oracle's
    rows.  One call per minimum coverage (some 1 300 of them, dealt to four parts)."""
    from sarlacc_amd import calls
    rows = coverage_msa_rows
    try:
        calls.set_option("consensus_chars", chars)
        for v, ns in list(K.coverage_batches().items())[part::4]:
            ns = [n for n in ns if n <= 64]
            if not ns:
                continue
            want = oracle.create_consensus_quality_loop([rows[n][0] for n in ns], v, [rows[n][1] for n in ns], oenc)
            goff, gvals, reads = K.flat_groups([K.coverage_reads(n)[0] for n in ns])
            rquals = [q for n in ns for q in K.coverage_reads(n)[1]]
            got = calls.msa_consensus_flat(goff, gvals, reads, *K.DEFAULT_SCORES, v, quals=rquals, encoding=enc)
            _same([got[0].to_strings(), got[1].to_strings()], want, "coverage %r, fused, rows %r" % (v, ns))
    finally:
        calls.set_option("consensus_chars", 0)


# ---------------------------------------------------------------------------
# Family E

def test_boundary_flood_basic(oracle):
    """6 000 columns on 20.5 in one alignment, and dealt to 40 alignments of one call: more than the boundary list
    holds at first, so the vote runs a second time with a list of the exact size."""
    from sarlacc_amd import calls
    rows, pc = K.flood_basic()
    want = oracle.create_consensus_basic(rows, 0.6, pc)
    got = calls.create_consensus_basic(rows, 0.6, pc)
    _vote_passes(2, "flood, basic, single")
    assert got[0] == want[0]
    assert np.allclose(got[1], want[1], rtol=1e-11, atol=0)
    alns, _ = K.split_groups(rows, rows)
    for batch in ([rows], alns):
        _same(calls.create_consensus_basic_loop(batch, 0.6, pc), oracle.create_consensus_basic_loop(batch, 0.6, pc), "flood, basic")
        _vote_passes(2, "flood, basic, %d groups" % len(batch))


def test_boundary_flood_quality(oracle):
    """The same for the quality vote on 25.5, through routes 1 to 5: whole, and dealt to 40 groups of which every
    third has an N in its last column -- k_consensus_qf has listed such a group's columns by the time it meets the N and
    hands the group to k_consensus_q4, which lists them again: the first entries are void, under a grown list too."""
    rows, quals, table = K.flood_quality()
    quality_routes(oracle, [rows], [quals], table, fused=([rows], [quals]), what="flood, whole", passes=2)
    alns, qs = K.split_groups(rows, quals)
    quality_routes(oracle, alns, qs, table, single=False, handover=False, fused=(alns, qs), what="flood, 40 groups", passes=2)
    mixed = [K.with_n(a) if g % 3 == 0 else a for g, a in enumerate(alns)]
    assert sum(len(a[0]) for a in mixed) - len(mixed[::3]) > 4096
    quality_routes(oracle, mixed, qs, table, single=False, handover=False, what="flood, hand-over", passes=2)
