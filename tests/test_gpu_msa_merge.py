"""Which paths of the merge of MSA spec v2 ran (sarlacc_amd/csrc/msa2.hip, k_m2_group), shown by the library's counters on inputs
built to reach them (tests/msa_merge_cases.py; tests/test_oracle_msa2_merge.py asserts on the CPU statement alone that they do):

  * the chain over the LDS ring given up in the middle of a join and redone over all columns in HBM (m2_chain_forward<true>
    returning false with part of pred[] written), beside joins of the same launch that stay in the ring;
  * a profile that outgrows the first-pass capacity by one column (m2_renumber returning -1), the group done again in a second
    pass with exact capacity, its rows put back in the caller's order; one that meets the capacity exactly; the column ceiling;
  * joins without a single match;
  * groups on the class boundaries of the launch (12 | 13, 24 | 25, 32 | 33 reads) with profiles of 1 to 130 columns, where the
    device's counters of the two row rules must equal the CPU statement's.

Every test compares the rows with oracle/msa2.c character for character and checks that each row spells its read.  Every call
prints its counters (pytest -s) before anything is asserted on them."""
import numpy as np
import pytest

from tests import msa_merge_cases as M

pytestmark = pytest.mark.gpu

COUNTERS = ("msa2_joins", "msa2_joins_chain_in_hbm", "msa2_groups_second_pass", "msa2_rows", "msa2_rows_capped",
            "msa2_entries_filtered", "msa2_rows_filtered", "msa2_entries_kept", "msa2_batches", "msa_v1_fallback", "msa_v1_fallback_too_wide")
# device counter -> statistic of the CPU statement (equal whenever no group was done twice)
SAME_AS_ORACLE = (("msa2_joins", "joins"), ("msa2_rows", "rows"), ("msa2_rows_capped", "rows_capped"), ("msa2_entries_filtered", "entries_filtered"),
                  ("msa2_rows_filtered", "rows_filtered"), ("msa2_entries_kept", "entries_kept"))


@pytest.fixture(autouse=True)
def spec2():
    from sarlacc_amd import calls
    calls.set_msa_spec(2)
    yield
    calls.set_msa_spec(0)


def run(what, read_groups, params, options=()):
    """calls.quick_msa under `options` -> (rows, counters of the call)"""
    from sarlacc_amd import _lib, calls
    reads, groups = M.flatten(read_groups)
    for name, val in options:
        calls.set_option(name, val)
    try:
        got = calls.quick_msa(groups, reads, *params)
        c = {n: int(_lib.stage_count(n)) for n in COUNTERS}
    finally:
        for name, _ in options:
            calls.set_option(name, 0)
    print("counters", what, dict(options), c)
    return got, c


def check(oracle, key, read_groups, params, options=(), max_columns=65535):
    """rows of the call equal the CPU statement's and spell their reads -> (rows, counters, statistics of the CPU statement)"""
    want, st = M.reference(oracle, key, read_groups, params, max_columns)
    got, c = run(key, read_groups, params, options)
    assert len(got) == len(want)
    for g, (a, b) in enumerate(zip(got, want)):
        assert a == b, "group %d differs (%r, %r)" % (g, key, dict(options))
    reads, groups = M.flatten(read_groups)
    M.rows_spell(got, reads, groups)
    return got, c, st


# ---- the chain: ring given up mid-join and redone in HBM ----

def ring_groups(taken):
    far = [M.split(600), M.split(600, extra=1), M.split(560, prefix=330)] if taken else []
    return far + [M.split(400), M.ordinary(1), M.ordinary(2)]


def test_chain_ring_given_up_mid_join_and_not(oracle):
    """split(600), its four-read variant and a split behind a common prefix of 330 bases (the ring is given up five blocks of
    matches into the join, with predecessors written and columns entered) beside split(400) and two ordinary clusters in one
    call: the joins whose rows reach 510 columns or more behind the front start in the ring, give it up and are redone in HBM;
    the others of the same launch stay in the ring.  The counter lies between the CPU statement's two bounds (oracle/msa2.c
    MSA2_RING_REACH) -- on these inputs the bounds coincide (4 joins).  Without the far-reaching groups no join leaves the ring."""
    got, c, st = check(oracle, "ring_taken", ring_groups(True), M.DEFAULT)
    print("oracle", {k: st[k] for k in ("joins", "max_row_reach", "max_reach_ahead", "joins_reach_certain", "joins_reach_possible")})
    assert st["joins_reach_certain"] >= 1
    assert st["joins_reach_certain"] <= c["msa2_joins_chain_in_hbm"] <= st["joins_reach_possible"]
    assert c["msa2_joins_chain_in_hbm"] < c["msa2_joins"] == st["joins"]
    assert c["msa2_groups_second_pass"] == 0 and c["msa_v1_fallback"] == 0
    _, c0, st0 = check(oracle, "ring_not_taken", ring_groups(False), M.DEFAULT)
    assert st0["joins_reach_possible"] == 0 and c0["msa2_joins_chain_in_hbm"] == 0 and c0["msa2_joins"] == st0["joins"] > 0


@pytest.mark.parametrize("option", ["msa2_single_wave", "msa2_general_rows", "msa2_chain_hbm"])
def test_chain_ring_given_up_under_the_other_code_paths(oracle, option):
    """The same call with one wavefront per group, with the any-weights row lists, and with the ring never tried: identical rows.
    The first two still start every chain in the ring, so the counter keeps its bounds; under msa2_chain_hbm it counts every join
    that has matches."""
    _, c, st = check(oracle, "ring_taken", ring_groups(True), M.DEFAULT, options=((option, 1),))
    if option == "msa2_chain_hbm":
        assert c["msa2_joins_chain_in_hbm"] == c["msa2_joins"] == st["joins"]   # (no join of this call has an empty match list)
    else:
        assert 1 <= st["joins_reach_certain"] <= c["msa2_joins_chain_in_hbm"] <= st["joins_reach_possible"] < c["msa2_joins"]


def test_chain_ring_given_up_in_the_multi_wavefront_classes(oracle):
    """split(600) with 22 and with 31 further copies of U + V: groups of 25 and of 34 reads, merged by workgroups of eight and of
    four wavefronts (the second with 64-bit member sets), where the match list of a join comes in one segment per wavefront.
    split(400) beside them stays in the ring."""
    read_groups = [M.split(600, extra=22), M.split(400), M.split(600, extra=31)]
    _, c, st = check(oracle, "ring_wide_groups", read_groups, M.DEFAULT)
    print("oracle", {k: st[k] for k in ("joins", "max_row_reach", "max_reach_ahead", "joins_reach_certain", "joins_reach_possible")})
    assert 2 <= st["joins_reach_certain"] <= c["msa2_joins_chain_in_hbm"] <= st["joins_reach_possible"] < c["msa2_joins"] == st["joins"]
    assert c["msa2_groups_second_pass"] == 0 and c["msa_v1_fallback"] == 0
    for dev, orc in SAME_AS_ORACLE:
        assert c[dev] == st[orc], (dev, c[dev], orc, st[orc])


# ---- the row rules and the counters on the class boundaries ----

@pytest.mark.parametrize("sizes", M.SWEEP_CALLS, ids=lambda s: "-".join(map(str, s)))
def test_counters_equal_the_cpu_statement_on_class_boundaries(oracle, sizes):
    """Groups of `sizes` reads of one and of two molecules of 1, 5, 63, 64, 65 and 129 bases (profiles narrower than the 64
    rows of a wavefront's range, so that most wavefronts of the larger classes have no rows; reads of 0 and 1 bases): rows, and
    joins / rows / capped rows / filtered entries and rows / kept entries as the CPU statement counts them."""
    read_groups = [g for size in sizes for _, _, g in M.sweep(size)]
    _, c, st = check(oracle, ("sweep_call", sizes), read_groups, M.DEFAULT)
    print("oracle", {o: st[o] for _, o in SAME_AS_ORACLE})
    assert c["msa_v1_fallback"] == 0
    if c["msa2_groups_second_pass"] == 0:   # (a group done twice counts the joins of its first pass twice)
        for dev, orc in SAME_AS_ORACLE:
            assert c[dev] == st[orc], (dev, c[dev], orc, st[orc])
    if min(sizes) >= 11:   # established on the CPU statement by test_oracle_msa2_merge.py::test_sweep_rows_and_rules
        assert st["rows_capped"] > 0 and st["entries_filtered"] > 0
        assert c["msa2_rows_capped"] > 0 and c["msa2_entries_filtered"] > 0


# ---- profile capacity: met, exceeded by one column, second pass, ceiling ----

@pytest.mark.parametrize("L,second", [(64, 0), (65, 1)])
def test_first_pass_capacity_met_and_exceeded_by_one_column(oracle, L, second):
    """Four homopolymers of L bases under scores that pair nothing: 4 L columns against min(4 L, 3 L + 64) of the first pass."""
    got, c, st = check(oracle, ("homopolymers", L), [M.homopolymers(L)], M.GAPS_ONLY)
    assert len(got[0][0]) == 4 * L
    assert c["msa2_groups_second_pass"] == second and c["msa_v1_fallback"] == 0
    if not second:
        for dev, orc in SAME_AS_ORACLE:
            assert c[dev] == st[orc], (dev, orc)


def overflow_call():
    return [M.ordinary(3), M.six_read_overflow(), M.ordinary(4)]


@pytest.mark.parametrize("batches", [0, 3])
def test_second_pass_rows_in_caller_order(oracle, batches):
    """A six-read group that outgrows its first-pass capacity in the middle of its tree (449 columns against 364), between two
    ordinary clusters: it alone takes the second pass and its rows come back between theirs; the same in three batches."""
    got, c, st = check(oracle, "six+ordinary", overflow_call(), M.GAPS_ONLY, options=(("msa2_batches", batches),) if batches else ())
    assert c["msa2_groups_second_pass"] == 1 and c["msa_v1_fallback"] == 0
    assert len(got[1][0]) > 3 * 100 + 64 and [len(g) for g in got] == [6, 6, 6]
    if batches:
        assert c["msa2_batches"] >= 3
    # the first pass counted the group's joins up to the one that overflowed, 1 to 5 of them, and the second pass all 5 again
    assert st["joins"] + 1 <= c["msa2_joins"] <= st["joins"] + 5


@pytest.mark.parametrize("chars", [0, 1], ids=["vote_codes", "consensus_chars"])
def test_second_pass_in_the_fused_call(chars):
    """The same call through msa_consensus_flat (rows stay in HBM, as 16-bit vote codes or as characters) against quick_msa_flat
    followed by create_consensus_flat."""
    import sarlacc_amd
    from sarlacc_amd import _lib, calls
    from sarlacc_amd.strset import StringSet, csr_from_lists
    reads, groups = M.flatten(overflow_call())
    rng = np.random.default_rng(65)
    quals = ["".join(chr(int(q)) for q in rng.integers(40, 90, len(r))) for r in reads]
    goff, gvals = csr_from_lists(groups)
    enc = sarlacc_amd.phred_encoding()
    rows, grp_rows, widths = calls.quick_msa_flat(goff, gvals, reads, *M.GAPS_ONLY)
    assert int(_lib.stage_count("msa2_groups_second_pass")) == 1
    qsub = StringSet.from_strings(quals).subset(gvals[:int(goff[-1])].astype(np.int64) - 1)
    # (minimum coverage 0.1: a column held by one read of six stays, so the consensus of the redone group has all its columns)
    want = calls.create_consensus_flat(rows, grp_rows, 0.1, quals=qsub, encoding=enc)
    calls.set_option("consensus_chars", chars)
    try:
        got = calls.msa_consensus_flat(goff, gvals, reads, *M.GAPS_ONLY, 0.1, quals=quals, encoding=enc)
        second = int(_lib.stage_count("msa2_groups_second_pass"))
    finally:
        calls.set_option("consensus_chars", 0)
    print("counters fused", {"consensus_chars": chars, "msa2_groups_second_pass": second})
    assert second == 1
    assert got[0].to_strings() == want[0].to_strings()
    assert got[1].to_strings() == want[1].to_strings()
    assert len(got[0]) == 3 and len(got[0][1]) == int(widths[1]) > 3 * 100 + 64


@pytest.mark.parametrize("ceiling", [259, 260])
def test_column_ceiling_one_below_and_at_the_width(oracle, ceiling):
    """homopolymers(65) is 260 columns wide: with the ceiling at 259 the second pass cannot hold it either and the group goes to
    spec v1, at 260 it fits -- `msa_v1_fallback_too_wide` as the CPU statement's `max_columns` decides."""
    v2rows, _ = M.reference(oracle, ("homopolymers", 65), [M.homopolymers(65)], M.GAPS_ONLY)
    too_wide = sum(1 for rows in v2rows if len(rows[0]) > ceiling)
    _, c, _ = check(oracle, ("homopolymers", 65, ceiling), [M.homopolymers(65)], M.GAPS_ONLY, options=(("msa2_max_columns", ceiling),),
                    max_columns=ceiling)
    print("oracle", {"max_columns": ceiling, "groups_too_wide": too_wide})
    assert c["msa_v1_fallback_too_wide"] == too_wide
    assert c["msa2_groups_second_pass"] == 1 and c["msa_v1_fallback"] == too_wide


# ---- joins without matches ----

@pytest.mark.parametrize("company", [False, True], ids=["alone", "beside_single_and_empty"])
def test_joins_with_empty_match_lists(oracle, company):
    read_groups = [M.homopolymers(60)] + ([["ACGTTGCA"], []] if company else [])
    got, c, st = check(oracle, ("homopolymers60", company), read_groups, M.GAPS_ONLY)
    assert len(got[0][0]) == 240 and c["msa2_entries_kept"] == 0 and c["msa2_joins"] == 3 == st["joins"]
    assert c["msa2_joins_chain_in_hbm"] == 0 and c["msa2_groups_second_pass"] == 0
    assert c["msa2_rows"] == st["rows"] and c["msa2_rows_capped"] == 0 and c["msa2_entries_filtered"] == 0
    if company:
        assert got[1] == ["ACGTTGCA"] and got[2] == []
