"""The graphs of tests/umi_cluster_cases.py hold what they claim: the oracle's literal form, its heap form and the plain
Python restatement of the greedy rule agree on every one of them, the result is the closed form where the builder
gives one, the lists are symmetric and name no node twice, and each case sits on the path it is named for (a case that
misses its path would let a wrong kernel pass).  No GPU."""
import numpy as np
import pytest

from tests import umi_cluster_cases as K


def as_lists(clusters):
    return [[int(v) for v in c] for c in clusters]


def restated(c):
    """(clusters, counts at each pick) of the Python restatement; None past the size at which it gets slow"""
    if c.nlinks > K.RESTATEMENT_MAX_LINKS:
        return None, None
    counts = []
    return K.greedy(c.links, counts), counts


@pytest.mark.parametrize("name", K.SPARSE_NAMES + K.DENSE_NAMES)
def test_oracle_forms_restatement_and_closed_form_agree(oracle, name):
    c = K.case(name)
    literal = as_lists(oracle.cluster_umis_test(c.links))
    assert as_lists(oracle.cluster_umis_test(c.links, fast=True)) == literal
    plain, _ = restated(c)
    assert plain is None or plain == literal
    assert c.expect is None or c.expect == literal
    assert sorted(v for clu in literal for v in clu) == list(range(1, c.n + 1))   # every node once


@pytest.mark.parametrize("name", K.SPARSE_NAMES + K.DENSE_NAMES)
def test_lists_are_symmetric_and_hold_each_node_once(name):
    c = K.case(name)
    src = np.repeat(np.arange(1, c.n + 1, dtype=np.int64), [len(l) for l in c.links])
    dst = np.concatenate([np.asarray(l, dtype=np.int64) for l in c.links])
    assert dst.min() >= 1 and dst.max() <= c.n
    forth, back = np.sort(src * (c.n + 1) + dst), np.sort(dst * (c.n + 1) + src)
    assert np.array_equal(forth, back)                        # symmetric
    assert np.all(np.diff(forth) > 0)                         # no node twice in a list
    assert np.count_nonzero(src == dst) == c.n                # every list holds its own node


@pytest.mark.parametrize("name", K.SPARSE_NAMES + K.DENSE_NAMES)
def test_case_reaches_its_path(name):
    c = K.case(name)
    # links per node on the stated side of the switch between a thread and a wavefront per node
    assert c.dense == (name in K.DENSE_NAMES)
    assert (c.nlinks >= 24 * c.n) == c.dense
    counts = sorted((len(l) for l in c.links), reverse=True)
    if "ties" in c.facts:                                     # the tie cases really tie
        assert counts.count(counts[0]) == c.facts["ties"], (counts[:5], c.facts["ties"])
    _, picked = restated(c)
    if "pick_counts" in c.facts and picked is not None:       # ... and every later pick carries the count it is built for
        assert picked == c.facts["pick_counts"]
    if c.expect is not None and picked is not None:
        assert len(picked) + sum(len(l) == 1 for l in c.links) == len(c.expect)


def test_paths_pick_one_node_after_the_other():
    for n in K.PATH_SIZES:
        c, counts = K.case("path-%d" % n), []
        clusters = K.greedy(c.links, counts)
        assert len(clusters) == -(-n // 3) and [len(x) for x in clusters[:n // 3]] == [3] * (n // 3)
        # the seeds walk down the path three at a time, each two hops from the one before and blocked by it until then
        assert [sorted(x) for x in clusters[:n // 3]] == [[s - 1, s, s + 1] for s in range(n - 1, 1, -3)]
        assert counts[:n // 3] == [3] * (n // 3)


def test_threshold_cliques_straddle_the_switch():
    assert not K.case("clique-23").dense and K.case("clique-24").dense and K.case("clique-25").dense
    assert K.case("clique-23").nlinks == 23 * 23 and K.case("clique-24").nlinks == 24 * 24


def test_orphans_end_with_a_count_of_one():
    c, counts = K.case("orphans"), []
    clusters = K.greedy(c.links, counts)
    solos, orph = c.facts["solos"], c.facts["orphans"]
    assert [len(l) for l in c.links].count(1) == solos and clusters[:solos] == sorted(clusters[:solos])
    assert counts[-orph:] == [1] * orph and all(len(x) == 1 for x in clusters[-orph:])
    last = [x[0] for x in clusters[-orph:]]
    assert last == sorted(last, reverse=True) and all(len(c.links[v - 1]) == 3 for v in last)
    # solo and orphan indices alternate
    single = sorted([x[0] for x in clusters[:solos]] + last)
    assert [v in last for v in single] == [k % 2 == 1 for k in range(solos + orph)]


def test_staircase_hubs_sit_one_decrement_from_a_reorder():
    c, counts = K.case("staircase-12"), []
    K.greedy(c.links, counts)
    assert counts[:1 + 2 * 11] == c.facts["pick_counts"]
    # X_j is picked one above hub j (a missed decrement ties them), hub j one above hub j - 1 + 2 (a doubled one swaps them)
    hubs, lone = counts[2:23:2], counts[1:23:2]
    assert [x - h for x, h in zip(lone, hubs)] == [1] * 11
    assert [a - b for a, b in zip(hubs, hubs[1:])] == [3] * 10


def test_three_blocks_second_pick_walks_a_mostly_dead_list():
    c = K.case("three-blocks")
    first, second = c.expect
    assert sorted(first) == list(range(61, 221)) and sorted(second) == list(range(1, 61))
    dead = [k for k, v in enumerate(c.links[59]) if v > 60]
    assert len(c.links[59]) == 100 and len(dead) == 40
    assert any(k < 64 for k in dead) and any(k >= 64 for k in dead)            # in both chunks
    assert any(k >= 64 and c.links[59][k] <= 60 for k in range(100))            # a live entry behind the first chunk


def test_equal_large_cliques_fill_most_of_the_candidate_list():
    c = K.case("large-cliques-30x30")
    assert c.facts["ties"] == 900 < K.candidate_capacity(c.n)
    assert [max(x) for x in c.expect] == list(range(900, 0, -30))


@pytest.mark.parametrize("name", ["cut-off", "cut-off-bridge"])
def test_cut_off_has_more_top_nodes_than_the_candidate_list_holds(name):
    c = K.case(name)
    assert c.facts["ties"] == 1025 > K.candidate_capacity(c.n) == 1024
    assert [len(x) for x in c.expect] == ([1025, 41, 29] if name == "cut-off-bridge" else [1025, 40, 30])


def test_wheels_first_window_is_all_picks_and_the_second_nearly_none(oracle):
    c = K.case("wheels")
    assert c.n == 8 * 401 + 300 + 40 and c.nlinks == 8 * (401 + 400 * 201) + 300 * 300 + 40 * 40
    sizes = sorted((len(l) for l in c.links), reverse=True)
    assert sizes[:8] == [401] * 8 and sizes[8:308] == [300] * 300 and sizes[308] == 201
    # round one: 8 candidates, 8 picks (4 * picks >= candidates: wider); round two: 300 candidates above 256, one pick
    # (64 * picks < candidates: narrower); a third round follows, in which the control block gets to see the second
    assert [len(x) for x in c.expect] == [401] * 8 + [300, 40]
    hubs = [x[[len(c.links[v - 1]) for v in x].index(401)] for x in c.expect[:8]]
    assert hubs == sorted(hubs, reverse=True)


@pytest.mark.parametrize("count", K.BOUNDARY_CLIQUES)
def test_distinct_cliques_give_one_clique_per_window(count):
    c = K.case("distinct-cliques-%d" % count)
    sizes = [len(x) for x in c.expect]
    assert sizes == list(range(23 + count, 23, -1))
    # a window of delta = 0 holds the largest clique alone: one pick among 24 or more candidates, never a quarter of
    # them (no wider), and never more than 256 candidates (no narrower)
    assert all(4 * 1 < s <= 256 for s in sizes)
    assert count % K.CL_GROUP in (K.CL_GROUP - 1, 0, 1)


# ---------------------------------------------------------------------------
# pre-groups

def per_group_restated(oracle, umis, groups, limit):
    """umi_group from its parts: the oracle's neighbour lists of each pre-group, the restated greedy rule, the members'
    read indices"""
    out = []
    for g in groups:
        if len(g) == 1:
            out.append(list(g))
            continue
        lists = [[int(v) for v in l] for l in oracle.fast_levdist_test([umis[r - 1] for r in g], limit)]
        out += [[g[v - 1] for v in clu] for clu in K.greedy(lists)]
    return out


@pytest.mark.parametrize("ngroups", K.PREGROUP_COUNTS)
def test_pregroup_sets(oracle, ngroups):
    umis, groups = K.pregroups(ngroups)
    assert len(groups) == ngroups and all(1 <= len(g) <= 6 for g in groups) and all(len(u) == 8 for u in umis)
    assert sorted(r for g in groups for r in g) == list(range(1, len(umis) + 1))
    if ngroups >= 3:
        assert all(len(g) == 1 for g in groups[::3]) and all(len(g) > 1 for g in groups[1::3])   # single reads in between
        assert sum(g != sorted(g) for g in groups) > ngroups // 4                                # unsorted
        assert sum(max(g) - min(g) >= len(g) for g in groups if len(g) > 1) >= ngroups // 2       # not contiguous
    literal = as_lists(oracle.umi_group(umis, 1, None, 1, groups))
    assert as_lists(oracle.umi_group(umis, 1, None, 1, groups, fast=True)) == literal
    assert per_group_restated(oracle, umis, groups, 1) == literal
    assert len(literal) > ngroups or ngroups < 255        # some groups split


def test_dense_pregroup_set(oracle):
    umis, groups = K.dense_pregroup()
    assert len(groups) == 301 and len(groups[150]) == 350 and all(len(g) <= 3 for k, g in enumerate(groups) if k != 150)
    big = [umis[r - 1] for r in groups[150]]
    a, b = sorted(set(big))
    assert sum(x != y for x, y in zip(a, b)) == 1 and sorted((big.count(a), big.count(b))) == [150, 200]
    assert 350 * 350 >= 24 * len(umis)     # the links of the large pre-group alone put the whole call past the switch
    literal = as_lists(oracle.umi_group(umis, 1, None, 1, groups))
    assert as_lists(oracle.umi_group(umis, 1, None, 1, groups, fast=True)) == literal
    assert per_group_restated(oracle, umis, groups, 1) == literal
    assert [len(x) for x in literal].count(350) == 1
