"""The greedy clustering of the UMI stage (umi_cluster.hip, cluster_dev) on graphs built for each of its round schemes.

Exact integer work: the clusters must be the oracle's, list for list and in its order.  The graphs come from
tests/umi_cluster_cases.py (tests/test_umi_cluster_cases.py shows that each reaches what it is named for); the counters
of the last call say which rounds ran:

  a thread per node (k_cl_m1, k_cl_pick, k_cl_decrement)         paths around the 256-thread block (a pick per round),
                                                                  stars (one long list walked by one thread), equal cliques
                                                                  (every key ties), staircase (each pick moves the next
                                                                  count), orphans (counts that fall to 1), 1 and 2 nodes
  a wavefront per node (k_cl_m1_w, k_cl_pick_w, k_cl_decrement_w) every dense case under umi_full_rounds = 1, and the round
                                                                  after a cut-off candidate list
  candidate-set rounds (k_cl_collect .. k_cl_decrement_list)      cliques of 24 and 25 (23 stays on a thread per node), of
                                                                  64, 65, 128, 129 (the 64-lane chunks of a list), three
                                                                  overlapping blocks (a pick past 40 dead entries), 900
                                                                  tied candidates, a cut-off list, the wheels (k_cl_control
                                                                  widens, then narrows), rounds that end on a group of 8
  the group sort of clusters_write                                1 .. 1000 pre-groups through umi_group and umi_group_flat
  the entry point's refusals                                      lists that are no neighbour lists"""
import numpy as np
import pytest

from tests import umi_cluster_cases as K

pytestmark = pytest.mark.gpu

COUNTERS = ("umi_links", "umi_cluster_rounds", "umi_cluster_candidate_rounds", "umi_cluster_full_rounds",
            "umi_cluster_widened", "umi_cluster_narrowed")
_WANT = {}


def as_lists(clusters):
    return [[int(v) for v in c] for c in clusters]


def want(oracle, name):
    """the oracle's clusters of a case, computed once"""
    if name not in _WANT:
        _WANT[name] = as_lists(oracle.cluster_umis_test(K.case(name).links))
    return _WANT[name]


def same_lists(got, ref):
    assert len(got) == len(ref), (len(got), len(ref))
    for k, (x, y) in enumerate(zip(got, ref)):
        assert x == y, (k, x[:40], y[:40], len(x), len(y))


def counters(what):
    from sarlacc_amd import _lib
    n = {k: int(_lib.stage_count(k)) for k in COUNTERS}
    print(what, " ".join("%s=%d" % (k[4:], v) for k, v in n.items()))
    return n


def clustered(links, full=0):
    """(clusters, counters) of one call under `umi_full_rounds` = full"""
    from sarlacc_amd import calls
    try:
        calls.set_option("umi_full_rounds", full)
        got = as_lists(calls.cluster_umis_test(links))
        return got, counters("full_rounds=%d" % full)
    finally:
        calls.set_option("umi_full_rounds", 0)


# ---------------------------------------------------------------------------
# a thread per node

@pytest.mark.parametrize("name", K.SPARSE_NAMES)
def test_thread_per_node_rounds(oracle, name):
    c = K.case(name)
    got, n = clustered(c.links)
    same_lists(got, want(oracle, name))
    assert n["umi_links"] == c.nlinks < 24 * c.n
    assert n["umi_cluster_candidate_rounds"] == n["umi_cluster_widened"] == n["umi_cluster_narrowed"] == 0
    assert n["umi_cluster_full_rounds"] == n["umi_cluster_rounds"]
    if "rounds" in c.facts:
        assert n["umi_cluster_rounds"] == c.facts["rounds"]
    if name.startswith("path-") and c.n > 3:     # (a path of 2 or 3 nodes is one cluster)
        assert n["umi_cluster_rounds"] > 1


# ---------------------------------------------------------------------------
# a wavefront per node, and the candidate-set rounds

@pytest.mark.parametrize("full", [0, 1])
@pytest.mark.parametrize("size", K.THRESHOLD_CLIQUES)
def test_clique_threshold_between_thread_and_wavefront(oracle, size, full):
    # 23 * 23 links on 23 nodes stay on a thread per node; 24 * 24 on 24 are the first on the other side
    name = "clique-%d" % size
    c = K.case(name)
    got, n = clustered(c.links, full)
    same_lists(got, want(oracle, name))
    assert n["umi_links"] == size * size and n["umi_cluster_rounds"] == 1
    if size == 23 or full:
        assert n["umi_cluster_candidate_rounds"] == 0 and n["umi_cluster_full_rounds"] == 1
    else:
        assert n["umi_cluster_candidate_rounds"] > 0 and n["umi_cluster_full_rounds"] == 0


@pytest.mark.parametrize("full", [0, 1])
@pytest.mark.parametrize("name", K.DENSE_NAMES)
def test_dense_rounds(oracle, name, full):
    c = K.case(name)
    got, n = clustered(c.links, full)
    same_lists(got, want(oracle, name))
    assert n["umi_links"] == c.nlinks >= 24 * c.n
    assert n["umi_cluster_rounds"] == n["umi_cluster_candidate_rounds"] + n["umi_cluster_full_rounds"]
    if full:
        assert n["umi_cluster_candidate_rounds"] == n["umi_cluster_widened"] == n["umi_cluster_narrowed"] == 0
        assert n["umi_cluster_rounds"] == c.facts["rounds_full"]
        return
    assert n["umi_cluster_candidate_rounds"] >= 1
    if name.startswith("cut-off"):
        # the cut-off list counts as a candidate round, the round over every list runs in its place; with the bridge a
        # candidate round follows for the 29 nodes that round had to leave
        assert n["umi_cluster_full_rounds"] >= 1
        assert n["umi_cluster_candidate_rounds"] >= (2 if name == "cut-off-bridge" else 1)
    else:
        assert n["umi_cluster_full_rounds"] == 0
    if name == "wheels":
        assert n["umi_cluster_widened"] > 0 and n["umi_cluster_narrowed"] > 0
    else:
        # one pick among 24 or more candidates, 30 among 900: never a quarter; a list of more than 256 with under a
        # 64th of it picked is the wheels' alone
        assert n["umi_cluster_widened"] == n["umi_cluster_narrowed"] == 0
    assert n["umi_cluster_rounds"] == c.facts["rounds"]


# ---------------------------------------------------------------------------
# pre-groups: clusters come back group by group (a second, stable sort over ceil_log2(ngroups + 1) bits)

def grouped(umis, groups, full=0):
    """(clusters of umi_group, clusters of umi_group_flat, counters) at threshold 1"""
    from sarlacc_amd import calls
    goff = np.zeros(len(groups) + 1, np.int64)
    np.cumsum([len(g) for g in groups], out=goff[1:])
    gflat = np.concatenate([np.asarray(g, np.int32) for g in groups])
    try:
        calls.set_option("umi_full_rounds", full)
        got = as_lists(calls.umi_group(umis, 1, None, 1, groups))
        n = counters("groups=%d full_rounds=%d" % (len(groups), full))
        coff, mem = calls.umi_group_flat(umis, 1, None, 1, goff, gflat)
        return got, [[int(v) for v in mem[a:b]] for a, b in zip(coff[:-1], coff[1:])], n
    finally:
        calls.set_option("umi_full_rounds", 0)


@pytest.mark.parametrize("ngroups", K.PREGROUP_COUNTS)
def test_pregroups_keep_their_order(oracle, ngroups):
    umis, groups = K.pregroups(ngroups)
    ref = as_lists(oracle.umi_group(umis, 1, None, 1, groups, fast=True))
    got, flat, n = grouped(umis, groups)
    same_lists(got, ref)
    same_lists(flat, ref)
    assert n["umi_links"] < 24 * len(umis) and n["umi_cluster_candidate_rounds"] == 0


@pytest.mark.parametrize("full", [0, 1])
def test_dense_pregroup_among_tiny_ones(oracle, full):
    umis, groups = K.dense_pregroup()
    ref = as_lists(oracle.umi_group(umis, 1, None, 1, groups, fast=True))
    got, flat, n = grouped(umis, groups, full)
    same_lists(got, ref)
    same_lists(flat, ref)
    assert n["umi_links"] >= 24 * len(umis)
    assert (n["umi_cluster_candidate_rounds"] == 0) == bool(full)
    assert n["umi_cluster_rounds"] == n["umi_cluster_candidate_rounds"] + n["umi_cluster_full_rounds"] >= 1


# ---------------------------------------------------------------------------
# refusals

SYMMETRIC = "neighbour lists must be symmetric and contain the read itself"


@pytest.mark.parametrize("links,message", [
    ([[1, 2], [1, 2], [4, 5], [3, 4, 5], [3, 4]], SYMMETRIC + r" \(list 3 is not\)"),             # lists 3 and 5 miss themselves
    ([[2, 3], [1, 2], [1, 3]], SYMMETRIC + r" \(list 1 is not\)"),
    ([[1], [2, 3], [3, 2, 4], [4]], SYMMETRIC + r" \(list 3 is not\)"),                            # 3 names 4, 4 does not name 3
    ([[1, 2], [2, 1, 3], [3, 2], [4, 5], [5]], SYMMETRIC + r" \(list 4 is not\)"),
    ([[1, 3], [2]], r"link 3 outside 1\.\.2"),
    ([[1, 2], [2, 0]], r"link 0 outside 1\.\.2"),
    ([[1, 2], [2, -1]], r"link -1 outside 1\.\.2"),
    ([[1, 1, 2], [1, 2]], "list 1 names a read twice"),                                           # 3 entries from 2 nodes
    ([[1, 2], [2, 1], [3, 4, 3], [4, 4, 3]], "list 3 names a read twice"),
    ([[1, 1]], "list 1 names a read twice"),
    ([[1, 2, 2], [2, 3], [3, 3, 2]], "list 1 names a read twice"),                                # list 1 is asymmetric too
    ([[1, 2], [2, 3], [3, 3, 2]], SYMMETRIC + r" \(list 1 is not\)"),                              # the lowest list decides
])
def test_lists_that_are_no_neighbour_lists_are_refused(links, message):
    from sarlacc_amd import SarlaccError, calls
    with pytest.raises(SarlaccError, match=message):
        calls.cluster_umis_test(links)


@pytest.mark.parametrize("links,message", [
    ([[], [1]], "zero length read group"),                                             # the empty list comes first
    ([[2], []], "single-read groups should contain only the read itself"),             # the bad solo comes first
    ([[1], [], [2]], "zero length read group"),
    ([[1], [3], []], "single-read groups should contain only the read itself"),
    ([[1, 1, 2], [1, 2], []], "zero length read group"),                               # the reference's errors before the library's
    ([[2, 3], [1, 2], [1, 3], [1]], "single-read groups should contain only the read itself"),
])
def test_reference_errors_come_in_index_order_and_first(oracle, links, message):
    from sarlacc_amd import SarlaccError, calls
    with pytest.raises(oracle.OracleError, match=message):
        oracle.cluster_umis_test(links)
    with pytest.raises(SarlaccError, match=message):
        calls.cluster_umis_test(links)


def test_a_refusal_leaves_the_next_call_intact(oracle):
    from sarlacc_amd import SarlaccError, calls
    with pytest.raises(SarlaccError, match="names a read twice"):
        calls.cluster_umis_test([[1, 1, 2], [1, 2]])
    same_lists(as_lists(calls.cluster_umis_test([[1, 2], [1, 2]])), [[1, 2]])
