"""Graphs for the greedy clustering of the UMI stage (umi_cluster.hip, cluster_dev in umi_host.cpp), shared by
tests/test_umi_cluster_cases.py (CPU: the builders against the oracle's two forms, a plain restatement and the closed
forms below, and each case on the path it is named for) and tests/test_gpu_umi_cluster.py (GPU: the kernels against the
oracle).

The clustering is exact integer work: the reference's sequential greedy pass, evaluated in parallel rounds that must
return its clusters in its order.  It runs in three ways -- a thread per node (fewer than 24 links per node on average),
a wavefront per node, and rounds on candidate sets under a control block on the device (24 and more) -- and random
graphs reach few of their edges: no ties on the count, no chains of dependent picks, no list whose length sits on 64 or
256, no pick whose list is mostly dead, nothing at the 24-link switch or at the capacity of the candidate list.

  paths, stars, equal_cliques, staircase, orphans, smallest      a thread per node
  clique, three_blocks, equal_large_cliques, cut_off, wheels,
  distinct_cliques                                                a wavefront per node / the candidate-set rounds
  pregroups, dense_pregroup                                       UMI strings and pre-groups, for umi_group

Every graph is a list of 1-based neighbour lists, symmetric, each holding its own node.  The order inside a list is
the order of the members of a cluster, so the builders shuffle it (seeded).  `expect` is the clustering as it follows
from the construction, where it does (None otherwise): a sequence of seeds, each taking what is left of its own list.

numpy and the standard library only; every draw is seeded."""
import functools

import numpy as np

DENSE_LINKS_PER_NODE = 24        # cluster_dev: one wavefront per node from this average on
CANDIDATE_CAPACITY = 1024        # cluster_candidates_begin: the candidate list holds max(1024, n / 8) nodes
CL_GROUP = 8                     # candidate-set rounds the host enqueues per read-back
RESTATEMENT_MAX_LINKS = 200000   # the pure-Python greedy gets slow beyond


def candidate_capacity(n):
    return max(CANDIDATE_CAPACITY, n // 8)


# ---------------------------------------------------------------------------
# the greedy rule, restated (lists and integers only)

def greedy(links, counts=None):
    """Solos first, by index.  Then, repeatedly, the node with the largest remaining count, ties to the largest index:
    its cluster is its still-unused neighbours in list order; each newly used node zeroes its own count and decrements
    every still-positive count in its list.  `counts`: a list that receives the count each seed was picked with."""
    rem = [len(l) for l in links]
    out = [[i + 1] for i in range(len(links)) if rem[i] == 1]
    pool = set(i for i in range(len(links)) if rem[i] > 1)
    while True:
        best = max((i for i in pool if rem[i] > 0), key=lambda i: (rem[i], i), default=None)
        if best is None:
            return out
        pool.discard(best)
        if counts is not None:
            counts.append(rem[best])
        out.append([])
        for v in links[best]:
            if rem[v - 1] > 0:
                out[-1].append(v)
                rem[v - 1] = 0
                for w in links[v - 1]:
                    rem[w - 1] -= rem[w - 1] > 0


class Case:
    """name; links (1-based lists); expect (clusters, or None); dense (24 links per node or more); `facts`: what the
    construction promises beyond that.  ties: nodes at the top count; pick_counts: the count each seed is picked with;
    solos, orphans: how many (the CPU test checks these against the restated rule).  rounds: parallel rounds the
    device needs by the argument in the builder's text, rounds_full: the same with `umi_full_rounds` set (the GPU
    test checks these against the counters)."""

    def __init__(self, name, links, expect=None, **facts):
        self.name, self.links, self.expect, self.facts = name, links, expect, facts
        self.n = len(links)
        self.nlinks = sum(len(l) for l in links)
        self.dense = self.nlinks >= DENSE_LINKS_PER_NODE * self.n

    def __repr__(self):
        return "Case(%s, n=%d, links=%d)" % (self.name, self.n, self.nlinks)


def _finish(nb, rng=None, label=None):
    """0-based neighbour collections -> 1-based lists, shuffled with `rng` (sorted without), nodes renamed by `label`
    (label[old] = new, 0-based) where one is given"""
    n = len(nb)
    label = np.arange(n) if label is None else np.asarray(label)
    out = [None] * n
    for v, l in enumerate(nb):
        a = np.sort(label[np.fromiter(l, dtype=np.int64, count=len(l))]) + 1
        out[int(label[v])] = (rng.permutation(a) if rng is not None else a).tolist()
    return out


def seeded(links, seeds):
    """the clusters of a known sequence of seeds (1-based): each takes what is left of its list, in list order"""
    used, out = set(), []
    for s in seeds:
        out.append([v for v in links[s - 1] if v not in used])
        used.update(out[-1])
    return out


# ---------------------------------------------------------------------------
# a thread per node

PATH_SIZES = (2, 3, 255, 256, 257, 1025)   # around the 256-thread blocks of the per-node kernels


def path(n, relabel=False):
    """A path of n nodes.  Indexed along the path the picks are strictly sequential -- node n - 1 first, then every
    third node downwards, each blocked by the one before it until that one's round is over -- and what is left at the
    low end (one node or two) comes last: a pick per round, ceil(n / 3) rounds.  With `relabel` the nodes are renamed at random."""
    rng = np.random.default_rng(1000 + 2 * n + relabel)
    nb = [[w for w in (v - 1, v, v + 1) if 0 <= w < n] for v in range(n)]
    if relabel:
        return Case("path-%d-relabelled" % n, _finish(nb, rng, rng.permutation(n)))
    links = _finish(nb, rng)
    seeds = list(range(n - 1, 1, -3)) if n > 2 else []
    left = n - 3 * len(seeds)                      # nodes 1..left are untouched by the triples above them
    seeds += [2] if left == 2 else [1] if left == 1 else []
    return Case("path-%d" % n, links, seeded(links, seeds), rounds=len(seeds))


STAR_LEAVES = (1, 63, 64, 65, 300)
STAR_HUB_AT = ("first", "last", "middle")


def star(leaves, hub_at):
    """A hub and its leaves; the hub stands first, last or in the middle of its own list (the rest of that list is
    shuffled).  One cluster: the hub's list as given.  The hub is the last node with one leaf (a pair: the tie goes to
    the larger index), the first, last or middle node otherwise."""
    rng = np.random.default_rng(2000 + 3 * leaves + STAR_HUB_AT.index(hub_at))
    n = leaves + 1
    hub = n if leaves == 1 or hub_at == "last" else 1 if hub_at == "first" else n // 2 + 1
    others = [int(v) for v in rng.permutation([v for v in range(1, n + 1) if v != hub])]
    at = {"first": 0, "last": leaves, "middle": leaves // 2}[hub_at]
    links = [[hub, v] if (v + leaves) % 2 else [v, hub] for v in range(1, n + 1)]
    links[hub - 1] = others[:at] + [hub] + others[at:]
    return Case("star-%d-hub-%s" % (leaves, hub_at), links, [list(links[hub - 1])], ties=1 if leaves > 1 else 2, rounds=1)


def equal_cliques(size, count, interleaved=True):
    """`count` disjoint cliques of `size` nodes: every node carries the same count, every pick is decided by the index
    alone.  Clusters by their largest member, descending, each that member's list.  Interleaved: node v belongs to
    clique v % count; otherwise the cliques are runs of consecutive nodes."""
    rng = np.random.default_rng(3000 + 100 * size + count)
    n = size * count
    if interleaved:
        members = [list(range(c, n, count)) for c in range(count)]
    else:
        members = [list(range(c * size, (c + 1) * size)) for c in range(count)]
    nb = [None] * n
    for m in members:
        for v in m:
            nb[v] = m
    links = _finish(nb, rng)
    seeds = sorted((max(m) + 1 for m in members), reverse=True)
    return Case("cliques-%dx%d" % (count, size), links, seeded(links, seeds), ties=n, rounds=1)


def staircase(hubs=12):
    """Hubs 1..m of growing count c_j = 3 + 3 j: hub j has its own leaves and shares two leaves with hub j + 1 and two
    with hub j - 1.  The pick of hub j + 1 takes the two shared leaves and so lowers hub j by exactly 2, to c_j - 2.
    Beside each hub j < m stands a lone star X_j of count c_j - 1, its hub at a smaller index.  In order: hub m, then
    X_j before hub j for j = m - 1 .. 1.  A missed decrement leaves hub j at c_j - 1 or above, level with X_j, and the
    larger index goes first; a doubled one drops it to c_j - 4, below hub j - 1 at c_j - 3.  One hub per round (each
    lies two hops from the next): m rounds."""
    rng = np.random.default_rng(4000 + hubs)
    m = hubs
    nb, hub, xhub = [], {}, {}

    def node():
        nb.append([len(nb)])
        return len(nb) - 1

    def join(a, b):
        nb[a].append(b)
        nb[b].append(a)

    for j in range(1, m):            # the lone stars first: smaller indices than the hubs
        xhub[j] = node()
    first_leaf = len(nb)
    for j in range(1, m):
        for _ in range(3 + 3 * j - 2):           # count c_j - 1 with the hub itself
            join(xhub[j], node())
    shared = {j: (node(), node()) for j in range(1, m)}      # between hub j and hub j + 1
    private = {j: [node() for _ in range(3 + 3 * j - 1 - 2 * (j < m) - 2 * (j > 1))] for j in range(1, m + 1)}
    last_leaf = len(nb)
    for j in range(1, m + 1):
        hub[j] = node()
        for l in private[j]:
            join(hub[j], l)
        for k in (j - 1, j):
            for l in shared.get(k, ()):
                join(hub[j], l)
    label = np.arange(len(nb))
    label[first_leaf:last_leaf] = first_leaf + rng.permutation(last_leaf - first_leaf)    # leaves in any order
    links = _finish(nb, rng, label)
    seeds = [hub[m]] + [s for j in range(m - 1, 0, -1) for s in (xhub[j], hub[j])]
    counts = [3 + 3 * m] + [c for j in range(m - 1, 0, -1) for c in (3 + 3 * j - 1, 3 + 3 * j - 2)]
    return Case("staircase-%d" % m, links, seeded(links, [int(label[s]) + 1 for s in seeds]), pick_counts=counts, rounds=m)


def orphans():
    """Two hubs (counts 9 and 7), five true solos, and four nodes whose only neighbours are a leaf of each hub: both
    leaves go with their hubs, the node's count falls from 3 to 1, and it comes last, alone, by descending index.  The
    solos come first, ascending; solo and orphan indices alternate."""
    rng = np.random.default_rng(5000)
    nb = []

    def node():
        nb.append([len(nb)])
        return len(nb) - 1

    def join(a, b):
        nb[a].append(b)
        nb[b].append(a)

    solo, orphan = [], []
    for k in range(9):
        (solo if k % 2 == 0 else orphan).append(node())
    A, B = node(), node()
    la = [node() for _ in range(8)]
    lb = [node() for _ in range(6)]
    for l in la:
        join(A, l)
    for l in lb:
        join(B, l)
    for k, o in enumerate(orphan):
        join(o, la[k])
        join(o, lb[k])
    links = _finish(nb, rng)
    expect = [[s + 1] for s in solo] + seeded(links, [A + 1, B + 1] + [o + 1 for o in reversed(orphan)])
    return Case("orphans", links, expect, solos=len(solo), orphans=len(orphan), pick_counts=[9, 7, 1, 1, 1, 1], rounds=2)


def smallest():
    """one solo; a pair (the tie goes to node 2, whose list gives the order); 300 solos (two blocks, no round at all)"""
    return [Case("one-solo", [[1]], [[1]], rounds=0),
            Case("pair", [[1, 2], [1, 2]], [[1, 2]], ties=2, rounds=1),
            Case("pair-reversed", [[2, 1], [2, 1]], [[2, 1]], ties=2, rounds=1),
            Case("solos-300", [[v] for v in range(1, 301)], [[v] for v in range(1, 301)], rounds=0)]


# ---------------------------------------------------------------------------
# a wavefront per node, and the candidate-set rounds

THRESHOLD_CLIQUES = (23, 24, 25)         # 23 links per node: a thread per node; 24: the first size on the wavefront rounds
CHUNK_CLIQUES = (64, 65, 128, 129)       # lists that end on and one past the 64 lanes of a wavefront


def clique(n):
    """one clique, lists shuffled: one cluster, the list of node n"""
    rng = np.random.default_rng(6000 + n)
    links = _finish([range(n)] * n, rng)
    return Case("clique-%d" % n, links, [list(links[n - 1])], ties=n, rounds=1, rounds_full=1)


def three_blocks():
    """Three cliques of 100 on the nodes 1..100, 61..160 and 121..220.  The 80 nodes of two cliques carry 160; node 160
    is the largest of them and takes 61..220 in its list order.  1..60 then carry 60 each; node 60 takes them in its
    list order, past the 40 dead entries that lie scattered over both 64-entry chunks of its list: the members of a
    cluster are compacted with a ballot and a running offset."""
    rng = np.random.default_rng(6500)
    nb = [set() for _ in range(220)]
    for lo in (0, 60, 120):
        for v in range(lo, lo + 100):
            nb[v].update(range(lo, lo + 100))
    links = _finish(nb, rng)
    return Case("three-blocks", links, seeded(links, [160, 60]), ties=80, pick_counts=[160, 60], rounds=2, rounds_full=2)


def equal_large_cliques():
    """30 disjoint cliques of 30, consecutive nodes: 900 candidates tie, under the list's capacity of 1 024; clusters by
    their largest member 900, 870, ..."""
    c = equal_cliques(30, 30, interleaved=False)
    c.name = "large-" + c.name
    c.facts.update(rounds=1, rounds_full=1)
    return c


def cut_off(bridge=False):
    """One clique of 1 025 and cliques of 40 and 30.  1 025 nodes carry the top count, more than the candidate list
    holds: the first candidate round is cut off and a round over every list runs in its place.  That round picks every
    2-hop maximum, so with disjoint cliques it finishes all three.  With `bridge`, one link joins a node of the 40 to a
    node of the 30: the first (count 41) takes its clique and the second, and the other 29, two hops away and blocked
    during the full round, are left for a candidate round after it."""
    rng = np.random.default_rng(7000 + bridge)
    n = 1025 + 40 + 30
    blocks = [range(0, 1025), range(1025, 1065), range(1065, n)]
    nb = [set() for _ in range(n)]
    for b in blocks:
        for v in b:
            nb[v].update(b)
    label = rng.permutation(n)
    top = [max(int(label[v]) for v in b) + 1 for b in blocks]
    if bridge:
        nb[1025].add(1065)
        nb[1065].add(1025)
        top = [top[0], int(label[1025]) + 1, max(int(label[v]) for v in blocks[2] if v != 1065) + 1]
    links = _finish(nb, rng, label)
    return Case("cut-off" + ("-bridge" if bridge else ""), links, seeded(links, top), ties=1025,
                pick_counts=[1025, 41, 29] if bridge else [1025, 40, 30], rounds=3 if bridge else 2, rounds_full=2 if bridge else 1)


def wheels(tail=40):
    """Eight components, each a hub joined to two disjoint cliques of 200 (the hub's list holds 401, a member's 201), a
    clique of 300 and one of `tail`, nodes renamed at random.  Candidate round one: the 8 hubs, all picked -- the window
    widens.  Round two: the 300 tied nodes, one pick -- it narrows.  The control block looks at a round's yield only when
    another round follows, which is what the last clique is for.  Eight clusters of 401 by descending hub, the clique of
    300, then the tail."""
    rng = np.random.default_rng(8000 + tail)
    n = 8 * 401 + 300 + tail
    nb = [set() for _ in range(n)]
    hubs = []
    for c in range(8):
        base = 401 * c
        hubs.append(base)
        nb[base].update(range(base, base + 401))
        for lo in (base + 1, base + 201):
            for v in range(lo, lo + 200):
                nb[v].update(range(lo, lo + 200))
                nb[v].add(base)
    for lo, size in ((8 * 401, 300), (8 * 401 + 300, tail)):
        for v in range(lo, lo + size):
            nb[v].update(range(lo, lo + size))
    label = rng.permutation(n)
    links = _finish(nb, rng, label)
    seeds = sorted((int(label[h]) + 1 for h in hubs), reverse=True)
    seeds += [max(int(label[v]) for v in range(lo, lo + size)) + 1 for lo, size in ((8 * 401, 300), (8 * 401 + 300, tail))]
    return Case("wheels", links, seeded(links, seeds), ties=8, pick_counts=[401] * 8 + [300, tail], rounds=3, rounds_full=1)


BOUNDARY_CLIQUES = (7, 8, 9, 15, 16, 17)


def distinct_cliques(count):
    """`count` disjoint cliques of 24, 25, ... nodes, interleaved.  The candidate window (count >= the largest count,
    never widened: one pick among 24 or more candidates) holds one clique per round, so the candidate rounds number
    `count`: with 8 and 16 the last working round is the last of a group of CL_GROUP = 8 and the group after it finds
    nothing left in its first round; 7 and 15 end one round before the group does, 9 and 17 one round into the next.
    Clusters by size, descending.  Measured on an MI355X: umi_cluster_rounds = 7, 8, 9, 15, 16, 17 for those counts (all
    candidate rounds), so 8 and 16 cliques sit on the boundary as built, no clique more or fewer; 1 round with
    `umi_full_rounds`, which picks every clique's largest node at once."""
    rng = np.random.default_rng(9000 + count)
    sizes = list(range(24, 24 + count))
    n = sum(sizes)
    order = rng.permutation(n)
    members, at = [], 0
    for s in sizes:
        members.append([int(v) for v in order[at:at + s]])
        at += s
    nb = [None] * n
    for m in members:
        for v in m:
            nb[v] = m
    links = _finish(nb, rng)
    seeds = [max(m) + 1 for m in reversed(members)]
    return Case("distinct-cliques-%d" % count, links, seeded(links, seeds), ties=sizes[-1], pick_counts=sizes[::-1], rounds=count, rounds_full=1)


SPARSE = dict([("path-%d%s" % (n, "-relabelled" if r else ""), (path, n, r)) for n in PATH_SIZES for r in (False, True)]
              + [("star-%d-hub-%s" % (l, at), (star, l, at)) for l in STAR_LEAVES for at in STAR_HUB_AT]
              + [("cliques-65x%d" % s, (equal_cliques, s, 65)) for s in (2, 3, 4, 5, 6)]
              + [("staircase-12", (staircase,)), ("orphans", (orphans,)), ("clique-23", (clique, 23))])
SMALLEST = ("one-solo", "pair", "pair-reversed", "solos-300")
DENSE = dict([("clique-%d" % n, (clique, n)) for n in THRESHOLD_CLIQUES[1:] + CHUNK_CLIQUES]
             + [("three-blocks", (three_blocks,)), ("large-cliques-30x30", (equal_large_cliques,)), ("cut-off", (cut_off,)),
                ("cut-off-bridge", (cut_off, True)), ("wheels", (wheels,))]
             + [("distinct-cliques-%d" % k, (distinct_cliques, k)) for k in BOUNDARY_CLIQUES])
SPARSE_NAMES = tuple(SPARSE) + SMALLEST
DENSE_NAMES = tuple(DENSE)


@functools.lru_cache(maxsize=None)
def case(name):
    """the case of that name, built once per process (nobody changes its lists)"""
    if name in SMALLEST:
        return {c.name: c for c in smallest()}[name]
    f = (SPARSE.get(name) or DENSE[name])
    c = f[0](*f[1:])
    assert c.name == name, (c.name, name)
    return c


# ---------------------------------------------------------------------------
# pre-groups, for umi_group

PREGROUP_COUNTS = (1, 2, 3, 255, 256, 257, 1000)   # the group sort runs over ceil_log2(ngroups + 1) bits: 1 2 2 8 9 9 10
BASES = "ACGT"


def _variant(rng, u):
    p = int(rng.integers(0, len(u)))
    return u[:p] + str(rng.choice([b for b in BASES if b != u[p]])) + u[p + 1:]


def pregroups(ngroups):
    """(umis, groups): `ngroups` pre-groups of 1 to 6 reads, every third one a single read, the members drawn from a
    random permutation of the read indices (1-based; no group is contiguous or sorted).  A group's 8-base UMIs are a
    random root, copies of it and strings one substitution from it: at threshold 1 two such variants may or may not be
    neighbours, so a group splits into one to a few clusters."""
    rng = np.random.default_rng(11000 + ngroups)
    sizes = rng.integers(2, 7, ngroups)
    sizes[::3] = 1
    if ngroups < 3:
        sizes = np.array([6, 1][:ngroups])
    total = int(sizes.sum())
    reads = rng.permutation(total) + 1
    umis, groups, at = [None] * total, [], 0
    for s in sizes:
        g = [int(r) for r in reads[at:at + int(s)]]
        at += int(s)
        root = "".join(rng.choice(list(BASES), 8))
        for r in g:
            umis[r - 1] = root if rng.random() < 0.3 else _variant(rng, root)
        groups.append(g)
    return umis, groups


def dense_pregroup():
    """(umis, groups): one pre-group of 200 + 150 copies of two UMIs one substitution apart -- a clique of 350 at
    threshold 1 -- in the middle of 300 pre-groups of 1 to 3 reads: 24 links per node and more over the whole call, which
    therefore takes the wavefront rounds while most of its components hold two or three nodes."""
    rng = np.random.default_rng(12000)
    sizes = [int(s) for s in rng.integers(1, 4, 300)]
    sizes.insert(150, 350)
    total = sum(sizes)
    reads = rng.permutation(total) + 1
    umis, groups, at = [None] * total, [], 0
    for s in sizes:
        g = [int(r) for r in reads[at:at + s]]
        at += s
        root = "".join(rng.choice(list(BASES), 8))
        other = _variant(rng, root)
        for k, r in enumerate(g):
            if s == 350:
                umis[r - 1] = root if k % 7 < 4 else other
            else:
                umis[r - 1] = root if rng.random() < 0.3 else _variant(rng, root)
        groups.append(g)
    return umis, groups
