"""Inputs for the neighbour search of the UMI stage, shared by tests/test_umi_cases.py (CPU: the generators against the
dense distances, so the pairs are where they claim to be) and tests/test_gpu_umi_thresholds.py (GPU: the search against
two CPU references).

The search is exact integer work behind a chain of filters (length, composition, shifted Hamming, the common prefixes of
256-string tiles and 64-string blocks), in kernels instantiated per threshold class.  A wrong cut or a filter that drops
a true neighbour shows only on a pair at the threshold, and only where the filter in question discards something:

  at_limit_families   families whose members lie exactly `limit` and `limit + 1` edits apart, the edits at the front, at
                      the back or spread out, with masked bases for the half-unit costs
  anchored_set        6 400 strings behind four shared 14-base flanks: tiles with long common prefixes, and true
                      neighbours in different tiles whose edits all sit inside those prefixes
  tile_pairs_kept     the rule of k_tile_info / k_tile_pairs restated in Python, to show that anchored_set makes the tile
                      filter discard something and keep something
  overflow_*          sets whose pair count exceeds the first pair buffer

numpy and the standard library only; every draw is seeded."""
import numpy as np

BASES = "ACGT"
RANK = {c: i for i, c in enumerate("ACGTN")}   # the trie's child order
TILE = 256
PAIR_BUFFER = 1 << 20                          # pairs the first search attempt has room for (at least)

# thresholds per path, and the template instantiation each one reaches (K of k_umi_pairs<K> / k_umi_pairs_long<K, XL>)
ONE_WORD_LENGTHS = (8, 12, 31, 32)
ONE_WORD_LIMITS = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 31, 32, 33, 40)
FOUR_WORD_LENGTHS = (33, 64, 65, 128)
FOUR_WORD_LIMITS = (4, 6, 7, 8, 10, 15, 16, 17, 19, 40)
XL_LENGTHS = (129, 300)
XL_LIMITS = (4, 7, 8, 16, 17)


def one_word_band(limit):
    """K of the k_umi_pairs<K> a threshold runs in"""
    for k in (0, 1, 2, 3, 4, 5, 8, 16):
        if limit <= k:
            return k
    return 32


def long_band(limit):
    """K of the k_umi_pairs_long<K, XL> a threshold runs in; -1: the full DP"""
    for k in (0, 1, 2, 3, 5, 8, 16):
        if limit <= k:
            return k
    return -1


def path_max_length(length):
    """the longest string that stays on the path of a `length`-base string"""
    return 32 if length <= 32 else 128 if length <= 128 else 1024


def case_seed(length, limit):
    return 7000 + 100 * length + limit


def case_alphabet(length):
    """two lengths stay free of N, so that whole calls without a masked base are searched too"""
    return "ACGT" if length in (12, 65) else "ACGTN"


def case_molecules(length):
    """fewer families at 31 and 32 bases: the dense reference there is pure Python at 1 000 cells per pair"""
    return 8 if length in (31, 32) else 11


# ---------------------------------------------------------------------------
# part 1: pairs exactly at and just past the limit

def _other_base(rng, c):
    return str(rng.choice([b for b in BASES if b != c]))


def _zone(zone, n):
    """positions [lo, hi) of an n-base string the edits of a zone fall in"""
    if zone == 0:
        return 0, min(4, n)
    if zone == 1:
        return max(0, n - 4), n
    return 0, n


def _edited(rng, ref, edits, kind, zone, max_length, target=None):
    """`ref` with `edits` edits of one kind (0 substitutions, 1 deletions, 2 insertions, 3 a random mix), all inside the
    zone (0: the first 4 bases, 1: the last 4, 2: anywhere).  No base is edited twice: a substitution that finds every base of
    its zone used moves on to the nearest unused one, and once the string is at the path's longest an insertion turns into a
    substitution.  Deletions and insertions alone therefore give a string at exactly `edits` edits from `ref`.  With a
    `target` every substitution puts that base in place of another one: each of them moves the composition by 2, none
    undoes another, and the composition bound of the search is met with equality."""
    s = [[c, False] for c in ref]   # base, already edited
    for _ in range(edits):
        k = kind if kind != 3 else int(rng.integers(0, 3))
        if k == 2 and len(s) >= max_length:
            k = 0
        if k != 2 and not s:
            break
        lo, hi = _zone(zone, len(s))
        if k == 0:
            free = [p for p in range(lo, hi) if not s[p][1] and s[p][0] != target]
            if not free:
                rest = [p for p in range(len(s)) if not s[p][1] and s[p][0] != target]
                if not rest:
                    continue
                end = hi - 1 if zone == 1 else lo
                free = [min(rest, key=lambda p: abs(p - end))]
            p = free[int(rng.integers(0, len(free)))]
            s[p] = [target or _other_base(rng, s[p][0]), True]
        elif k == 1:
            del s[int(rng.integers(lo, hi))]
        else:
            s.insert(int(rng.integers(lo, hi + 1)), [BASES[int(rng.integers(0, 4))], True])
    return "".join(c for c, _ in s)


def _masked(rng, s, count, zone):
    """`s` with `count` of its bases (inside the zone, where it has that many) replaced by N"""
    t = list(s)
    lo, hi = _zone(zone, len(t))
    if hi - lo < count:
        lo, hi = 0, len(t)
    for p in rng.permutation(np.arange(lo, hi))[:count]:
        t[int(p)] = "N"
    return "".join(t)


def at_limit_families(rng, length, limit, alphabet="ACGT", molecules=11):
    """`molecules` random strings of `length` bases with 8 relatives each, five duplicates and ten strings of 1 to 7
    bases, shuffled (114 strings for 11 molecules; up to three more for a threshold beyond the molecules' length, so that
    such a case holds a pair at exactly `limit` edits as long as the path's longest string allows one).

    Relative k of a molecule gets `limit` (k even) or `limit + 1` (k odd) edits; by k % 3 they all fall in the first 4
    bases, all in the last 4, or anywhere.  The kind of edit goes round with k and the molecule: substitutions (all to one
    base, so that the compositions of the pair differ by exactly twice their number and the composition bound holds with
    equality), deletions (`limit + 1` of them leave the empty string where the molecule has no more bases), insertions (up
    to the longest string of the path) or a mix.  Deletions and insertions alone put the relative at exactly that many
    edits from its molecule, whatever the threshold: a string is never nearer to a shorter one than the difference in length.

    With N in the alphabet, every second family carries masked bases: its relatives get one edit less and 1 to 3 N instead
    (an N against anything costs half an edit), so that molecule and relative lie at d2 = 2 * limit - 1 .. 2 * limit + 3, odd
    values included, and half of the short strings hold one N.  That is about 3 % N among the bases of a 32-base case.  The
    other families stay free of N: their pairs at exactly `limit` and `limit + 1` edits do not depend on where an N lands."""
    max_length = path_max_length(length)
    with_n = "N" in alphabet
    out = []
    for m in range(molecules):
        ref = "".join(rng.choice(list(BASES), length))
        masked_family = with_n and m % 2 == 1
        out.append(ref)
        for k in range(8):
            edits = limit + (k & 1)
            kind, zone = (k + m) % 4, k % 3
            target = BASES[int(rng.integers(0, 4))] if kind == 0 else None   # substitutions alone: all to one base
            if masked_family:
                rel = _edited(rng, ref, max(edits - 1, 0), kind, zone, max_length, target)
                rel = _masked(rng, rel, 1 + (k // 2) % 3, zone)
            else:
                rel = _edited(rng, ref, edits, kind, zone, max_length, target)
            out.append(rel)
    if length < limit <= max_length:
        # beyond the molecules' length a deletion relative ends at the empty string and an insertion relative at the path's
        # longest string, short of `limit` edits: one more molecule grown by insertions alone, and what `limit` and
        # `limit + 1` deletions leave of it -- at exactly that many edits, by the difference in length
        grown = _edited(rng, out[0], min(max_length, length + limit) - length, 2, 2, max_length)
        out.append(grown)
        for edits in (limit, limit + 1):
            if edits <= len(grown):
                out.append(_edited(rng, grown, edits, 1, 2, max_length))
    out += [out[int(i)] for i in rng.integers(0, len(out), 5)]
    for k in range(10):
        s = "".join(rng.choice(list(BASES), int(rng.integers(1, 8))))
        out.append(_masked(rng, s, 1, 2) if with_n and k % 2 else s)
    return [out[int(i)] for i in rng.permutation(len(out))]


def three_groups(rng, n):
    """three pre-groups over the ids 1..n, every string in one of them"""
    pre = rng.integers(0, 3, n)
    return [g for g in ((np.flatnonzero(pre == x) + 1).tolist() for x in range(3)) if g]


def neighbours_from_d2(seqs, d2, limit):
    """neighbour lists (1-based, trie order: A < C < G < T < N, a prefix first, ties by index) from a dense matrix of
    doubled distances -- the content comes from the matrix alone"""
    order = trie_order(seqs)
    within = np.asarray(d2) <= 2 * limit
    return [np.array([j + 1 for j in order if within[i, j]], dtype=np.int32) for i in range(len(seqs))]


def square_from_condensed(values, n, diagonal):
    """the symmetric matrix of the pairs (i, j), i < j, listed row by row"""
    d = np.zeros((n, n), dtype=np.int64)
    iu = np.triu_indices(n, 1)
    d[iu] = values
    d = d + d.T
    d[np.arange(n), np.arange(n)] = diagonal
    return d


def dense_d2(seqs, oracle):
    """doubled masked distances of all pairs from full tables, no trie, band or filter: the pure-Python lev2 up to 32
    bases, the oracle's dense distances beyond"""
    n = len(seqs)
    if max(len(s) for s in seqs) <= 32:
        from tests.test_oracle_umi import lev2
        d = square_from_condensed([lev2(seqs[i], seqs[j]) for i in range(n) for j in range(i + 1, n)], n, 0)
        d[np.arange(n), np.arange(n)] = [lev2(s, s) for s in seqs]
        return d
    halves = oracle.compute_lev_masked(seqs)
    return square_from_condensed(np.rint(2 * halves).astype(np.int64), n, [s.count("N") for s in seqs])


def limit_census(d2, limit):
    """pairs i < j at exactly the limit, just past it (2 * limit + 1 or + 2), and at any odd d2"""
    v = np.asarray(d2)[np.triu_indices(len(d2), 1)]
    return {"at": int(np.sum(v == 2 * limit)), "past": int(np.sum((v == 2 * limit + 1) | (v == 2 * limit + 2))),
            "odd": int(np.sum(v % 2 == 1))}


# ---------------------------------------------------------------------------
# part 2: the prefix filters, engaged

def _lev(a, b):
    prev = list(range(len(a) + 1))
    for ch in b:
        cur = [prev[0] + 1]
        for i, c in enumerate(a):
            cur.append(min(prev[i + 1] + 1, cur[i] + 1, prev[i] + (c != ch)))
        prev = cur
    return prev[-1]


def anchored_set(rng, L):
    """6 400 strings of up to 32 bases: four anchors A of 14 random bases, each with a relative B at exactly `L` edits
    (substitutions, deletions, insertions) inside its first 7 bases; 800 random 10-base tails, each once behind every A and
    once behind every B, there unchanged or with one substitution.  In trie order the 1 600 strings of an anchor and the
    1 600 of its relative fill tiles with common prefixes of 12 to 16 bases, and an A-string and the B-string of the same
    tail are neighbours at exactly L (or not, at L + 1) whose edits all lie in the prefix the tile filter looks at."""
    tails = ["".join(rng.choice(list(BASES), 10)) for _ in range(800)]
    out = []
    for _ in range(4):
        a = "".join(rng.choice(list(BASES), 14))
        while True:
            b = _edited(rng, a[:7], L, 3, 2, 32) + a[7:]
            if _lev(a, b) == L:
                break
        for t in tails:
            out.append(a + t)
            if rng.random() < 0.5:
                p = int(rng.integers(0, 10))
                t = t[:p] + _other_base(rng, t[p]) + t[p + 1:]
            out.append(b + t)
    out = [s[:32] for s in out]
    return [out[int(i)] for i in rng.permutation(len(out))]


def with_some_n(rng, seqs, fraction=0.01):
    """a copy where `fraction` of the strings have one base replaced by N"""
    out = list(seqs)
    for i in rng.permutation(len(out))[:max(1, int(round(fraction * len(out))))]:
        out[int(i)] = _masked(rng, out[int(i)], 1, 2)
    return out


def _tile_info(strings):
    """k_tile_info: (common prefix of the first and the last string, its length); a tile with an N carries none"""
    if any("N" in s for s in strings):
        return None
    a, b = strings[0], strings[-1]
    cp = 0
    while cp < min(len(a), len(b)) and a[cp] == b[cp]:
        cp += 1
    return a[:cp]


def _prefix_dist(x, y, L):
    """prefix_dist<L>: the least edit distance between x and y[:m'], |m' - len(x)| <= L; y holds at least len(x) + L
    bases.  A plain full table, no band."""
    prev = list(range(len(y) + 1))
    for c in x:
        cur = [prev[0] + 1]
        for j, ch in enumerate(y):
            cur.append(min(prev[j + 1] + 1, cur[j] + 1, prev[j] + (c != ch)))
        prev = cur
    m = len(x)
    return min(prev[max(0, m - L):m + L + 1])


def trie_order(seqs):
    """indices in the order of the trie walk: A < C < G < T < N, a prefix first, ties by index"""
    return sorted(range(len(seqs)), key=lambda j: ([RANK[c] for c in seqs[j]], j))


def tile_pairs_kept_set(seqs, L, tile=TILE, allowed=None):
    """(set of kept (row tile, column tile), total) over the upper triangle, diagonal included, under the rule of
    k_tile_pairs<L> for one pre-group: a pair of different tiles is dropped when the first min(|R|, |C| - L) bases of one
    tile's common prefix R, more than L of them, align with no prefix of the other's C within L edits, in either
    orientation.  `allowed`: the edits the comparison grants, where a test wants a rule that is too strict."""
    allowed = L if allowed is None else allowed
    order = trie_order(seqs)
    ranked = [seqs[j] for j in order]
    info = [_tile_info(ranked[t:t + tile]) for t in range(0, len(ranked), tile)]
    kept, total = set(), 0
    for i in range(len(info)):
        for j in range(i, len(info)):
            total += 1
            keep = True
            R, C = info[i], info[j]
            if j != i and R is not None and C is not None:
                m1, m2 = min(len(R), len(C) - L), min(len(C), len(R) - L)
                if m1 > L and _prefix_dist(R[:m1], C, L) > allowed:
                    keep = False
                if keep and m2 > L and _prefix_dist(C[:m2], R, L) > allowed:
                    keep = False
            if keep:
                kept.add((i, j))
    return kept, total


def tile_pairs_kept(seqs, L, tile=TILE):
    """(kept, total) tile pairs under the rule of k_tile_pairs<L>"""
    kept, total = tile_pairs_kept_set(seqs, L, tile)
    return len(kept), total


def tile_pairs_with_neighbours(seqs, lists, tile=TILE):
    """the (row tile, column tile) pairs that hold at least one pair of neighbours of the 1-based lists"""
    rank = np.empty(len(seqs), dtype=np.int64)
    rank[trie_order(seqs)] = np.arange(len(seqs))
    out = set()
    for i, nb in enumerate(lists):
        ti = int(rank[i]) // tile
        for tj in np.unique(rank[np.asarray(nb, dtype=np.int64) - 1] // tile):
            out.add((min(ti, int(tj)), max(ti, int(tj))))
    return out


# ---------------------------------------------------------------------------
# part 3: more pairs than the first pair buffer holds

def overflow_clump(rng):
    """1 500 copies of one 10-base UMI (1 124 250 pairs, past the 2^20 of the first buffer), 40 copies of a neighbour at
    distance 1 and 300 random UMIs: 8 tiles, too few for the tile list, so nothing is sampled"""
    umis = ["ACGTTGCAAC"] * 1500 + ["ACGTTGCAAG"] * 40 + ["".join(rng.choice(list(BASES), 10)) for _ in range(300)]
    return [umis[int(i)] for i in rng.permutation(len(umis))]


def overflow_sampled(rng):
    """20 000 random 12-base UMIs and 1 600 copies of one more (1 279 200 pairs): 85 tiles, a list of more than 2 048 tile
    pairs, so every 32nd of them is searched first to size the buffer"""
    umis = ["".join(r) for r in rng.choice(list(BASES), (20000, 12))] + ["GATTACAGATTC"] * 1600
    return [umis[int(i)] for i in rng.permutation(len(umis))]


def undirected_pairs(lists):
    """pairs i < j in 1-based neighbour lists (a string in its own list is no pair)"""
    links = sum(len(x) for x in lists)
    own = sum(int(np.any(np.asarray(x) == i + 1)) for i, x in enumerate(lists))
    return (links - own) // 2
