"""The generators of tests/umi_cases.py against the dense distances, without a GPU: a case that holds no pair at the
threshold, or a set on which the tile filter keeps everything, would let a wrong cut or a wrong filter pass."""
import functools

import numpy as np
import pytest

from tests import umi_cases as K

PART1 = ([(n, t) for n in K.ONE_WORD_LENGTHS for t in K.ONE_WORD_LIMITS]
         + [(n, t) for n in K.FOUR_WORD_LENGTHS for t in K.FOUR_WORD_LIMITS]
         + [(n, t) for n in K.XL_LENGTHS for t in K.XL_LIMITS])


@pytest.mark.parametrize("length,limit", PART1)
def test_at_limit_families_hold_pairs_at_and_just_past_the_limit(oracle, length, limit):
    alphabet = K.case_alphabet(length)
    seqs = K.at_limit_families(np.random.default_rng(K.case_seed(length, limit)), length, limit, alphabet, K.case_molecules(length))
    assert len(seqs) <= 120 and len(set(seqs)) < len(seqs)
    assert max(len(s) for s in seqs) <= K.path_max_length(length) and max(len(s) for s in seqs) >= length
    assert min(len(s) for s in seqs) <= 7
    d2 = K.dense_d2(seqs, oracle)
    census = K.limit_census(d2, limit)
    # two strings are never further apart than the longer one is long, and relatives grow up to the path's longest string:
    # only a threshold beyond that length (33 and 40 on the one-word path) can hold no pair at exactly the limit.  From the
    # molecules' own length on, a pair just past the limit is not required.
    if limit <= K.path_max_length(length):
        assert census["at"] >= 1, census
    if limit < length:
        assert census["past"] >= 1, census
    if limit > K.path_max_length(length):
        assert int(d2.max()) <= 2 * limit   # every pair of a pre-group is a neighbour
    if "N" in alphabet:
        assert census["odd"] >= 1, census
        assert any("N" in s for s in seqs) and any("N" not in s for s in seqs)
    else:
        assert not any("N" in s for s in seqs)


def test_dense_neighbours_are_the_trie_walk(oracle):
    # the two references agree on a case of their own, so a difference on the GPU is the GPU's
    rng = np.random.default_rng(3)
    for length, limit in ((12, 2), (40, 6)):
        seqs = K.at_limit_families(rng, length, limit, "ACGTN")
        got = K.neighbours_from_d2(seqs, K.dense_d2(seqs, oracle), limit)
        for g, w in zip(got, oracle.fast_levdist_test(seqs, limit)):
            assert g.tolist() == w.tolist()


def test_bands():
    assert [K.one_word_band(t) for t in K.ONE_WORD_LIMITS] == [0, 1, 2, 3, 4, 5, 8, 8, 8, 16, 16, 16, 32, 32, 32, 32, 32]
    assert [K.long_band(t) for t in K.FOUR_WORD_LIMITS] == [5, 8, 8, 8, 16, 16, 16, -1, -1, -1]
    assert [K.long_band(t) for t in K.XL_LIMITS] == [5, 8, 8, 16, -1]


@functools.lru_cache(maxsize=None)
def anchored(L):
    return tuple(K.anchored_set(np.random.default_rng(40 + L), L))


@pytest.mark.parametrize("L", [1, 2, 3, 4, 5])
def test_anchored_set_engages_the_tile_filter(L):
    seqs = anchored(L)
    assert len(seqs) == 6400 and max(len(s) for s in seqs) <= 32 and not any("N" in s for s in seqs)
    kept, total = K.tile_pairs_kept(seqs, L)
    print("L=%d: %d of %d tile pairs kept" % (L, kept, total))
    assert total == 325 and 0 < kept < total
    # neighbours at exactly L edits (and pairs at L + 1) that the tiles separate
    tile_of = {seqs[j]: r // K.TILE for r, j in enumerate(K.trie_order(seqs))}
    from tests.test_oracle_umi import lev2
    by_tail = {}
    for s in seqs:
        by_tail.setdefault(s[-10:], []).append(s)
    at = 0
    for group in list(by_tail.values())[:100]:
        for a in group:
            for b in group:
                if a < b and tile_of[a] != tile_of[b]:
                    at += lev2(a, b) == 2 * L
    assert at >= 1


@pytest.mark.parametrize("L", [1, 2, 3, 4, 5])
def test_tile_rule_keeps_every_neighbour_and_a_stricter_one_does_not(oracle, L):
    # the restated rule drops no tile pair that holds a neighbour; granted one edit less it drops some that do, so a
    # filter that is wrong by as little as that loses links of this set
    seqs = list(anchored(L))
    need = K.tile_pairs_with_neighbours(seqs, oracle.fast_levdist_test(seqs, L))
    kept, total = K.tile_pairs_kept_set(seqs, L)
    assert need <= kept and len(need - {(t, t) for t in range(25)}) > 0
    strict, _ = K.tile_pairs_kept_set(seqs, L, allowed=L - 1)
    assert need - strict


def test_overflow_sets():
    clump = K.overflow_clump(np.random.default_rng(9))
    assert len(clump) == 1840 and -(-len(clump) // K.TILE) < 16
    assert clump.count("ACGTTGCAAC") * (clump.count("ACGTTGCAAC") - 1) // 2 > K.PAIR_BUFFER
    sampled = K.overflow_sampled(np.random.default_rng(10))
    nt = -(-len(sampled) // K.TILE)
    assert len(sampled) == 21600 and nt == 85
    assert 1600 * 1599 // 2 > max(K.PAIR_BUFFER, 32 * len(sampled))
    assert K.undirected_pairs([np.array([1, 2]), np.array([1, 2, 3]), np.array([2])]) == 2
