"""Plain-Python / numpy restatement of generics.referenceGroups (sarlacc_amd/refmap.py, csrc/ref_map.hip; the rules are
DESIGN §4.20, numbered here as there) and the cases its tests share.  It builds on tests/sketch_cases.py (rules 1 to 4
of §4.19: the sketches) and tests/links_verify_cases.py (rule 6a: the banded distance and its decision); everything is
integers and nothing here touches the library.  tests/test_reference_groups_host.py pins the restatement on literals
worked out by hand; tests/test_gpu_reference_groups.py holds the device to it."""
import numpy as np

from sarlacc_amd import mock
from tests import links_verify_cases as V
from tests import sketch_cases as S
from tests.read_groups_cases import split_labels

EMPTY = S.EMPTY
KEYS = ("reference", "strand", "dist", "shared", "n.candidates", "n.kmers", "ref.n.kmers", "group", "groups", "n.hits")


# ---- rule M2 -------------------------------------------------------------------------------------------------------------
def hits_of(ref_sketch, read_sketch):
    """({(r, f): shared(r, f)} of the pairs with a hit, n.hits): bucket by bucket, equal and not empty."""
    ref_sketch, read_sketch = np.asarray(ref_sketch, np.uint64), np.asarray(read_sketch, np.uint64)
    shared = {}
    for r, row in enumerate(read_sketch):
        for f, frow in enumerate(ref_sketch):
            c = sum(1 for a, b in zip(row.tolist(), frow.tolist()) if a == b != EMPTY)
            if c:
                shared[(r, f)] = c
    return shared, sum(shared.values())


# ---- rule M3 -------------------------------------------------------------------------------------------------------------
def candidates_of(shared, n_reads, min_shared, max_candidates):
    """(int32[n_reads, max_candidates] references, the same of `shared`, int32[n_reads] kept): unused slots -1 / 0."""
    cand_ref = np.full((n_reads, max_candidates), -1, np.int32)
    cand_shared = np.zeros((n_reads, max_candidates), np.int32)
    ncand = np.zeros(n_reads, np.int32)
    for r in range(n_reads):
        ranked = sorted((-c, f) for (rr, f), c in shared.items() if rr == r and c >= min_shared)[:max_candidates]
        for s, (c, f) in enumerate(ranked):
            cand_ref[r, s], cand_shared[r, s] = f, -c
        ncand[r] = len(ranked)
    return cand_ref, cand_shared, ncand


# ---- rule M4 -------------------------------------------------------------------------------------------------------------
def check_slots(refs, reads, cand_ref, ppm, w, both_strands=True):
    """Rule 6a.1 to 6a.4 on every used slot, x = the reference and y = the read: (int32 dist, -1 where the slot is
    unused or fails; uint8 strand; candidates checked), shaped as cand_ref."""
    cand_ref = np.asarray(cand_ref, np.int32)
    used = np.argwhere(cand_ref >= 0)
    dist, strand = np.full(cand_ref.shape, -1, np.int32), np.zeros(cand_ref.shape, np.uint8)
    if len(used):
        d, s = V.verify_pairs([refs[cand_ref[r, c]] for r, c in used], [reads[r] for r, _ in used], ppm, w, both_strands)
        dist[used[:, 0], used[:, 1]], strand[used[:, 0], used[:, 1]] = d, s
    return dist, strand, len(used)


# ---- rule M5 -------------------------------------------------------------------------------------------------------------
def choose(cand_ref, cand_shared, cand_dist=None, cand_strand=None):
    """(int32 reference, uint8 strand, int32 dist, int32 shared) per read.  With distances: the passing slot of smallest
    distance, the lowest among equals.  Without (identity=None): slot 0 where it is used, dist -1, strand 0."""
    n = len(cand_ref)
    reference, strand = np.full(n, -1, np.int32), np.zeros(n, np.uint8)
    dist, shared = np.full(n, -1, np.int32), np.zeros(n, np.int32)
    for r in range(n):
        if cand_dist is None:
            best = 0 if cand_ref[r][0] >= 0 else None
        else:
            passing = [(int(cand_dist[r][s]), s) for s in range(len(cand_ref[r])) if cand_ref[r][s] >= 0 and cand_dist[r][s] >= 0]
            best = min(passing)[1] if passing else None
        if best is not None:
            reference[r], shared[r] = cand_ref[r][best], cand_shared[r][best]
            if cand_dist is not None:
                dist[r], strand[r] = cand_dist[r][best], cand_strand[r][best]
    return reference, strand, dist, shared


# ---- rules M1 to M6 ------------------------------------------------------------------------------------------------------
def expected(reads, refs, k=13, buckets=64, min_shared=2, max_candidates=4, identity=0.8, bandwidth=100, both_strands=True):
    """What referenceGroups returns for reads and references given as bytes."""
    n, nf = len(reads), len(refs)
    if n == 0 or nf == 0:
        minus = np.full(n, -1, np.int32)
        out = {"reference": minus, "strand": np.zeros(n, np.uint8), "dist": minus.copy(), "shared": np.zeros(n, np.int32),
               "n.candidates": np.zeros(n, np.int32), "n.kmers": minus.copy(), "ref.n.kmers": np.full(nf, -1, np.int32),
               "group": minus.copy(), "groups": split_labels(minus), "n.hits": np.int64(0)}
        return dict(out, **({} if identity is None else {"n.checked": np.int64(0)}))
    fsk, fnk = S.sketches(refs, k, buckets, both_strands)                                              # M1
    rsk, rnk = S.sketches(reads, k, buckets, both_strands)
    shared, nhits = hits_of(fsk, rsk)                                                                  # M2
    cand_ref, cand_shared, ncand = candidates_of(shared, n, min_shared, max_candidates)                # M3
    checked = {}
    if identity is None:
        reference, strand, dist, sh = choose(cand_ref, cand_shared)                                    # M5
    else:
        cd, cs, nchecked = check_slots(refs, reads, cand_ref, V.max_diff_ppm(identity), bandwidth, both_strands)      # M4
        reference, strand, dist, sh = choose(cand_ref, cand_shared, cd, cs)
        checked["n.checked"] = np.int64(nchecked)
    return {"reference": reference, "strand": strand, "dist": dist, "shared": sh, "n.candidates": ncand, "n.kmers": rnk,
            "ref.n.kmers": fnk, "group": reference.copy(), "groups": split_labels(reference), "n.hits": np.int64(nhits), **checked}     # M6


def same(got, want, what=""):
    """Every entry of two referenceGroups results, exactly, dtype included."""
    assert set(got) == set(want), (what, sorted(got), sorted(want))
    for key in ("reference", "dist", "shared", "n.candidates", "n.kmers", "ref.n.kmers", "group"):
        assert got[key].dtype == np.int32 and np.array_equal(got[key], want[key]), (what, key, got[key][:20], want[key][:20])
    assert got["strand"].dtype == np.uint8 and np.array_equal(got["strand"], want["strand"]), (what, "strand")
    assert got["groups"][0].dtype == np.int64 and got["groups"][1].dtype == np.int32, what
    assert np.array_equal(got["groups"][0], want["groups"][0]) and np.array_equal(got["groups"][1], want["groups"][1]), (what, "groups")
    for key in ("n.hits", "n.checked"):
        if key in want:
            assert isinstance(got[key], np.int64) and int(got[key]) == int(want[key]), (what, key, got[key], want[key])


# ---- cases ---------------------------------------------------------------------------------------------------------------
E = EMPTY
# Two references, three reads, four buckets (rules M2 to M5 do not care how many, nor whether a hash lies in its bucket's
# range).  Hits: read 0 with reference 0 in buckets 0, 1, 3 and with reference 1 in bucket 2; read 1 with reference 0 in
# bucket 0 and with reference 1 in buckets 1, 2; read 2 with nothing (its 20 stands in another bucket than reference
# 0's, its 31 in another than reference 1's).
HAND_REFS = [[10, 20, 30, 40],
             [11, 21, 31, E]]
HAND_READS = [[10, 20, 31, 40],
              [10, 21, 31, E],
              [20, 31, E, E]]
HAND_SHARED = {(0, 0): 3, (0, 1): 1, (1, 0): 1, (1, 1): 2}
HAND_HITS = 7

# (rates, min_shared, identity) of the planted sets: every read on its own transcript
PLANTED = [((0.05, 0.01), 1, 0.8), ((0.05, 0.01), 2, 0.8), ((0.05, 0.01), 3, 0.8), ((0.10, 0.02), 1, 0.7)]


def planted_set(seed, sub_rate, indel_rate, transcripts=8, copies=6, length=300, shared=100):
    """(reads as bytes, transcript of every read, transcripts as bytes): V.planted_set, draw for draw, with its
    transcripts returned as the references."""
    rng = np.random.default_rng(seed)
    truth = [bytearray(S.random_bases(rng, length)) for _ in range(transcripts)]
    for j in range(1, transcripts, 2):
        truth[j][200:200 + shared] = truth[j - 1][200:200 + shared]
    refs = [bytes(t) for t in truth]
    truth = [np.frombuffer(t, np.uint8) for t in refs]
    reads = [(mock.mutate(t, rng, sub_rate=sub_rate, indel_rate=indel_rate).tobytes(), j) for j, t in enumerate(truth) for _ in range(copies)]
    reads = [reads[i] for i in rng.permutation(len(reads))]
    reads = [(mock.revcomp(s).encode() if i % 2 else s, j) for i, (s, j) in enumerate(reads)]
    return [s for s, _ in reads], np.array([j for _, j in reads], np.int32), refs


def in_bucket(sketch, buckets):
    """A hand-set sketch array (small values, EMPTY) with every value moved into its column's bucket range, as the device
    call requires of its input: value v of column j becomes j << (64 - log2 buckets) | v."""
    sk = np.asarray(sketch, np.uint64).copy()
    shift = np.uint64(64 - (buckets.bit_length() - 1))
    for j in range(sk.shape[1]):
        col = sk[:, j]
        col[col != np.uint64(EMPTY)] |= np.uint64(j) << shift
    return sk


def hand_sketch_pair(ref_rows, read_rows, buckets=16):
    """(reference sketches, read sketches) of `buckets` columns from rows of a few small values (E: empty), the columns
    beyond a row's length empty."""
    def widen(rows):
        sk = np.full((len(rows), buckets), EMPTY, np.uint64)
        for i, row in enumerate(rows):
            sk[i, :len(row)] = np.array(row, np.uint64)
        return in_bucket(sk, buckets)
    return widen(ref_rows), widen(read_rows)
