"""Plain-Python / numpy restatement of generics.sequenceGroups (sarlacc_amd/sketch.py, csrc/sketch.hip; the rules are
DESIGN §4.19, numbered here as there) and the cases its tests share.  Everything is integers; nothing here touches the
library.  tests/test_sketch_host.py pins the restatement on literals worked out by hand; tests/test_gpu_sketch.py holds
the device to it.

Two restatements of rules 1 to 4 stand side by side: one k-mer at a time on Python integers (kmer_value,
revcomp_value, fmix64, read_hashes), which the literals pin, and the same on numpy columns (read_hashes_np), which the
host test holds to the first and the long reads of the device tests use."""
import numpy as np

from sarlacc_amd import mock
from tests.read_groups_cases import split_labels

M64 = (1 << 64) - 1
EMPTY = M64
CODES = {ord("A"): 0, ord("C"): 1, ord("G"): 2, ord("T"): 3}                  # rule 1
_CODE_OF = np.full(256, 255, np.uint8)
for _b, _c in CODES.items():
    _CODE_OF[_b] = _c


def as_bytes(s):
    return s.encode("latin-1") if isinstance(s, str) else bytes(s)


# ---- rules 2 and 3, one k-mer at a time ----------------------------------------------------------------------------------
def kmer_value(kmer):
    """lo | hi << 32 of k valid bases: bit i of lo / hi is the low / high code bit of base i."""
    lo = hi = 0
    for i, b in enumerate(as_bytes(kmer)):
        lo |= (CODES[b] & 1) << i
        hi |= (CODES[b] >> 1) << i
    return lo | (hi << 32)


def revcomp_value(x, k):
    """The value of the reverse complement: both planes inverted and bit-reversed within k bits."""
    out = 0
    for shift in (0, 32):
        plane = (x >> shift) & 0xffffffff
        out |= sum((1 - ((plane >> i) & 1)) << (k - 1 - i) for i in range(k)) << shift
    return out


def fmix64(x):
    x ^= x >> 33
    x = (x * 0xff51afd7ed558ccd) & M64
    x ^= x >> 33
    x = (x * 0xc4ceb9fe1a85ec53) & M64
    x ^= x >> 33
    return x


def read_hashes(seq, k, canonical=True):
    """The hashes of the present k-mers of one read, in read order."""
    seq = as_bytes(seq)
    out = []
    for p in range(len(seq) - k + 1):
        kmer = seq[p:p + k]
        if any(b not in CODES for b in kmer):
            continue
        x = kmer_value(kmer)
        if canonical:
            x = min(x, revcomp_value(x, k))
        h = fmix64(x)
        if h != EMPTY:
            out.append(h)
    return out


# ---- the same on numpy columns -------------------------------------------------------------------------------------------
def read_hashes_np(seq, k, canonical=True):
    code = _CODE_OF[np.frombuffer(as_bytes(seq), np.uint8)]
    npos = code.size - k + 1
    if npos <= 0:
        return np.zeros(0, np.uint64)
    bad = np.concatenate([[0], np.cumsum(code > 3)])
    ok = (bad[k:] - bad[:-k]) == 0
    c = (code & 3).astype(np.uint64)
    lo, hi, rlo, rhi = (np.zeros(npos, np.uint64) for _ in range(4))
    one = np.uint64(1)
    for i in range(k):
        col = c[i:i + npos]
        lo |= (col & one) << np.uint64(i)
        hi |= (col >> one) << np.uint64(i)
        rlo |= (one - (col & one)) << np.uint64(k - 1 - i)
        rhi |= (one - (col >> one)) << np.uint64(k - 1 - i)
    x = lo | (hi << np.uint64(32))
    if canonical:
        x = np.minimum(x, rlo | (rhi << np.uint64(32)))
    x = x[ok]
    with np.errstate(over="ignore"):
        x ^= x >> np.uint64(33)
        x *= np.uint64(0xff51afd7ed558ccd)
        x ^= x >> np.uint64(33)
        x *= np.uint64(0xc4ceb9fe1a85ec53)
        x ^= x >> np.uint64(33)
    return x[x != np.uint64(EMPTY)]


# ---- rule 4 --------------------------------------------------------------------------------------------------------------
def sketch_of(hashes, buckets):
    """(uint64[buckets] minima, number of k-mers) from a read's hashes."""
    h = np.asarray(hashes, np.uint64)
    sk = np.full(buckets, EMPTY, np.uint64)
    shift = np.uint64(64 - (buckets.bit_length() - 1))
    np.minimum.at(sk, (h >> shift).astype(np.int64), h)
    return sk, h.size


def sketches(seqs, k, buckets, canonical=True):
    """(uint64[n, buckets], int32[n]) of a list of reads."""
    rows = [sketch_of(read_hashes_np(s, k, canonical), buckets) for s in seqs]
    sk = np.array([r[0] for r in rows], np.uint64).reshape(len(rows), buckets)
    return sk, np.array([r[1] for r in rows], np.int32)


# ---- rules 5 and 6 -------------------------------------------------------------------------------------------------------
def shared_counts(sketch, window):
    """{(a, b): shared(a, b)} of the reads a < b, from the sorted non-empty entries."""
    sketch = np.asarray(sketch, np.uint64)
    entries = sorted((int(h), r) for r, row in enumerate(sketch) for h in row if int(h) != EMPTY)
    shared = {}
    for p, (h, b) in enumerate(entries):
        for d in range(1, window + 1):
            if p - d >= 0 and entries[p - d][0] == h:
                pair = (entries[p - d][1], b)
                shared[pair] = shared.get(pair, 0) + 1
    return shared


def links_of(sketch, window, min_shared):
    """(links as uint64 a << 32 | b ascending, n.pairs, n.links)."""
    shared = shared_counts(sketch, window)
    links = sorted(pair for pair, c in shared.items() if c >= min_shared)
    return np.array([(a << 32) | b for a, b in links], np.uint64), len(shared), len(links)


# ---- rule 7 --------------------------------------------------------------------------------------------------------------
def components_of(links, n, nkmers=None):
    """int32 labels by union-find; groups numbered in ascending order of their lowest vertex, -1 where nkmers is 0."""
    counted = [True] * n if nkmers is None else [int(c) > 0 for c in nkmers]
    parent = list(range(n))

    def find(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v
    for link in links:
        a, b = int(link) >> 32, int(link) & 0xffffffff
        if counted[a] and counted[b]:
            ra, rb = find(a), find(b)
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)
    label, number = np.full(n, -1, np.int32), {}
    for v in range(n):
        if counted[v]:
            label[v] = number.setdefault(find(v), len(number))
    return label


def expected(seqs, k=13, buckets=64, window=8, min_shared=3, canonical=True):
    """What sequenceGroups returns."""
    sk, nk = sketches(seqs, k, buckets, canonical)
    links, npairs, nlinks = links_of(sk, window, min_shared)
    group = components_of(links, len(seqs), nk)
    return {"group": group, "groups": split_labels(group), "n.kmers": nk, "n.pairs": np.int64(npairs), "n.links": np.int64(nlinks)}


def same(got, want, what=""):
    """Every entry of two sequenceGroups results, exactly, dtype included."""
    for key in ("group", "n.kmers"):
        assert got[key].dtype == np.int32 and np.array_equal(got[key], want[key]), (what, key, got[key][:20], want[key][:20])
    assert got["groups"][0].dtype == np.int64 and got["groups"][1].dtype == np.int32, what
    assert np.array_equal(got["groups"][0], want["groups"][0]) and np.array_equal(got["groups"][1], want["groups"][1]), (what, "groups")
    for key in ("n.pairs", "n.links"):
        assert isinstance(got[key], np.int64) and int(got[key]) == int(want[key]), (what, key, got[key], want[key])


# ---- cases ---------------------------------------------------------------------------------------------------------------
E = EMPTY
# three reads, four buckets (the rules do not care how many): sorted entries (10,0) (10,1) (11,2) (20,0) (20,1) (30,1)
# (30,2) (40,0) (40,2); pairs 0-1 (hash 10), 0-1 (20), 1-2 (30), 0-2 (40)
THREE_READS = [[10, 20, E, 40],
               [10, 20, 30, E],
               [11, E, 30, 40]]
THREE_SHARED = {(0, 1): 2, (1, 2): 1, (0, 2): 1}

SEEDS = (1, 2, 3)             # of the 12 x 10 mock set, on the host and on the device


def random_bases(rng, length):
    return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, length)].tobytes()


def mock_set(seed, transcripts=12, copies=10, length=600, sub_rate=0.05, indel_rate=0.01, shuffle=True, flip=True):
    """(reads as bytes, transcript of every read): `copies` noisy copies (mock.mutate) of each of `transcripts` random
    sequences, shuffled, every second read of the shuffled order reverse-complemented."""
    rng = np.random.default_rng(seed)
    truth = [np.frombuffer(random_bases(rng, length), np.uint8) for _ in range(transcripts)]
    reads = [(mock.mutate(t, rng, sub_rate=sub_rate, indel_rate=indel_rate).tobytes(), j) for j, t in enumerate(truth) for _ in range(copies)]
    if shuffle:
        reads = [reads[i] for i in rng.permutation(len(reads))]
    if flip:
        reads = [(mock.revcomp(s).encode() if i % 2 else s, j) for i, (s, j) in enumerate(reads)]
    return [s for s, _ in reads], np.array([j for _, j in reads], np.int32)


def one_group_per_transcript(group, transcript):
    """Every transcript in one group and no group with two transcripts."""
    pairs = set(zip(group.tolist(), transcript.tolist()))
    return (group >= 0).all() and len(pairs) == len(set(transcript.tolist())) == len(set(group.tolist()))


def length_reads(k, seed=7):
    """Random reads of the lengths at which k_sketch takes another path: around k, around one and two 64-base words, a
    k-mer that spans two words, many words, and one read of about 70 000 bases."""
    rng = np.random.default_rng(seed)
    lengths = [0, k - 1, k, k + 1, 63, 64, 65, 63 + k, 64 + k, 127, 128, 129, 5003, 70001, 1, 200]
    return [random_bases(rng, n) for n in lengths]


def invalid_reads(k, seed=8):
    """Reads of 129 + k bases with a byte that is no base -- N, lower case, a byte >= 128 -- at base 0, at the last base, at
    bases 63 and 64, and at every k-th base (no k-mer at all), and a read of nothing but N."""
    rng = np.random.default_rng(seed)
    out = []
    for bad in (ord("N"), ord("a"), ord("t"), 0x80, 0xc7, 0xff, 0):
        for where in ("first", "last", "63", "64", "63+64", "every"):
            s = bytearray(random_bases(rng, 129 + k))
            at = {"first": [0], "last": [len(s) - 1], "63": [63], "64": [64], "63+64": [63, 64], "every": range(k - 1, len(s), k)}[where]
            for p in at:
                s[p] = bad
            out.append(bytes(s))
    out.append(b"N" * 100)
    return out


def hand_sketches(runs, buckets=16, n=None):
    """A sketch array in which run j -- a list of reads -- shares the hash 1000 + j, one run per bucket column j % buckets,
    every other entry empty or private.  Hashes need not lie in their bucket's range: the link stage reads the array as a
    set of (hash, read) entries."""
    n = (max(max(r) for r in runs if r) + 1) if n is None else n
    sk = np.full((n, buckets), EMPTY, np.uint64)
    for j, reads in enumerate(runs):
        assert j < buckets
        for r in reads:
            sk[r, j] = 1000 + j
    return sk
