"""Plain-numpy restatement of rule 6a of DESIGN §4.19 -- the alignment check of sequenceGroups' links
(sarlacc_dev_links_verify, csrc/links_verify.hip) -- and the cases its tests share.  Everything is integers; nothing here
touches the library.  tests/test_links_verify_host.py pins the restatement on an unbanded Levenshtein distance and on
literals worked out by hand; tests/test_gpu_links_verify.py and tests/test_gpu_sequence_groups_identity.py hold the
device to it.

The distance works column by column on the band alone, many pairs side by side: cell k of column j is row i = j - w + k,
its diagonal neighbour is cell k of column j - 1 and its left neighbour cell k + 1; the dependency on the cell above is
resolved by np.minimum.accumulate(tmp - idx) + idx."""
import numpy as np

from sarlacc_amd import mock
from tests import sketch_cases as sc
from tests.read_groups_cases import split_labels

PPM = 10 ** 6
INF = 1 << 40                                         # above every distance; sums of two stay inside int64
_CODE_OF = np.full(256, 4, np.uint8)                  # rule 6a.1: A, C, G, T in upper case; every other byte is no base
for _b, _c in sc.CODES.items():
    _CODE_OF[_b] = _c
_RC = np.arange(256, dtype=np.uint8)
for _p, _q in ("AT", "TA", "CG", "GC"):
    _RC[ord(_p)] = ord(_q)


def rc(seq):
    """Reversed, with A <-> T and C <-> G; every other byte stays what it is."""
    return _RC[np.frombuffer(sc.as_bytes(seq), np.uint8)][::-1].tobytes()


def max_diff_ppm(identity):
    return int(round((1.0 - identity) * PPM))


def threshold(ppm, la, lb):
    """Rule 6a.3: the largest distance with which a pair of these lengths passes."""
    return (ppm * max(la, lb)) // PPM


def levenshtein(x, y):
    """The unbanded unit-cost distance under rule 6a.1's equality, row by row on Python integers."""
    x, y = _CODE_OF[np.frombuffer(sc.as_bytes(x), np.uint8)].tolist(), _CODE_OF[np.frombuffer(sc.as_bytes(y), np.uint8)].tolist()
    row = list(range(len(y) + 1))
    for i, a in enumerate(x, 1):
        new = [i]
        for j, b in enumerate(y, 1):
            new.append(min(row[j - 1] + (0 if a == b and a < 4 else 1), row[j] + 1, new[j - 1] + 1))
        row = new
    return row[len(y)]


def banded_many(xs, ys, w):
    """D_w(x, y) of every pair, None where it is infinite (the lengths differ by more than w).  Pairs whose second reads are
    of like length (the same number of binary digits) share a pass over the columns."""
    out = [None] * len(xs)
    classes = {}
    for p in range(len(xs)):
        if abs(len(xs[p]) - len(ys[p])) <= w:
            classes.setdefault(len(ys[p]).bit_length(), []).append(p)
    for todo in classes.values():
        _banded_class(xs, ys, w, todo, out)
    return out


def _banded_class(xs, ys, w, todo, out):
    la = np.array([len(xs[p]) for p in todo], np.int64)
    lb = np.array([len(ys[p]) for p in todo], np.int64)
    band, npair = 2 * w + 1, len(todo)
    # x with w + 1 cells in front and enough behind: the rows of column j are xrow[:, j : j + band]; 5 and 6 equal nothing
    xrow = np.full((npair, int(lb.max()) + band + 1), 5, np.uint8)
    ycol = np.full((npair, int(lb.max()) + 1), 6, np.uint8)
    for q, p in enumerate(todo):
        cx, cy = _CODE_OF[np.frombuffer(sc.as_bytes(xs[p]), np.uint8)], _CODE_OF[np.frombuffer(sc.as_bytes(ys[p]), np.uint8)]
        cx = cx[:xrow.shape[1] - (w + 1)]                  # rows below every band
        xrow[q, w + 1:w + 1 + cx.size] = np.where(cx < 4, cx, 5)
        ycol[q, :cy.size] = np.where(cy < 4, cy, 6)
    idx = np.arange(band, dtype=np.int64)
    rows0 = idx - w                                        # rows of column 0
    prev = np.where((rows0 >= 0) & (rows0[None, :] <= la[:, None]), rows0[None, :], INF).astype(np.int64)      # D(i, 0) = i
    final = np.where(lb == 0, prev[np.arange(npair), np.minimum(la + w, band - 1)], INF)
    left = np.full((npair, band), INF, np.int64)
    for j in range(1, int(lb.max()) + 1):
        rows = rows0 + j
        cost = (xrow[:, j:j + band] != ycol[:, j - 1:j]).astype(np.int64)
        left[:, :-1] = prev[:, 1:]
        tmp = np.minimum(prev + cost, left + 1)
        tmp[(rows[None, :] < 0) | (rows[None, :] > la[:, None])] = INF
        tmp[:, rows == 0] = j if j <= w else INF           # D(0, j) = j inside the band
        new = np.minimum.accumulate(tmp - idx, axis=1) + idx
        new[(rows[None, :] < 0) | (rows[None, :] > la[:, None]) | (new >= INF)] = INF
        done = np.flatnonzero(lb == j)
        final[done] = new[done, la[done] - j + w]
        prev = new
    for q, p in enumerate(todo):
        out[p] = int(final[q]) if final[q] < INF else None


def banded(x, y, w):
    return banded_many([x], [y], w)[0]


def verify_pairs(xs, ys, ppm, w, both_strands=True):
    """Rule 6a.4 on pairs of reads: (int32 dist, -1 where the pair fails; uint8 strand)."""
    t = [threshold(ppm, len(x), len(y)) for x, y in zip(xs, ys)]
    dist, strand = np.full(len(xs), -1, np.int32), np.zeros(len(xs), np.uint8)
    forward = banded_many(xs, ys, w)
    for p, d in enumerate(forward):
        if d is not None and d <= t[p]:
            dist[p] = d
    if both_strands:
        rest = np.flatnonzero(dist < 0).tolist()
        reverse = banded_many([xs[p] for p in rest], [rc(ys[p]) for p in rest], w)
        for p, d in zip(rest, reverse):
            if d is not None and d <= t[p]:
                dist[p], strand[p] = d, 1
    return dist, strand


def verify(seqs, links, ppm, w, both_strands=True):
    """What sarlacc_dev_links_verify returns for the links a << 32 | b over `seqs`: (kept links in input order, int32
    dist, uint8 strand)."""
    links = np.asarray(links, np.uint64)
    distinct, which = np.unique(links, return_inverse=True)          # a repeated link is worked out once
    a, b = (distinct >> np.uint64(32)).astype(np.int64), (distinct & np.uint64(0xffffffff)).astype(np.int64)
    dist, strand = verify_pairs([seqs[i] for i in a], [seqs[i] for i in b], ppm, w, both_strands)
    dist, strand = dist[which], strand[which]
    return links[dist >= 0], dist, strand


def expected(seqs, k=13, buckets=64, window=8, min_shared=3, canonical=True, identity=None, bandwidth=100):
    """What sequenceGroups(..., identity=, bandwidth=) returns."""
    if identity is None:
        return sc.expected(seqs, k, buckets, window, min_shared, canonical)
    sk, nk = sc.sketches(seqs, k, buckets, canonical)
    links, npairs, nlinks = sc.links_of(sk, window, min_shared)
    kept, _, _ = verify(seqs, links, max_diff_ppm(identity), bandwidth, bool(canonical))
    group = sc.components_of(kept, len(seqs), nk)
    return {"group": group, "groups": split_labels(group), "n.kmers": nk, "n.pairs": np.int64(npairs), "n.links": np.int64(nlinks),
            "n.verified": np.int64(kept.size)}


def same(got, want, what=""):
    """Every entry of two sequenceGroups(identity=) results, exactly."""
    sc.same(got, want, what)
    assert set(got) == set(want), (what, sorted(got))
    if "n.verified" in want:
        assert isinstance(got["n.verified"], np.int64) and int(got["n.verified"]) == int(want["n.verified"]), (what, got["n.verified"], want["n.verified"])


# ---- cases ---------------------------------------------------------------------------------------------------------------
PLANTED = (((0.05, 0.01), 3, 0.8), ((0.10, 0.02), 1, 0.7))      # (rates, min_shared, identity): one group per transcript


def planted_set(seed, sub_rate, indel_rate, transcripts=8, copies=6, length=300, shared=100):
    """(reads as bytes, transcript of every read): transcripts of which every odd one carries `shared` bases of the one
    before it at the same place, `copies` noisy copies of each, shuffled, every second read of the shuffled order
    reverse-complemented.  No sketch setting separates neighbours that share a third of their bases; the reads do."""
    rng = np.random.default_rng(seed)
    truth = [bytearray(sc.random_bases(rng, length)) for _ in range(transcripts)]
    for j in range(1, transcripts, 2):
        truth[j][200:200 + shared] = truth[j - 1][200:200 + shared]
    truth = [np.frombuffer(bytes(t), np.uint8) for t in truth]
    reads = [(mock.mutate(t, rng, sub_rate=sub_rate, indel_rate=indel_rate).tobytes(), j) for j, t in enumerate(truth) for _ in range(copies)]
    reads = [reads[i] for i in rng.permutation(len(reads))]
    reads = [(mock.revcomp(s).encode() if i % 2 else s, j) for i, (s, j) in enumerate(reads)]
    return [s for s, _ in reads], np.array([j for _, j in reads], np.int32)


def links_between(pairs):
    """uint64 links of (a, b) tuples."""
    return np.array([(a << 32) | b for a, b in pairs], np.uint64)


def noisy(rng, seq, nsub=0, ndel=0, nins=0):
    """A copy of `seq` with substitutions to another base, deletions and insertions at distinct random places away from
    its ends."""
    s = bytearray(seq)
    places = rng.choice(np.arange(2, len(s) - 2), nsub + ndel + nins, replace=False).tolist()
    kinds = ["sub"] * nsub + ["del"] * ndel + ["ins"] * nins
    for p, kind in sorted(zip(places, kinds), reverse=True):
        if kind == "sub":
            s[p] = ord("ACGT"[("ACGT".index(chr(s[p])) + 1 + int(rng.integers(0, 3))) % 4])
        elif kind == "del":
            del s[p]
        else:
            s.insert(p, ord("ACGT"[int(rng.integers(0, 4))]))
    return bytes(s)
