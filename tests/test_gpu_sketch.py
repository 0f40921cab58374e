"""sequenceGroups on the device (csrc/sketch.hip: sarlacc_dev_sketch_reads / _sketch_links / _components,
sarlacc_amd/sketch.py, generics.sequenceGroups), compared exactly with tests/sketch_cases.py, the plain-Python
restatement that tests/test_sketch_host.py pins.  Everything is integers: no tolerance.

k_sketch takes 64 bases of a read per step of the wavefront and a k-mer may span two steps, so the read lengths tried
sit around k, 64, 64 + k and 128; every batch is uploaded at its exact size, so its last read ends at the buffer's last
byte.  The link and component stages are fed arrays built by hand, so that every count is known."""
import ctypes as C

import numpy as np
import pytest

from tests import sketch_cases as S

pytestmark = pytest.mark.gpu


def _device_reads(seqs):
    """A resident batch whose buffers are exactly as long as the reads."""
    from sarlacc_amd.resident import DevBuffer, DeviceReads
    chars = np.frombuffer(b"".join(seqs), np.uint8)
    off = np.zeros(len(seqs) + 1, np.int64)
    np.cumsum([len(s) for s in seqs], out=off[1:])
    assert chars.size and len(seqs[-1]) > 0
    return DeviceReads(DevBuffer.from_numpy(chars), DevBuffer.from_numpy(chars), DevBuffer.from_numpy(off), off, None)


def _check_sketch(seqs, k, buckets, canonical, what):
    sk, nk = _device_reads(seqs).sketch(k, buckets, canonical)
    want_sk, want_nk = S.sketches(seqs, k, buckets, canonical)
    assert sk.dtype == np.uint64 and sk.shape == (len(seqs), buckets) and nk.dtype == np.int32
    assert np.array_equal(nk, want_nk), (what, nk.tolist(), want_nk.tolist())
    rows = np.flatnonzero((sk != want_sk).any(axis=1))
    assert rows.size == 0, (what, "reads", rows[:10].tolist(), [len(seqs[r]) for r in rows[:10]])
    return sk, nk


# ---- sketch ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("canonical", [True, False], ids=["canonical", "stranded"])
@pytest.mark.parametrize("buckets", [16, 64, 256])
@pytest.mark.parametrize("k", [5, 13, 16, 31])
def test_sketch_at_every_length(k, buckets, canonical):
    seqs = S.length_reads(k)
    sk, nk = _check_sketch(seqs, k, buckets, canonical, "k %d, %d buckets" % (k, buckets))
    assert nk[:4].tolist() == [0, 0, 1, 2] and nk[13] == 70001 - k + 1
    assert (sk[:2] == np.uint64(S.EMPTY)).all() and (sk[2] != np.uint64(S.EMPTY)).sum() == 1


@pytest.mark.parametrize("canonical", [True, False], ids=["canonical", "stranded"])
@pytest.mark.parametrize("k", [5, 13, 16, 31])
def test_sketch_with_bytes_that_are_no_base(k, canonical):
    seqs = S.invalid_reads(k)
    sk, nk = _check_sketch(seqs, k, 64, canonical, "k %d" % k)
    every = np.arange(5, len(seqs) - 1, 6)                  # the reads with such a byte at every k-th base
    assert (nk[every] == 0).all() and (sk[every] == np.uint64(S.EMPTY)).all() and nk[-1] == 0
    assert (nk[np.arange(0, len(seqs) - 1, 6)] == 129).all()      # at base 0: one k-mer fewer


def test_a_read_and_its_reverse_complement():
    from sarlacc_amd import mock
    rng = np.random.default_rng(3)
    fwd = [S.random_bases(rng, n) for n in (40, 64, 129, 700, 3000)]
    rev = [mock.revcomp(s).encode() for s in fwd]
    for k in (5, 13, 16, 31):
        sk, nk = _check_sketch(fwd + rev, k, 64, True, "canonical, k %d" % k)
        assert np.array_equal(sk[:5], sk[5:]) and np.array_equal(nk[:5], nk[5:])
        sk, nk = _check_sketch(fwd + rev, k, 64, False, "stranded, k %d" % k)
        assert all((sk[i] != sk[5 + i]).any() for i in range(5)) and np.array_equal(nk[:5], nk[5:])


def test_sketch_refuses_offsets_that_do_not_ascend():
    from sarlacc_amd import sketch
    from sarlacc_amd._lib import SarlaccError
    from sarlacc_amd.resident import DevBuffer
    chars = np.frombuffer(S.random_bases(np.random.default_rng(1), 100), np.uint8)
    for off, message in (([0, 50, 40, 100], "read 2: its offsets"), ([0, 50, 120, 100], "read 2: its offsets"), ([-1, 50, 60, 100], "read 1: its offsets")):
        with pytest.raises(SarlaccError, match=message):
            sketch.sketch_reads(DevBuffer.from_numpy(chars), DevBuffer.from_numpy(np.array(off, np.int64)), 3, 13, 64)


# ---- links -----------------------------------------------------------------------------------------------------------------
def _links(sk, window, min_shared):
    from sarlacc_amd import sketch
    from sarlacc_amd.resident import DevBuffer
    sk = np.ascontiguousarray(sk, np.uint64)
    n, buckets = sk.shape
    d_links, npairs, nlinks = sketch.sketch_links(DevBuffer.from_numpy(sk), n, buckets, window, min_shared)
    return d_links.to_numpy(np.uint64, nlinks).copy(), npairs, nlinks


def _check_links(sk, window, min_shared, what):
    got, want = _links(sk, window, min_shared), S.links_of(sk, window, min_shared)
    assert got[1:] == want[1:], (what, got[1:], want[1:])
    assert got[0].dtype == np.uint64 and np.array_equal(got[0], want[0]), (what, got[0][:10], want[0][:10])
    return [(int(x) >> 32, int(x) & 0xffffffff) for x in got[0]]


@pytest.mark.parametrize("window", [1, 2, 8, 64])
def test_links_of_runs_around_the_window(window):
    """Runs of 1, 2, window, window + 1, window + 2 and 3 window reads that hold one hash each: up to window + 1 reads give
    all their pairs, longer runs the band of distance <= window."""
    lengths = [1, 2, window, window + 1, window + 2, 3 * window]
    first = np.concatenate([[0], np.cumsum(lengths)])
    runs = [list(range(first[j], first[j + 1])) for j in range(len(lengths))]
    links = _check_links(S.hand_sketches(runs), window, 1, "window %d" % window)
    by_run = [[(a, b) for a, b in links if first[j] <= a < first[j + 1]] for j in range(len(lengths))]
    assert all(first[j] <= b < first[j + 1] for j in range(len(lengths)) for _, b in by_run[j])
    full = lambda m: m * (m - 1) // 2
    band = lambda m: sum(min(window, m - 1 - i) for i in range(m))
    assert [len(x) for x in by_run] == [0, 1, full(window), full(window + 1), band(window + 2), band(3 * window)]
    a = int(first[4])
    assert (a, a + window) in links and (a, a + window + 1) not in links and (a + 1, a + window + 1) in links


@pytest.mark.parametrize("min_shared", [1, 2, 3, 16])
def test_links_need_min_shared_entries(min_shared):
    """Reads 0 and 1 share min_shared - 1 buckets, reads 2 and 3 share min_shared."""
    sk = S.hand_sketches([[0, 1]] * (min_shared - 1), n=4)
    for j in range(min_shared):
        sk[2, j] = sk[3, j] = 5000 + j
    links = _check_links(sk, 8, min_shared, "min_shared %d" % min_shared)
    assert links == [(2, 3)]
    assert _links(sk, 8, min_shared)[1] == (2 if min_shared > 1 else 1)


def test_links_of_identical_sketches_empty_sketches_and_one_read():
    row = np.arange(100, 116, dtype=np.uint64)
    for n, window in ((2, 8), (9, 8), (10, 8), (30, 8), (30, 1), (70, 64)):
        links = _check_links(np.tile(row, (n, 1)), window, 16, "%d identical reads, window %d" % (n, window))
        assert len(links) == sum(min(window, n - 1 - i) for i in range(n))
    assert _links(np.tile(row, (30, 1)), 8, 16)[1:] == (30 * 8 - 36, 30 * 8 - 36)
    for n in (1, 2, 200):
        got = _links(np.full((n, 64), S.EMPTY, np.uint64), 8, 1)
        assert got[0].size == 0 and got[1:] == (0, 0)
    got = _links(np.arange(64, dtype=np.uint64)[None, :], 8, 1)
    assert got[0].size == 0 and got[1:] == (0, 0)


@pytest.mark.parametrize("buckets, window, min_shared, values", [(16, 64, 1, 25), (64, 8, 3, 25), (256, 1, 2, 25), (64, 3, 1, 25),
                                                                 (16, 8, 6, 3), (16, 16, 8, 3)])
def test_links_of_random_sketches(buckets, window, min_shared, values):
    """300 reads whose buckets draw from few values, a tenth of them empty: long runs, many pairs, shared counts around
    min_shared."""
    rng = np.random.default_rng(buckets + window)
    n = 300
    sk = (rng.integers(0, values, (n, buckets)) + 1000 * np.arange(buckets)[None, :]).astype(np.uint64)
    sk[rng.random((n, buckets)) < 0.1] = np.uint64(S.EMPTY)
    links = _check_links(sk, window, min_shared, "random")
    assert len(links) > 50 and all(a < b for a, b in links)


def test_links_sizing_and_capacity():
    """d_links = NULL only counts; a capacity below the number of links gets the first links and the full number."""
    from sarlacc_amd import _lib
    from sarlacc_amd._lib import check
    from sarlacc_amd.resident import DevBuffer
    sk = S.hand_sketches([list(range(12))])
    want, npairs, nlinks = S.links_of(sk, 8, 1)
    d_sk = DevBuffer.from_numpy(sk)
    got_pairs, got_links = C.c_int64(-1), C.c_int64(-1)
    check(_lib.lib().sarlacc_dev_sketch_links(d_sk, 12, 16, 8, 1, None, 0, C.byref(got_pairs), C.byref(got_links), None))
    assert (got_pairs.value, got_links.value) == (npairs, nlinks) == (60, 60)
    room = DevBuffer.from_numpy(np.full(8, 77, np.uint64))
    check(_lib.lib().sarlacc_dev_sketch_links(d_sk, 12, 16, 8, 1, room, 5, C.byref(got_pairs), C.byref(got_links), None))
    assert got_links.value == 60
    assert room.to_numpy(np.uint64, 8).tolist() == want[:5].tolist() + [77, 77, 77]


# ---- components ------------------------------------------------------------------------------------------------------------
def _components(links, n, nkmers=None):
    from sarlacc_amd import sketch
    from sarlacc_amd.resident import DevBuffer
    links = np.array([(int(a) << 32) | int(b) for a, b in links], np.uint64)
    d_nk = None if nkmers is None else DevBuffer.from_numpy(np.asarray(nkmers, np.int32))
    d_label, ngroups = sketch.components(DevBuffer.from_numpy(links if links.size else np.zeros(1, np.uint64)), links.size, n, d_nk)
    label = d_label.to_numpy(np.int32, n).copy()
    want = S.components_of(links, n, nkmers)
    assert np.array_equal(label, want), (label[:20], want[:20])
    assert ngroups == int(label.max()) + 1 if (label >= 0).any() else ngroups == 0
    seen = label[label >= 0]
    heads = seen[np.sort(np.unique(seen, return_index=True)[1])]
    assert np.array_equal(heads, np.arange(heads.size))      # labels ascend by lowest member
    return label


def test_components_without_links():
    assert _components([], 1).tolist() == [0]
    assert _components([], 700).tolist() == list(range(700))


def test_components_of_paths():
    n = 2000
    up = [(v, v + 1) for v in range(n - 1)]
    assert (_components(up, n) == 0).all()
    assert (_components(up[::-1], n) == 0).all()
    assert (_components([(b, a) for a, b in up], n) == 0).all()
    perm = np.random.default_rng(4).permutation(n)
    shuffled = [(perm[a], perm[b]) for a, b in up]
    assert (_components(shuffled, n) == 0).all()
    two = [(perm[a], perm[b]) for a, b in up if a != 1000]      # cut once: two paths
    assert np.unique(_components(two, n)).tolist() == [0, 1]


def test_components_of_a_star_and_of_joined_cliques():
    assert (_components([(1234, v) for v in range(3000) if v != 1234], 3000) == 0).all()
    assert _components([(v, 2999) for v in range(5, 2999)], 3000).tolist() == [0, 1, 2, 3, 4] + [5] * 2995
    left, right = range(10, 60), range(500, 540)
    cliques = [(a, b) for a in left for b in left if a < b] + [(a, b) for a in right for b in right if a > b]
    apart = _components(cliques, 600)
    assert apart[10] == 10 and apart[500] == 451 and (apart[10:60] == 10).all() and (apart[500:540] == 451).all()
    joined = _components(cliques + [(539, 59)], 600)
    assert (joined[500:540] == 10).all() and joined[499] == 450 and joined[540] == 451


def test_components_of_a_random_graph():
    rng = np.random.default_rng(9)
    n = 5000
    for m in (2000, 4000, 20000):
        links = rng.integers(0, n, (m, 2)).tolist()          # repeats and loops among them
        label = _components(links, n)
        assert label.max() + 1 == np.unique(label).size


def test_components_leave_out_reads_without_kmers():
    nk = [3, 0, 5, 1, 0, 2, 7]
    assert _components([(0, 2), (3, 5)], 7, nk).tolist() == [0, -1, 0, 1, -1, 1, 2]
    assert _components([(0, 1), (1, 2), (5, 6)], 7, nk).tolist() == [0, -1, 1, 2, -1, 3, 3]      # a link of such a read is ignored
    assert _components([], 3, [0, 0, 0]).tolist() == [-1, -1, -1]


def test_components_refuse_a_link_outside_the_vertices():
    from sarlacc_amd._lib import SarlaccError
    with pytest.raises(SarlaccError, match="link 2: an end outside"):
        _components([(0, 1), (2, 5), (1, 2)], 5)


# ---- end to end ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", S.SEEDS)
def test_sequence_groups_on_mock_reads(seed):
    """12 transcripts x 10 reads of 600 bases, shuffled, half of them reverse-complemented."""
    from sarlacc_amd import calls, generics
    seqs, transcript = S.mock_set(seed)
    want = S.expected(seqs)
    assert S.one_group_per_transcript(want["group"], transcript)
    dev = _device_reads(seqs)
    got = generics.sequenceGroups(dev)
    S.same(got, want, "DeviceReads")
    S.same(generics.sequenceGroups(generics.Reads([s.decode() for s in seqs])), want, "Reads")
    S.same(generics.sequenceGroups(dev), got, "second run")
    for kwargs in (dict(min_shared=2), dict(k=16, buckets=128, window=3, min_shared=4), dict(canonical=False), dict(min_shared=64)):
        S.same(generics.sequenceGroups(dev, **kwargs), S.expected(seqs, **kwargs), str(kwargs))
    rng = np.random.default_rng(seed)
    umis = ["".join("ACGT"[c] for c in rng.integers(0, 4, 12)) for _ in range(12)]
    off, members = calls.umi_group_flat([umis[t] for t in transcript], 1, None, 1, *got["groups"])
    assert off.size - 1 == 12 and sorted(members.tolist()) == list(range(1, 121))


def test_sequence_groups_with_reads_that_have_no_kmer():
    from sarlacc_amd import generics
    rng = np.random.default_rng(5)
    base = S.random_bases(rng, 300)
    seqs = [b"ACGT", base, b"N" * 50, base[:150] + S.random_bases(rng, 150), b"", S.random_bases(rng, 300), base]
    got = generics.sequenceGroups(generics.Reads([s.decode() for s in seqs]))
    S.same(got, S.expected(seqs), "mixed")
    assert got["group"].tolist() == [-1, 0, -1, 0, -1, 1, 0] and got["n.kmers"].tolist()[:5:2] == [0, 0, 0]
    assert got["groups"][0].tolist() == [0, 3, 4] and got["groups"][1].tolist() == [2, 4, 7, 6]
