"""sarlacc_dev_links_verify on the device (csrc/links_verify.hip, sarlacc_amd/sketch.py verify_links), compared exactly
with tests/links_verify_cases.py, the plain-numpy restatement of DESIGN §4.19 rule 6a that
tests/test_links_verify_host.py pins.  Everything is integers: no tolerance.

The kernel keeps the band's 2 w + 1 rows in 1, 2, 4, 7 or 8 words of 32 bits and fetches bases eight at a time, forward
for the first strand and from the end of the second read for the other, so the bandwidths tried sit either side of
every word count, the lengths around the grabs, and every batch is uploaded at its exact size: its last read ends at the
buffer's last byte and its first starts at byte 0."""
import ctypes as C

import numpy as np
import pytest

from tests import links_verify_cases as V
from tests import sketch_cases as S

pytestmark = pytest.mark.gpu

BANDWIDTHS = [0, 1, 15, 16, 31, 32, 63, 64, 100, 127]


def _upload(seqs):
    """(device bases, device offsets) of a batch whose buffer is exactly as long as the reads."""
    from sarlacc_amd.resident import DevBuffer
    chars = np.frombuffer(b"".join(seqs), np.uint8)
    off = np.zeros(len(seqs) + 1, np.int64)
    np.cumsum([len(s) for s in seqs], out=off[1:])
    assert chars.size
    return DevBuffer.from_numpy(chars), DevBuffer.from_numpy(off)


def _call(seqs, links, ppm, w, both=True, with_strand=True, with_kept=True, n=None):
    """The C call itself: (rc, kept as left by the call, n_kept, dist, strand); the outputs are filled with 77 before."""
    from sarlacc_amd import _lib
    from sarlacc_amd.resident import DevBuffer
    links = np.asarray(links, np.uint64)
    room = max(links.size, 1)
    d_seq, d_off = _upload(seqs)
    d_links = DevBuffer.from_numpy(links if links.size else np.zeros(1, np.uint64))
    d_dist, d_strand, d_kept = (DevBuffer.from_numpy(np.full(room, 77, t)) for t in (np.int32, np.uint8, np.uint64))
    nkept = C.c_int64(-5)
    rc = _lib.lib().sarlacc_dev_links_verify(d_seq, d_off, len(seqs) if n is None else n, d_links, links.size, w, ppm, 1 if both else 0, d_dist,
                                             d_strand if with_strand else None, d_kept if with_kept else None, C.byref(nkept), None)
    return (rc, d_kept.to_numpy(np.uint64, room).copy(), nkept.value, d_dist.to_numpy(np.int32, room).copy(),
            d_strand.to_numpy(np.uint8, room).copy())


def _check(seqs, pairs, ppm, w, both=True, what=""):
    """Every output against the restatement; returns (dist, strand, kept) of the device."""
    links = V.links_between(pairs)
    rc, kept, nkept, dist, strand = _call(seqs, links, ppm, w, both)
    from sarlacc_amd._lib import check
    check(rc)
    want_kept, want_dist, want_strand = V.verify(seqs, links, ppm, w, both)
    m = links.size
    wrong = np.flatnonzero((dist[:m] != want_dist) | (strand[:m] != want_strand))
    assert wrong.size == 0, (what, "w", w, "ppm", ppm, "links", wrong[:8].tolist(), [pairs[i] for i in wrong[:8]],
                             dist[wrong[:8]].tolist(), want_dist[wrong[:8]].tolist(), strand[wrong[:8]].tolist(), want_strand[wrong[:8]].tolist())
    assert nkept == want_kept.size and np.array_equal(kept[:nkept], want_kept), (what, nkept, want_kept.size)
    assert (kept[nkept:] == 77).all()
    return dist[:m], strand[:m], kept[:nkept]


def _ppm_for(t, longest):
    """The smallest max_diff_ppm whose bound for a pair with this longer read is t."""
    ppm = -(-t * V.PPM // longest)
    assert 0 <= ppm < V.PPM and V.threshold(ppm, longest, 1) == t
    return ppm


# ---- the band's words ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", BANDWIDTHS)
def test_band_word_edges(w):
    """Pairs of 40 .. 300 bases whose lengths differ by 0, 1, w - 1, w and w + 1, the longer read on either side, a noisy
    copy (some pass, some do not) or its reverse complement, at bounds below and above w."""
    rng = np.random.default_rng(500 + w)
    seqs, pairs = [], []
    for gap in sorted({g for g in (0, 1, w - 1, w, w + 1) if g >= 0}):
        for length in (40 + gap, 171, 300):
            if length - gap < 40:
                continue
            for nsub in (0, 3, length // 12, length // 4):
                long_read = S.random_bases(rng, length)
                short_read = V.noisy(rng, long_read, nsub=min(nsub, length - gap - 8), ndel=gap)
                first, second = (long_read, short_read) if len(pairs) % 2 else (short_read, long_read)
                if len(pairs) % 3 == 0:
                    second = V.rc(second)
                pairs.append((len(seqs), len(seqs) + 1))
                seqs += [first, second]
    passed = 0
    for identity in (0.5, 0.9):
        dist, strand, _ = _check(seqs, pairs, V.max_diff_ppm(identity), w, True, "band words")
        passed += int((dist >= 0).sum())
        assert (dist < 0).any()
        _check(seqs, pairs, V.max_diff_ppm(identity), w, False, "band words, one strand")
    assert passed >= 10 and (strand == 1).any()


# ---- lengths ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [0, 1, 16, 100])
def test_length_edges(w):
    """Reads of 0 and 1 bases: two empty reads are equal (t = 0, D = 0); an empty read and any other differ by more than any
    bound; identity 1.0 passes equal reads only."""
    seqs = [b"", b"", b"A", b"A", b"C", b"T", b"N", b"N", b"", b"AC", b"AC", b"GT", b"AG", b"ACGTTGCA" * 3, b"ACGTTGCA" * 3, b"G"]
    pairs = [(0, 1), (0, 2), (2, 3), (2, 4), (2, 5), (6, 7), (1, 8), (7, 8), (9, 10), (9, 11), (9, 12), (13, 14), (8, 13), (2, 9), (5, 15)]
    for ppm in (0, 200000, 500000, 999999):
        dist, strand, kept = _check(seqs, pairs, ppm, w, True, "short reads")
        assert dist[0] == 0 and strand[0] == 0 and dist[1] == -1              # both empty; one empty
        assert dist[2] == 0 and dist[3] == -1 and (dist[4], strand[4]) == (0, 1) and dist[5] == -1      # A A; A C; A T = rc; N N
        assert dist[6] == 0 and dist[7] == -1 and dist[8] == 0 and (dist[9], strand[9]) == (0, 1)
        assert dist[11] == 0 and dist[12] == -1
        assert dist[10] == (1 if ppm >= 500000 else -1)                        # AC AG: t = 2 ppm div 10^6
        _check(seqs, pairs, ppm, w, False, "short reads, one strand")


# ---- the threshold ---------------------------------------------------------------------------------------------------------
def _at_and_above(seqs, pair, w, what):
    """The pair passes with D = t and fails with D = t + 1, the bound moved by max_diff_ppm."""
    a, b = seqs[pair[0]], seqs[pair[1]]
    d = V.banded(a, b, w)
    assert d is not None and d >= 1
    longest = max(len(a), len(b))
    at, _, _ = _check(seqs, [pair], _ppm_for(d, longest), w, False, what + ", D = t")
    above, _, _ = _check(seqs, [pair], _ppm_for(d - 1, longest), w, False, what + ", D = t + 1")
    assert at.tolist() == [d] and above.tolist() == [-1]
    return d


@pytest.mark.parametrize("w", [5, 16, 40, 100])
def test_threshold_edges(w):
    rng = np.random.default_rng(700 + w)
    a = S.random_bases(rng, 200)
    # the last difference sits in the last column and the last row: until there the distance is one short
    b = bytearray(V.noisy(rng, a, nsub=9))
    b[-1] = ord("ACGT"[("ACGT".index(chr(b[-1])) + 1) % 4])
    assert _at_and_above([a, bytes(b)], (0, 1), w, "last column") == 10
    # the first read is longer by four bases at its end: the last rows alone carry the four
    assert _at_and_above([a + b"ACGT", V.noisy(rng, a, nsub=6)], (0, 1), w, "last rows") == 10
    # ... and the second read longer: the last columns
    assert _at_and_above([V.noisy(rng, a, nsub=6), a + b"ACGT"], (0, 1), w, "last columns") == 10


@pytest.mark.parametrize("w", [1, 3, 15, 16])
def test_the_banded_value_decides_where_the_bound_lies_above_the_band(w):
    """w + 2 bases deleted in front and as many inserted behind: the true distance is 2 w + 4, which no path inside the
    band reaches; the banded value is far larger, and it -- not the true one -- is what passes at D = t and fails at t + 1."""
    rng = np.random.default_rng(800 + w)
    a = S.random_bases(rng, 120)
    b = a[w + 2:] + S.random_bases(rng, w + 2)
    true = V.levenshtein(a, b)
    assert w < true <= 2 * w + 4
    d = _at_and_above([a, b], (0, 1), w, "shifted")
    assert d > true + 10 and V.threshold(_ppm_for(d - 1, 120), 120, 120) >= true


# ---- bytes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [16, 100])
def test_bytes_that_are_no_base(w):
    """N, lower case, bytes >= 128 and 0 at the first, last, 31st / 32nd and 63rd / 64th base of either read or of both (the
    same byte in both is still a difference), as the reads stand and with the second one reverse-complemented."""
    rng = np.random.default_rng(9)
    seqs, pairs = [], []
    for bad in (ord("N"), ord("a"), ord("t"), 0x80, 0xc7, 0xff, 0):
        for place in (0, -1, 30, 31, 62, 63):
            for where in ("first", "second", "both"):
                for flip in (False, True):
                    a = bytearray(S.random_bases(rng, 131))
                    b = bytearray(a)
                    if where != "second":
                        a[place] = bad
                    if where != "first":
                        b[place] = bad
                    pairs.append((len(seqs), len(seqs) + 1))
                    seqs += [bytes(a), V.rc(bytes(b)) if flip else bytes(b)]
    dist, strand, kept = _check(seqs, pairs, V.max_diff_ppm(0.9), w, True, "no base")
    assert (dist == 1).all() and strand.tolist() == [0, 1] * (len(pairs) // 2) and kept.size == len(pairs)
    dist, _, _ = _check(seqs, pairs, 0, w, True, "no base, identity 1")
    assert (dist == -1).all()


# ---- strands ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [16, 100])
def test_strands(w):
    rng = np.random.default_rng(11)
    a = S.random_bases(rng, 250)
    near = V.noisy(rng, a, nsub=12, ndel=3, nins=3)
    q = b"ACGGTCATGC" + V.rc(b"ACGGTCATGC")                      # its own reverse complement
    a1 = b"ACTGTCATGCGCATGACCGT"                                  # q with base 2 substituted; rc(a1) is q with base 17 substituted
    half = S.random_bases(rng, 100)
    palindrome = half + V.rc(half)
    seqs = [a, V.rc(near), near, a1, V.rc(a1), q, q, palindrome, V.noisy(rng, palindrome, nsub=5), S.random_bases(rng, 250)]
    pairs = [(0, 1), (0, 2), (3, 4), (5, 6), (3, 5), (7, 8), (0, 9)]
    dist, strand, _ = _check(seqs, pairs, V.max_diff_ppm(0.8), w, True, "both strands")
    assert dist[0] == dist[1] > 0 and strand.tolist() == [1, 0, 0, 0, 0, 0, 0]
    assert dist[2:5].tolist() == [2, 0, 1] and 0 < dist[5] <= 5 and dist[6] == -1      # forward though the reverse is closer
    one, _, _ = _check(seqs, pairs, V.max_diff_ppm(0.8), w, False, "one strand")
    assert one[0] == -1 and np.array_equal(one[1:], dist[1:])


def test_second_strand_counter_and_python_wrapper():
    from sarlacc_amd import _lib, sketch
    from sarlacc_amd.resident import DevBuffer
    rng = np.random.default_rng(12)
    a, other = S.random_bases(rng, 150), S.random_bases(rng, 150)
    seqs = [a, V.noisy(rng, a, nsub=5), V.rc(V.noisy(rng, a, nsub=5)), other, a[:60]]
    links = V.links_between([(0, 1), (0, 2), (0, 3), (1, 2), (0, 4)])
    d_seq, d_off = _upload(seqs)
    want_kept, want_dist, want_strand = V.verify(seqs, links, 200000, 100)
    d_kept, nkept, d_dist, d_strand = sketch.verify_links(d_seq, d_off, len(seqs), DevBuffer.from_numpy(links), links.size, 0.8)
    assert nkept == 3 and np.array_equal(d_kept.to_numpy(np.uint64, nkept), want_kept)
    assert np.array_equal(d_dist.to_numpy(np.int32, 5), want_dist) and np.array_equal(d_strand.to_numpy(np.uint8, 5), want_strand)
    # 0-2, 0-3 and 1-2 fail forward and are tried again; 0-4 is decided by its lengths alone
    assert _lib.stage_count("sketch_verify_pairs") == 5 and _lib.stage_count("sketch_verify_second_strand") == 3
    assert _lib.stage_ms("sketch_verify") > 0
    sketch.verify_links(d_seq, d_off, len(seqs), DevBuffer.from_numpy(links), links.size, 0.8, both_strands=False)
    assert _lib.stage_count("sketch_verify_pairs") == 5 and _lib.stage_count("sketch_verify_second_strand") == 0


# ---- counts ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def families():
    """Four families of three noisy copies of 90 bases, a family of 10 bases and one of 5 003: links inside a family pass."""
    rng = np.random.default_rng(13)
    seqs = []
    for length in (90, 90, 90, 90, 10, 5003):
        truth = S.random_bases(rng, length)
        seqs += [truth, V.noisy(rng, truth, nsub=length // 20), V.rc(V.noisy(rng, truth, nsub=length // 20, ndel=min(1, length // 50)))]
    return seqs


@pytest.mark.parametrize("n_links", [1, 63, 64, 65, 4097])
def test_link_counts_and_the_order_of_the_kept_links(families, n_links):
    """Passing and failing links interleaved, repeats among them, reads of 10 bases beside reads of 5 003 in one wavefront."""
    rng = np.random.default_rng(n_links)
    short = [(a, b) for a in range(15) for b in range(a + 1, 15)]
    pairs = [short[i] for i in rng.integers(0, len(short), n_links)]
    if n_links >= 63:
        for at, pair in ((3, (15, 16)), (4, (12, 13)), (5, (15, 17)), (6, (13, 14)), (40, (16, 17)), (41, (3, 15)), (n_links - 1, (12, 14))):
            pairs[at] = pair
    dist, strand, kept = _check(families, pairs, V.max_diff_ppm(0.8), 100, True, "%d links" % n_links)
    inside = np.array([a // 3 == b // 3 for a, b in pairs])
    assert np.array_equal(dist >= 0, inside) and np.array_equal(kept, V.links_between(pairs)[inside])
    if n_links >= 63:
        assert 0 < inside.sum() < n_links and (strand == 1).any() and dist[3] > 100


def test_no_links_launch_nothing():
    rc, kept, nkept, dist, strand = _call([b"ACGT", b"ACGA"], np.zeros(0, np.uint64), 200000, 100)
    assert rc == 0 and nkept == 0 and kept.tolist() == [77] and dist.tolist() == [77] and strand.tolist() == [77]


def test_outputs_that_are_not_asked_for(families):
    pairs = [(0, 1), (0, 3), (1, 2), (4, 9), (15, 17)]
    links = V.links_between(pairs)
    want_kept, want_dist, _ = V.verify(families, links, 200000, 100)
    for with_strand, with_kept in ((False, True), (True, False), (False, False)):
        rc, kept, nkept, dist, strand = _call(families, links, 200000, 100, True, with_strand, with_kept)
        assert rc == 0 and nkept == want_kept.size == 3 and np.array_equal(dist, want_dist)
        assert (strand == 77).all() if not with_strand else strand.tolist() == [0, 0, 1, 0, 1]
        assert (kept == 77).all() if not with_kept else np.array_equal(kept[:nkept], want_kept)


# ---- long reads ------------------------------------------------------------------------------------------------------------
def test_a_pair_of_70001_bases():
    """Positions beyond 16 bits; 400 substitutions and 60 + 60 indels spread along the read keep the path inside w = 100."""
    rng = np.random.default_rng(14)
    a = S.random_bases(rng, 70001)
    b = V.noisy(rng, a, nsub=400, ndel=60, nins=60)
    seqs = [a, b, V.rc(b)]
    dist, strand, _ = _check(seqs, [(0, 1), (0, 2)], V.max_diff_ppm(0.99), 100, True, "70 001 bases")
    assert 400 < dist[0] == dist[1] <= 520 and strand.tolist() == [0, 1]


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_refusals():
    from sarlacc_amd import _lib
    seqs = [b"ACGTACGTAC", b"ACGTACGTAC", b"ACGTACGTAT"]
    good = [(0, 1), (0, 2), (1, 2)]

    def refused(links, ppm, w, n=None):
        rc, kept, nkept, _, _ = _call(seqs, V.links_between(links), ppm, w, n=n)
        assert rc != 0 and (kept == 77).all() and nkept in (0, -5)      # nothing was kept
        return _lib.lib().sarlacc_last_error().decode()
    assert "link 2: its ends are not 0 <= a < b < n" in refused([(0, 1), (2, 1), (1, 2)], 200000, 100)      # a > b
    assert "link 1: its ends are not 0 <= a < b < n" in refused([(1, 1), (0, 2)], 200000, 100)              # a = b
    assert "link 3: its ends are not 0 <= a < b < n" in refused([(0, 1), (0, 2), (1, 3)], 200000, 100)      # b = n
    assert "link 2: its ends are not 0 <= a < b < n" in refused([(0, 1), (0, 2)], 200000, 100, n=2)
    assert "'bandwidth' lies in 0 .. 127" in refused(good, 200000, 128)
    assert "'bandwidth' lies in 0 .. 127" in refused(good, 200000, -1)
    assert "'max_diff_ppm' lies in 0 .. 999999" in refused(good, 10 ** 6, 100)
    assert "'max_diff_ppm' lies in 0 .. 999999" in refused(good, -1, 100)
    dist, _, kept = _check(seqs, good, 200000, 100)                        # and the library goes on
    assert dist.tolist() == [0, 1, 1] and kept.size == 3


def test_offsets_that_do_not_ascend_are_refused():
    from sarlacc_amd import _lib
    from sarlacc_amd.resident import DevBuffer
    chars = np.frombuffer(S.random_bases(np.random.default_rng(1), 100), np.uint8)
    links = DevBuffer.from_numpy(V.links_between([(0, 1), (1, 2)]))
    for off, message in (([0, 50, 40, 100], "read 2: its offsets"), ([0, 50, 120, 100], "read 2: its offsets"), ([-1, 50, 60, 100], "read 1: its offsets")):
        out = DevBuffer(64)
        rc = _lib.lib().sarlacc_dev_links_verify(DevBuffer.from_numpy(chars), DevBuffer.from_numpy(np.array(off, np.int64)), 3, links, 2, 100, 200000, 1,
                                                 out, None, None, None, None)
        assert rc != 0 and message in _lib.lib().sarlacc_last_error().decode()
