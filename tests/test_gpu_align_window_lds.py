"""GPU parity and counters of the LDS code ring of adaptor_align's window kernel (align.hip: WIN_LDS_WAVES, tile_word).

The MODE 4 window keeps the code words of its last blocks in a per-wave LDS ring besides the global tile; a walk reads a
block from the ring while it is one of the ring's, else from the tile.  Every case is compared with the CPU oracle bit
for bit, and output for output across the ring sizes (align_window_lds = 0: the default ring; -1: the tile alone, the
path before the ring; 2 and 3: a ring of that many blocks, which wraps many times and sends nearly every walk to the
tile) and the snapshot path (align_locate = -1).  Batches are at most 300 reads of at most 2 400 bases.
"""
import numpy as np
import pytest

from tests.encodings import BY_NAME
from tests.test_gpu_align import compare_adaptor, rand_quals
from tests.test_gpu_align_locate import ADAPTOR, FILLED, _families
from tests.test_gpu_align_window_classes import _align, _histogram, _same, _strong_hits

pytestmark = pytest.mark.gpu

RINGS = (-1, 2, 3)


def _counters():
    from sarlacc_amd import _lib
    keys = ("redo", "stalls", "oversize", "window_steps", "walk_global", "walk_left_ring")
    return {k: _lib.stage_count("align_" + k) for k in keys}


def _body(rng, n):
    return "".join(np.array(list("ACGT"))[rng.integers(0, 4, n)])


def _all_paths(oracle, oenc, enc, reads, quals, adaptor=ADAPTOR, go=5, ge=1, ss=(9,), se=(21,)):
    """The oracle against the default ring, then every other ring size and the snapshot path against the default's
    outputs.  Returns the outputs and, per align_window_lds value, the counters and the class histogram."""
    assert len(reads) <= 300 and max(len(r) for r in reads) <= 2400
    ss, se = list(ss), list(se)
    want = compare_adaptor(oracle, oenc, enc, reads, quals, adaptor, go, ge, ss, se)
    seen = {0: (_counters(), _histogram())}
    for ring in RINGS:
        got, _ = _align(enc, reads, quals, adaptor, go, ge, ss, se, align_window_lds=ring)
        seen[ring] = (_counters(), _histogram())
        _same(want, got, "align_window_lds = %d" % ring)
    snap, _ = _align(enc, reads, quals, adaptor, go, ge, ss, se, align_locate=-1)
    _same(want, snap, "align_locate = -1")
    print("LDS ring: %s" % {ring: c for ring, (c, _) in seen.items()})
    return want, seen


def _ring_counters(seen, locator=True, above=False, one_window=False):
    """What holds for every batch: the same windows with and without the ring, nothing stalled, and, where any window
    ran, a ring of two or three blocks sends more code reads to the tile than the default ring does (`above`: every
    walk of the batch starts above the default ring already and reads the tile alone, so nothing can grow).

    align_window_steps: a work item runs the steps of the tallest of its eight windows, and which reads of a class share
    an item is decided by the order of k_loc_order's atomics, which differs from call to call of one and the same
    library (seen on the GPU: 526 and 528 steps for one batch under one ring size).  The counter is therefore compared
    exactly where the grouping cannot matter (`one_window`: every read has the same window; or a single work item) and
    otherwise within the 8 steps of a class per work item; the class histogram, which fixes every read's own window, is
    always compared exactly."""
    c0, h0 = seen[0]
    if not locator:
        assert c0["redo"] == -1.0 and c0["walk_global"] == -1.0
        return
    assert c0["redo"] >= 0, "the call did not take the locator path"
    off, hoff = seen[-1]
    for k in ("redo", "stalls", "oversize"):
        assert c0[k] == off[k], k
    assert h0 == hoff
    assert c0["stalls"] == 0
    items = (sum(h0.values()) + 7) // 8
    exact = one_window or items <= 1
    for ring in RINGS:
        c, h = seen[ring]
        assert h == h0 and c["stalls"] == 0
        if exact:
            assert c["window_steps"] == c0["window_steps"], "align_window_lds = %d" % ring
        else:
            assert abs(c["window_steps"] - c0["window_steps"]) < 8 * items, "align_window_lds = %d" % ring
    assert off["walk_global"] == -1.0 and off["walk_left_ring"] == -1.0
    assert c0["walk_global"] >= c0["walk_left_ring"] >= 0
    for ring in (2, 3):
        c, _ = seen[ring]
        if c0["window_steps"] > 0 and not above:
            assert c["walk_global"] > c0["walk_global"], "a ring of %d blocks" % ring
        assert c["walk_global"] >= c0["walk_global"] and c["walk_left_ring"] >= c0["walk_left_ring"]
    assert seen[2][0]["walk_global"] >= seen[3][0]["walk_global"]


def _tops(seed):
    """windows that start at the true row 0 or just below it, hits that end with the read, and reads about as long as
    the adaptor"""
    rng = np.random.default_rng(seed)
    reads = []
    for at in (0, 1, 7, 8, 9, 70):
        for tail in (0, 3, 200):
            reads.append(_body(rng, at) + FILLED + _body(rng, tail))
    for n in (40, 333, 1999):
        reads.append(_body(rng, n) + FILLED)   # the copy ends at the read's last base
    for n in range(30, 61, 3):
        reads.append(_body(rng, n))
        reads.append((_body(rng, n - 30) + FILLED)[:n])
        reads.append((FILLED + _body(rng, n - 30))[:n])
    return reads


def _cut(reads):
    return [r[:2400] for r in reads]


def test_window_tops(oracle, oenc, enc):
    reads = _tops(1) + _cut(_families(31))
    for lo, hi in ((40, 75), (33, 126)):
        quals = rand_quals(reads, lo + hi, lo=lo, hi=hi)
        _, seen = _all_paths(oracle, oenc, enc, reads, quals)
        _ring_counters(seen)


def _indels(seed):
    """deletions of 1 - 5 adaptor columns and insertions of 1 - 5 read bases at every third column: horizontal and
    vertical chains at every place of the path, so some are measured across a ring boundary"""
    rng = np.random.default_rng(seed)
    reads = []
    for col in range(0, 30, 3):
        for n in range(1, 6):
            head, tail = _body(rng, int(rng.integers(0, 90))), _body(rng, int(rng.integers(0, 60)))
            reads.append(head + FILLED[:col] + FILLED[col + n:] + tail)
            reads.append(head + FILLED[:col] + _body(rng, n) + FILLED[col:] + tail)
    return reads


def _tall(seed, ins):
    """`ins` read bases inserted inside the hit, at three places of the adaptor and three of the read"""
    rng = np.random.default_rng(seed)
    reads = []
    for col in (4, 15, 26):
        for at in (0, 150, 900):
            reads.append(_body(rng, at) + FILLED[:col] + _body(rng, ins) + FILLED[col:] + _body(rng, 120))
    return reads


def test_indel_chains_across_ring_boundaries(oracle, oenc, enc):
    reads = _indels(2)
    assert len(reads) == 100
    for seed, lo, hi in ((3, 40, 75), (4, 33, 126), (5, 70, 70)):
        quals = rand_quals(reads, seed, lo=lo, hi=hi)
        _, seen = _all_paths(oracle, oenc, enc, reads, quals)
        _ring_counters(seen)


@pytest.mark.parametrize("ins", [20, 40, 80])
def test_paths_taller_than_the_ring(oracle, oenc, enc, ins):
    """the walk crosses from the ring into the global tile inside a vertical chain"""
    reads = _tall(6 + ins, ins)
    quals = ["I" * len(r) for r in reads]   # even qualities: the path takes the insertion as one vertical chain
    _, seen = _all_paths(oracle, oenc, enc, reads, quals)
    _ring_counters(seen)
    c0 = seen[0][0]
    if ins >= 40:
        assert c0["walk_global"] > 0 and c0["walk_left_ring"] > 0, "a %d-base insertion stays in the default ring" % ins
    quals = rand_quals(reads, ins, lo=40, hi=75)
    _, seen = _all_paths(oracle, oenc, enc, reads, quals)
    _ring_counters(seen)


def test_clean_hits_stay_in_the_ring(oracle, oenc, enc):
    reads = _strong_hits(7, 64, at=200)
    quals = ["I" * len(r) for r in reads]
    _, seen = _all_paths(oracle, oenc, enc, reads, quals)
    _ring_counters(seen, one_window=True)
    c0, h0 = seen[0]
    assert len(h0) == 1, "one window height"
    assert c0["walk_global"] == 0 and c0["walk_left_ring"] == 0
    assert seen[2][0]["walk_left_ring"] == len(reads)


def test_counters_with_and_without_the_ring(oracle, oenc, enc):
    """align_window_steps, align_redo, align_stalls and the class histogram, align_window_lds = 0 against -1, on batches
    whose steps do not depend on the window order: one work item of mixed windows, and 65 reads with one window"""
    mixed = [_cut(_families(35))[k] for k in (0, 3, 8, 13, 15, 30, 40)]
    uniform = _strong_hits(9, 65, at=333)
    for reads, same in ((mixed, False), (uniform, True)):
        quals = ["I" * len(r) for r in reads] if same else rand_quals(reads, 77, lo=40, hi=75)
        _, seen = _all_paths(oracle, oenc, enc, reads, quals)
        (c0, h0), (off, hoff) = seen[0], seen[-1]
        assert c0["window_steps"] > 0
        for k in ("window_steps", "redo", "stalls"):
            assert c0[k] == off[k], k
        assert h0 == hoff and (len(h0) == 1) == same
        _ring_counters(seen, one_window=same)


@pytest.mark.parametrize("gap", [15, 25, 40])
def test_landing_row_above_the_ring(oracle, oenc, enc, gap):
    """Two equal-scoring copies `gap` bases apart (the second given the qualities of the first): the window holds both
    and the walk starts at the first, well above the window's last row."""
    rng = np.random.default_rng(40 + gap)
    reads = []
    for at in (0, 5, 100, 700):
        b = _body(rng, at + 260 + gap)
        reads.append(b[:at] + FILLED + b[at + 30:at + 30 + gap] + FILLED + b[at + 60 + gap:])
    # (good qualities: a weak hit would raise the window's head room and, at 40 bases, make the read oversize)
    for lo, hi in ((65, 75), (73, 73)):
        quals = rand_quals(reads, gap + lo, lo=lo, hi=hi)
        for k, at in enumerate((0, 5, 100, 700)):
            q, second = quals[k], at + 30 + gap
            assert reads[k][at:at + 30] == FILLED == reads[k][second:second + 30]
            quals[k] = q[:second] + q[at:at + 30] + q[second + 30:]
        _, seen = _all_paths(oracle, oenc, enc, reads, quals)
        _ring_counters(seen, above=True)
        assert seen[0][0]["oversize"] == 0 and seen[0][0]["redo"] == 0
        if gap >= 25:
            assert seen[0][0]["walk_left_ring"] > 0


A32 = "ACGATCAGCTTGCAAGTCGTCAGTCAGACGTTG"[:32]


def _planted(seed, adaptor, n=48):
    """clean and damaged copies of `adaptor` (IUPAC-free) in random bodies, hit-free reads and reads shorter than it"""
    rng = np.random.default_rng(seed)
    R = len(adaptor)
    reads = []
    for k in range(n):
        b = _body(rng, int(rng.integers(0, 700)))
        e = int(rng.integers(0, len(b) + 1))
        copy = adaptor
        if k % 3 == 1 and R > 4:   # a deletion and a substitution
            p = int(rng.integers(1, R - 2))
            copy = adaptor[:p] + adaptor[p + 1:R - 1] + "ACGT"[int(rng.integers(0, 4))]
        if k % 3 == 2:             # an insertion
            p = int(rng.integers(1, R))
            copy = adaptor[:p] + _body(rng, int(rng.integers(1, 12))) + adaptor[p:]
        reads.append(b[:e] + copy + b[e:])
    reads += [_body(rng, int(rng.integers(0, 900))) for _ in range(8)]
    reads += ["", adaptor, adaptor[:R // 2], adaptor[1:], "N" * 40, adaptor + adaptor]
    return reads


@pytest.mark.parametrize("R", [32, 30, 17, 16, 9, 5])
def test_adaptor_shapes(oracle, oenc, enc, R):
    """four columns per lane and two steps per code word (22 - 32 columns), two columns and four steps (up to 16); 17
    columns take sixteen-lane alignments and the snapshot path, which has no ring"""
    adaptor = A32[:R]
    reads = _planted(50 + R, adaptor)
    for seed, lo, hi in ((1, 40, 75), (2, 33, 126)):
        quals = rand_quals(reads, seed + R, lo=lo, hi=hi)
        _, seen = _all_paths(oracle, oenc, enc, reads, quals, adaptor, 5, 1, [0, R // 3], [R, R - 1])
        _ring_counters(seen, locator=R != 17)


@pytest.mark.parametrize("adaptor,go,ge", [(ADAPTOR, 5, 1), (ADAPTOR, 2, 0.5), (ADAPTOR, 0, 1), ("ACGTACGTAC", 2, 0.5),
                                           ("ACGTNNNNACGTRYACGTVHACGT", 5, 1), (ADAPTOR, 3, 1)])
def test_penalty_sets(oracle, oenc, enc, adaptor, go, ge):
    reads = _cut(_families(33))[:44] + _tall(8, 40)[:3] + _indels(9)[::7]
    quals = rand_quals(reads, 11, lo=35, hi=80)
    _, seen = _all_paths(oracle, oenc, enc, reads, quals, adaptor, go, ge, [0], [len(adaptor)])
    _ring_counters(seen)


def test_other_phred_encoding(oracle):
    table = BY_NAME["illumina"]   # Phred+64
    reads = _tops(12)[::2] + _tall(13, 40)[:4] + _indels(14)[::5] + _cut(_families(34))[:30]
    quals = rand_quals(reads, 15, table=table)
    _, seen = _all_paths(oracle, table.oenc, table.enc, reads, quals)
    _ring_counters(seen)
