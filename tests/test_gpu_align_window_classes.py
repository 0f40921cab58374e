"""GPU parity and counters of adaptor_align's window classes (align.hip: LOC_NCLS, k_loc_order).

The locator files every read under the height of its fp64 window, the window kernel takes the reads tallest class first,
and the reads whose window exceeds the code tile go on a list the locator fills itself; the snapshot kernel aligns that
list on a second stream beside the windows.  Outputs are written by read index, so every case must equal the CPU oracle
bit for bit and the two A/B paths (align_window_classes = -1: index order, one redo list filled by the window kernel;
align_locate = -1: the snapshot path alone) output for output.
"""
import numpy as np
import pytest

from tests.test_gpu_align import bits, compare_adaptor, rand_quals
from tests.test_gpu_align_locate import ADAPTOR, FILLED, _families

pytestmark = pytest.mark.gpu


def _counters():
    from sarlacc_amd import _lib
    return {k: _lib.stage_count("align_" + k) for k in ("redo", "stalls", "oversize", "window_steps")}


def _histogram():
    """reads per window class of the last call, classes without a read left out"""
    from sarlacc_amd import _lib
    h = {c: int(_lib.stage_count("align_window_class_%d" % c)) for c in range(1, 32)}
    return {c: k for c, k in h.items() if k > 0}


def _align(enc, reads, quals, adaptor=ADAPTOR, go=5, ge=1, ss=(9,), se=(21,), **options):
    """outputs and counters of one call under the given options (restored afterwards)"""
    from sarlacc_amd import calls
    for name, value in options.items():
        calls.set_option(name, value)
    try:
        out = calls.adaptor_align(reads, quals, enc, go, ge, adaptor, list(ss), list(se))
        return out, _counters()
    finally:
        for name in options:
            calls.set_option(name, 0)


def _same(want, got, what):
    assert np.array_equal(bits(want[0]), bits(got[0])), "scores differ: " + what
    assert np.array_equal(want[1], got[1]) and np.array_equal(want[2], got[2]), "positions differ: " + what
    for a, b in zip(list(want[3]) + list(want[4]), list(got[3]) + list(got[4])):
        assert np.array_equal(a, b), "sections differ: " + what


def _body(rng, n):
    return "".join(np.array(list("ACGT"))[rng.integers(0, 4, n)])


def _strong_hits(seed, n, at=None):
    """reads with one clean copy of the adaptor; `at`: the same place in every read (one window height)"""
    rng = np.random.default_rng(seed)
    reads = []
    for _ in range(n):
        b = _body(rng, 600 if at is not None else int(rng.integers(100, 2400)))
        e = at if at is not None else int(rng.integers(0, len(b)))
        reads.append(b[:e] + FILLED + b[e:])
    return reads


# strong hits, hit-free reads, two identical copies 300 and 1 500 bases apart, 40- and 80-base insertions inside the hit,
# reads shorter than the adaptor, empty and all-N reads: _families holds every one of them (84 reads)
@pytest.fixture(scope="module")
def mixed():
    reads = _families(21)
    assert "" in reads and "N" * 2000 in reads and len(reads) <= 300
    return reads


DOUBLES = {5: 300, 6: 1500}   # _families: read -> bases between its two copies (the first at base 100)


def _mixed_quals(reads, seed, lo, hi):
    """random qualities; the second copy of the far-apart double hits gets the qualities of the first, so the two hits
    score the same, the candidate rows span both and the window is oversize"""
    quals = rand_quals(reads, seed, lo=lo, hi=hi)
    for k, gap in DOUBLES.items():
        q, second = quals[k], 130 + gap
        assert reads[k][100:130] == FILLED == reads[k][second:second + 30]
        quals[k] = q[:second] + q[100:130] + q[second + 30:]
    return quals


@pytest.mark.parametrize("lo,hi", [(33, 126), (40, 75)])
def test_mixed_batch_parity_and_counters(oracle, oenc, enc, mixed, lo, hi):
    quals = _mixed_quals(mixed, lo + hi, lo, hi)
    new = compare_adaptor(oracle, oenc, enc, mixed, quals, ADAPTOR, 5, 1, [9], [21])
    cn, hist = _counters(), _histogram()
    snap, cs = _align(enc, mixed, quals, align_locate=-1)
    _same(new, snap, "align_locate = -1")
    assert cs["redo"] == -1.0
    old, co = _align(enc, mixed, quals, align_window_classes=-1)
    _same(new, old, "align_window_classes = -1")
    print("classes on %s, off %s, histogram %s" % (cn, co, hist))
    assert cn["stalls"] == 0 and co["stalls"] == 0
    assert cn["oversize"] == cn["redo"] == co["redo"]
    assert cn["oversize"] >= len(DOUBLES), "the far-apart double hits are oversize"
    assert sum(hist.values()) == len(mixed) - cn["oversize"]
    assert co["oversize"] == 0
    assert 0 < cn["window_steps"] < co["window_steps"]


@pytest.mark.parametrize("n", [1, 7, 8, 9, 65])
def test_batch_sizes_one_class(oracle, oenc, enc, n):
    """partial work items, and a class of exactly 8 and of exactly 9 reads: the same hit in the same place gives every read
    the same window"""
    reads = _strong_hits(30 + n, n, at=200)
    quals = ["I" * len(r) for r in reads]
    new = compare_adaptor(oracle, oenc, enc, reads, quals, ADAPTOR, 5, 1, [9], [21])
    cn = _counters()
    hist = _histogram()
    assert list(hist.values()) == [n], hist
    assert cn["redo"] == 0 and cn["oversize"] == 0 and cn["stalls"] == 0
    # every item runs the class's steps, rounded to the 8-step store granule at most
    (cls,) = hist
    assert 8 * (cls - 1) * ((n + 7) // 8) < cn["window_steps"] <= 8 * cls * ((n + 7) // 8)
    old, _ = _align(enc, reads, quals, align_window_classes=-1)
    _same(new, old, "align_window_classes = -1")


@pytest.mark.parametrize("adaptor,go,ge", [("ACGTACGTAC", 2, 0.5), ("ACGTNNNNACGTRYACGTVHACGT", 5, 1), (ADAPTOR, 2, 0.5)])
def test_other_adaptors(oracle, oenc, enc, mixed, adaptor, go, ge):
    quals = _mixed_quals(mixed, 11, 35, 80)
    new = compare_adaptor(oracle, oenc, enc, mixed, quals, adaptor, go, ge, [0], [len(adaptor)])
    cn = _counters()
    assert cn["redo"] >= 0, "the call did not take the locator path"
    assert cn["stalls"] == 0 and cn["oversize"] == cn["redo"]
    old, co = _align(enc, mixed, quals, adaptor, go, ge, [0], [len(adaptor)], align_window_classes=-1)
    _same(new, old, "align_window_classes = -1")
    assert co["redo"] == cn["redo"] and cn["window_steps"] <= co["window_steps"]


def test_uniform_batch_runs_no_more_steps(enc):
    reads = _strong_hits(5, 64)
    quals = rand_quals(reads, 6, lo=40, hi=75)
    new, cn = _align(enc, reads, quals)
    old, co = _align(enc, reads, quals, align_window_classes=-1)
    _same(new, old, "align_window_classes = -1")
    assert cn["stalls"] == 0 and cn["redo"] == co["redo"]
    assert 0 < cn["window_steps"] <= co["window_steps"]


def test_forced_redo(oracle, oenc, enc, mixed):
    quals = _mixed_quals(mixed, 12, 35, 80)
    new, _ = _align(enc, mixed, quals)
    from sarlacc_amd import calls
    calls.set_option("align_locate", 1)
    try:
        forced = compare_adaptor(oracle, oenc, enc, mixed, quals, ADAPTOR, 5, 1, [9], [21])
        cf = _counters()
    finally:
        calls.set_option("align_locate", 0)
    _same(new, forced, "align_locate = 1")
    assert cf["redo"] == len(mixed) and cf["oversize"] == len(mixed) and cf["stalls"] == 0
    assert cf["window_steps"] == 0 and _histogram() == {}


def test_back_to_back_calls_and_streams(oracle, oenc, enc, mixed):
    """two calls on one stream, the second on other reads, and a call on a stream that is not the default one: the join
    of the side stream orders the lists and tiles the calls share"""
    torch = pytest.importorskip("torch")
    from sarlacc_amd import device as sdev
    from sarlacc_amd.strset import StringSet
    dev = torch.device("cuda", 0)
    batches = [mixed, _families(22)[::-1]]
    wants, bufs = [], []
    for k, reads in enumerate(batches):
        quals = _mixed_quals(reads, 40 + k, 35, 90) if k == 0 else rand_quals(reads, 40 + k, lo=35, hi=90)
        wants.append(oracle.adaptor_align(reads, quals, oenc, 5, 1, ADAPTOR, [9], [21]))
        s, q = StringSet.from_strings(reads), StringSet.from_strings(quals)
        bufs.append((torch.from_numpy(s.chars).to(dev), torch.from_numpy(q.chars).to(dev), torch.from_numpy(s.off).to(dev),
                     len(s), int(s.widths().max())))

    def launch(k, stream):
        d_seq, d_qual, d_off, n, max_len = bufs[k]
        out = [torch.zeros(n, dtype=torch.float64, device=dev)] + [torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(4)]
        sdev.dev_align(d_seq, d_qual, d_off, n, max_len, enc, 5, 1, ADAPTOR, True, [9], [21], *out, stream)
        return out

    def check(k, out):
        got = [t.cpu().numpy() for t in out]
        want = wants[k]
        assert np.array_equal(bits(got[0]), bits(want[0])), "scores differ"
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
        assert np.array_equal(got[3], want[3][0]) and np.array_equal(got[4], want[4][0])

    torch.cuda.synchronize()
    main = torch.cuda.current_stream().cuda_stream
    first, second = launch(0, main), launch(1, main)
    torch.cuda.synchronize()
    check(0, first)
    check(1, second)
    other = torch.cuda.Stream()
    with torch.cuda.stream(other):
        third = launch(0, other.cuda_stream)
    other.synchronize()
    check(0, third)
    assert _counters()["oversize"] >= 2


def test_first_bad_quality_read_is_still_reported(enc, mixed):
    """The locator stages every base of every read in index order and reports the first read with a quality below the
    encoding; the window kernel, which runs in class order, reports none.  With an adaptor character that is not IUPAC
    beyond column 1 the reference raises the quality error only where the bad read is the first read with a base at
    all, so the message tells whether the index that came back is exactly that read's."""
    from sarlacc_amd import SarlaccError, calls
    rng = np.random.default_rng(9)
    double = _body(rng, 700)
    double = double[:300] + FILLED + double[330:350] + FILLED + double[380:]   # two hits 20 rows apart: a tall window, not oversize
    k = 70
    reads = [""] * k + [double] + _strong_hits(8, 29)
    quals = rand_quals(reads, 10, lo=40, hi=75)
    _, c = _align(enc, reads, quals)
    hist = _histogram()
    assert c["oversize"] == 0 and len(hist) >= 2, hist
    bad = list(quals)
    bad[k] = bad[k][:340] + " " + bad[k][341:]
    bad[k + 20] = " " + bad[k + 20][1:]
    for options in ({}, {"align_window_classes": -1}):
        with pytest.raises(SarlaccError, match="quality cannot be lower than smallest encoded value"):
            _align(enc, reads, bad, **options)
        with pytest.raises(SarlaccError, match="quality cannot be lower than smallest encoded value"):
            _align(enc, reads, bad, ADAPTOR[:15] + "X" + ADAPTOR[16:], **options)
        assert _counters()["redo"] >= 0, "the call did not take the locator path"
        # the first bad read is no longer the first read with a base: the adaptor's error comes first
        later = list(quals)
        later[k + 20] = bad[k + 20]
        with pytest.raises(SarlaccError, match="unrecognized base in reference sequence"):
            _align(enc, reads, later, ADAPTOR[:15] + "X" + ADAPTOR[16:], **options)
