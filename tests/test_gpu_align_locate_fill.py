"""GPU parity of the locator fill (align.hip MODE 5 / 6) across the shapes at which its loop changes path.

Every case compares adaptor_align on the default path (locator in the extension-free frame, its un-framed form where the
frame's range rule refuses) with the CPU oracle bit for bit: score, start, end, section start and section width, and no
walk may stall.  The same reads then go through the redo list (align_locate = 1) and the snapshot kernel alone (-1); all
three must agree.  The oracle runs once per case.
"""
import numpy as np
import pytest

from tests.test_gpu_align import bits

pytestmark = pytest.mark.gpu

ADAPTOR = "ACGATCAGC" + "N" * 12 + "GTCAGTCAG"
# block of 2 steps, 8-step entry, 64-row refill, ring wrap at 128, 8-entry mirror
LENGTHS = [1, 3, 7, 8, 9, 31, 63, 64, 65, 127, 128, 129, 136, 300]
NUC = np.array(list("ACGT"))


def _reference(n):
    """n columns: the bench adaptor (12 N columns) cut or extended with plain and ambiguous columns."""
    return (ADAPTOR + "RY")[:n] if n <= 32 else None


def _filled(ref, rng):
    return "".join(c if c in "ACGT" else str(NUC[rng.integers(0, 4)]) for c in ref)


def _reads(lengths, ref, seed):
    """One read per length: random bases with a (sometimes edited, sometimes cut) copy of the reference planted, a few
    non-ACGT bases, and qualities over the whole encoding with its lowest and highest character present."""
    rng = np.random.default_rng(seed)
    reads, quals = [], []
    for n, L in enumerate(lengths):
        hit = list(_filled(ref, rng))
        if n % 3 == 1 and len(hit) > 4:
            del hit[int(rng.integers(0, len(hit)))]
            at = int(rng.integers(0, len(hit)))
            hit[at:at] = ["ACGT"[n % 4]] * int(rng.integers(1, 5))
        b = list(NUC[rng.integers(0, 4, L)])
        if n % 4 != 3:
            at = int(rng.integers(0, max(1, L - len(hit) + 1)))
            b[at:at + len(hit)] = hit
        b = b[:L]
        for p in rng.integers(0, L, L // 40 + (n % 2)):
            b[int(p)] = "N"
        q = rng.integers(33, 127, L).astype(np.uint8)
        q[int(rng.integers(0, L))] = 33
        q[int(rng.integers(0, L))] = 126
        reads.append("".join(b))
        quals.append(q.tobytes().decode())
    return reads, quals


def _counts():
    from sarlacc_amd import _lib
    return _lib.stage_count("align_redo"), _lib.stage_count("align_stalls"), _lib.stage_count("align_locate_k")


def _same(want, got, what):
    assert np.array_equal(bits(want[0]), bits(got[0])), "scores differ (%s)" % what
    assert np.array_equal(want[1], got[1]) and np.array_equal(want[2], got[2]), "starts / ends differ (%s)" % what
    for a, b in zip(list(want[3]) + list(want[4]), list(got[3]) + list(got[4])):
        assert np.array_equal(a, b), "sections differ (%s)" % what


def check_paths(oracle, oenc, enc, reads, quals, ref, go, ge, path):
    """path: 'framed' / 'plain' (the locator, in or out of the frame), 'snapshot', or None (whichever the shape takes)."""
    from sarlacc_amd import calls
    ss, se = ([min(9, len(ref) - 1)], [min(21, len(ref))]) if len(ref) > 2 else ([0], [len(ref)])
    want = oracle.adaptor_align(reads, quals, oenc, go, ge, ref, ss, se)
    seen_k = None
    try:
        for opt in (0, 1, -1):
            calls.set_option("align_locate", opt)
            got = calls.adaptor_align(reads, quals, enc, go, ge, ref, ss, se)
            _same(want, got, "align_locate = %d" % opt)
            redo, stalls, k = _counts()
            if opt == -1 or path == "snapshot":
                assert (redo, stalls) == (-1.0, -1.0)
                continue
            if path is None and redo < 0:
                continue
            assert redo >= 0 and stalls == 0
            assert (k > 0) == (path != "plain") and k != 0
            if opt == 1:
                assert redo == len(reads)
            seen_k = k
    finally:
        calls.set_option("align_locate", 0)
    return seen_k


@pytest.mark.parametrize("nreads", [1, 7, 8, 9, 17])
def test_read_lengths_and_batch_sizes(oracle, oenc, enc, nreads):
    """Different lengths inside one wavefront (the guarded and the steady loop hand over to each other at different
    steps), partly filled wavefronts and the last work item."""
    order = np.random.default_rng(nreads).permutation(len(LENGTHS))
    lengths = [LENGTHS[i] for i in order] + [300, 64, 9]
    if nreads == 17:
        lengths = LENGTHS + [300, 64, 9]
    reads, quals = _reads(lengths[:nreads], ADAPTOR, 100 + nreads)
    check_paths(oracle, oenc, enc, reads, quals, ADAPTOR, 5, 1, "framed")
    # eight equally long reads: the whole fill but its entry and exit runs in the steady loop
    if nreads == 8:
        reads, quals = _reads([300] * 8, ADAPTOR, 7)
        check_paths(oracle, oenc, enc, reads, quals, ADAPTOR, 5, 1, "framed")


@pytest.mark.parametrize("ncol", [5, 6, 16, 17, 29, 30, 31, 32])
def test_reference_widths(oracle, oenc, enc, ncol):
    """Column R at every position inside its lane (K = 2: 5, 6 and 16 columns; K = 4: 17 and 29 to 32), idle columns
    past it, and the bench adaptor.  17 columns take another shape by default and the locator when asked to."""
    from sarlacc_amd import calls
    ref = _reference(ncol)
    reads, quals = _reads(LENGTHS + [300, 64, 9], ref, ncol)
    check_paths(oracle, oenc, enc, reads, quals, ref, 5, 1, None if ncol == 17 else "framed")
    if ncol == 17:
        calls.set_option("align_k", 4)
        calls.set_option("align_interleave", 1)
        try:
            check_paths(oracle, oenc, enc, reads, quals, ref, 5, 1, "framed")
        finally:
            calls.set_option("align_k", 0)
            calls.set_option("align_interleave", 0)


@pytest.mark.parametrize("go,ge,path", [(5, 1, "framed"), (0, 1, "framed"), (2.5, 0.5, "framed"), (4, 0.25, "framed"),
                                        (0.3, 0.7, "snapshot")])
@pytest.mark.parametrize("ncol", [30, 6])
def test_penalties(oracle, oenc, enc, go, ge, path, ncol):
    ref = _reference(ncol)
    reads, quals = _reads(LENGTHS + [300, 64, 9], ref, 50 + ncol)
    check_paths(oracle, oenc, enc, reads, quals, ref, go, ge, path)


@pytest.fixture(scope="module")
def long_reads():
    return _reads([20_000, 70_000, 40, 129, 8, 300, 2000], ADAPTOR, 77)


@pytest.mark.parametrize("pick", [(0,), (1,), (0, 2, 3, 4), (2, 1, 3, 4, 5, 6, 0)])
def test_long_reads_lower_the_scale(oracle, oenc, enc, long_reads, pick):
    """The frame grows with the row: the longest read of the call sets k (the model test states the rule)."""
    reads, quals = [long_reads[0][i] for i in pick], [long_reads[1][i] for i in pick]
    k = check_paths(oracle, oenc, enc, reads, quals, ADAPTOR, 5, 1, "framed")
    k_short = check_paths(oracle, oenc, enc, [long_reads[0][5]], [long_reads[1][5]], ADAPTOR, 5, 1, "framed")
    assert 8 <= k < k_short
    if 1 in pick:
        k20 = check_paths(oracle, oenc, enc, long_reads[0][:1], long_reads[1][:1], ADAPTOR, 5, 1, "framed")
        assert k < k20


def test_frame_out_of_range_takes_the_plain_locator(oracle, oenc, enc, long_reads):
    """No k >= 8 holds 70 000 rows of an extension of 64: the call runs the un-framed locator."""
    reads, quals = long_reads[0][1:5], long_reads[1][1:5]
    check_paths(oracle, oenc, enc, reads, quals, ADAPTOR, 64, 64, "plain")
    # and the same reads in the frame at the benchmark's penalties, against the un-framed locator asked for by option
    from sarlacc_amd import calls
    framed = calls.adaptor_align(reads, quals, enc, 5, 1, ADAPTOR, [9], [21])
    assert _counts()[2] > 0
    calls.set_option("align_locate", 2)
    try:
        plain = calls.adaptor_align(reads, quals, enc, 5, 1, ADAPTOR, [9], [21])
        assert _counts()[2] < 0 and _counts()[1] == 0
    finally:
        calls.set_option("align_locate", 0)
    _same(framed, plain, "framed against un-framed")
