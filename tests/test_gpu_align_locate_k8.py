"""GPU parity of the locator at eight columns per lane (align.hip: k_align's ROWF 4; option align_locate_shape).

For adaptors of 25 to 32 columns the framed locator runs sixteen alignments per wavefront, four lanes of eight columns
each, four alignments interleaved per DPP row; the window kernel keeps eight alignments of eight lanes.  The locator
computes the same integers cell for cell, so nothing downstream may change: every case is compared bit for bit with the
CPU oracle, with the locator in the window kernel's shape (align_locate_shape = -1) and with the snapshot path
(align_locate = -1), on resident ASCII reads and on the 2-bit packed format, and the two locator shapes must agree on
{I_max, lo, hi} of every read (sarlacc_align_locate_records) and with them on the oversize list's length, the redo count
and the window class histogram.  The counter "align_locate_cols" tells which shape ran.

Adaptors of 25 to 28 columns run the steady state's blocks on odd steps and those of 29 to 32 on even steps (k_align's
LOC_ODD), so the cases about the schedule run at 27 and at 30 columns.

The inputs are the smallest at which this shape can go wrong: every adaptor width from 24 to 33, wavefronts filled with
1 to 33 reads, reads shorter than the four-lane skew, sixteen different lengths in one
wavefront, lengths around the 64-position refills of each of the four staging passes, hits ending on the rows around the
ring's boundaries, two equal hits far apart, the forced oversize list, other penalties and another quality encoding.
"""
import numpy as np
import pytest

from tests.encodings import BY_NAME
from tests.test_gpu_align import rand_quals
from tests.test_gpu_align_locate import ADAPTOR, FILLED
from tests.test_gpu_align_locate_trim import _body, _dev_align, _planted, _same

pytestmark = pytest.mark.gpu

LONG = "ACGATCAGC" + "N" * 12 + "GTCAGTCAGTCATG"   # 35 columns; its prefixes are the adaptors of other widths
ODD = LONG[:27]                                     # a width whose blocks start on odd steps; FILLED[:27] is a copy of it
SCHEDULES = pytest.mark.parametrize("adaptor", [ADAPTOR, ODD], ids=["even30", "odd27"])
FORMATS = (False, True)


def _counts():
    from sarlacc_amd import _lib
    c = {k: _lib.stage_count("align_" + k) for k in ("redo", "stalls", "oversize", "locate_k", "locate_cols")}
    c["classes"] = [_lib.stage_count("align_window_class_%d" % x) for x in range(1, 32)]
    return c


def _run(enc, reads, quals, adaptor, go, ge, packed, **options):
    from sarlacc_amd import _lib
    got, _ = _dev_align(enc, reads, quals, adaptor, go, ge, (9,), (21,), packed, **options)
    c = _counts()
    c["records"] = _lib.align_locate_records(len(reads)) if c["locate_cols"] > 0 else None
    return got, c


def _check(oracle, oenc, enc, reads, quals, adaptor=ADAPTOR, go=5, ge=1, cols=8, **options):
    """The oracle against the default locator shape, the window kernel's shape and the snapshot path, per resident
    format; `cols`: the columns per lane the default rule must pick (0: the call takes no locator).  Returns the counters
    of the default shape (of the last format)."""
    want = oracle.adaptor_align(reads, quals, oenc, go, ge, adaptor, [9], [21])
    for packed in FORMATS:
        what = "packed" if packed else "ASCII"
        new, cn = _run(enc, reads, quals, adaptor, go, ge, packed, **options)
        _same(want, new, what)
        old, co = _run(enc, reads, quals, adaptor, go, ge, packed, align_locate_shape=-1, **options)
        _same(want, old, what + ", align_locate_shape = -1")
        snap, cs = _run(enc, reads, quals, adaptor, go, ge, packed, align_locate=-1)
        _same(want, snap, what + ", align_locate = -1")
        assert cs["redo"] == -1.0 and cs["locate_cols"] == 0
        assert cn["locate_cols"] == cols, "columns per lane of the locator (%s)" % what
        assert co["locate_cols"] == (4 if cols else 0)
        if cols:
            assert cn["stalls"] == 0 and co["stalls"] == 0
            differ = np.flatnonzero((cn["records"] != co["records"]).any(axis=1))
            assert differ.size == 0, "{I_max, lo, hi} differ between the locator shapes (%s): reads %s, %s against %s" % (
                what, differ[:8], cn["records"][differ[:8]].tolist(), co["records"][differ[:8]].tolist())
            for k in ("redo", "oversize", "locate_k", "classes"):
                assert cn[k] == co[k], "%s differs between the locator shapes (%s)" % (k, what)
    return cn


def _filled(adaptor, rng):
    return "".join(c if c != "N" else "ACGT"[int(rng.integers(0, 4))] for c in adaptor)


@pytest.mark.parametrize("R", [24, 25, 26, 27, 28, 29, 30, 31, 32, 33])
def test_adaptor_widths(oracle, oenc, enc, R):
    """Column R in each of the last lane's eight positions, one instantiation each (R = 25 leaves seven idle slots);
    24 columns keep four columns per lane, 33 take sixteen-lane alignments and no locator."""
    adaptor = LONG[:R]
    rng = np.random.default_rng(R)
    reads = []
    for k in range(36):
        copy = list(_filled(adaptor, rng))
        if k % 3 == 1:
            copy[int(rng.integers(0, R))] = "ACGT"[k % 4]      # a substitution
        if k % 3 == 2:
            del copy[int(rng.integers(1, R - 1))]                # a deletion
        reads.append(_body(rng, int(rng.integers(0, 90))) + "".join(copy) + _body(rng, int(rng.integers(0, 50))))
    reads += [_body(rng, n) for n in (1, 5, 33, 70)]             # and no copy at all
    # a wavefront of long reads: its steady state runs through the refill at step 64 (63 where the blocks are odd)
    reads += [_body(rng, 80 + 5 * k) + _filled(adaptor, rng) + _body(rng, 40) for k in range(16)]
    quals = rand_quals(reads, R, lo=35, hi=80)
    _check(oracle, oenc, enc, reads, quals, adaptor, cols=8 if 25 <= R <= 32 else 4 if R == 24 else 0)


@pytest.mark.parametrize("n", [1, 3, 4, 5, 15, 16, 17, 33])
def test_wavefront_filling(oracle, oenc, enc, n):
    """A lone leader, one DPP row partly and exactly filled, a row plus one, a wavefront less one, full, plus one, two
    wavefronts plus one."""
    rng = np.random.default_rng(100 + n)
    reads = [_planted(rng, 90 + 7 * k) for k in range(n)]
    _check(oracle, oenc, enc, reads, rand_quals(reads, n, lo=35, hi=80))


@SCHEDULES
def test_reads_shorter_than_the_pipeline(oracle, oenc, enc, adaptor):
    """Reads of 1 to 9 bases, mixed in one wavefront and sixteen of a length together: a four-lane skew has no steady
    state below its depth."""
    rng = np.random.default_rng(3)
    lengths = (1, 2, 3, 4, 5, 7, 8, 9)
    mixed = [_body(rng, n) for n in lengths]
    uniform = [_body(rng, n) for n in lengths for _ in range(16)]
    for reads in (mixed, uniform):
        _check(oracle, oenc, enc, reads, rand_quals(reads, len(reads), lo=35, hi=80), adaptor)


@SCHEDULES
def test_guarded_phases(oracle, oenc, enc, adaptor):
    """Sixteen reads of sixteen different lengths, 40 to 400 bases, in one wavefront: the entry, the steady state up to
    the shortest read and a long guarded tail all run, and the half of the wavefront without the shortest read takes
    the block rule on guarded rows.  The same from 100 to 400 bases: the steady state passes the refill at step 64 (63 on the odd schedule).
    Then a 1-base read beside a 300-base read."""
    rng = np.random.default_rng(4)
    for first, step in ((40, 24), (100, 20)):
        lengths = [first + step * k for k in range(16)]
        assert lengths[-1] == 400 and len(set(lengths)) == 16
        reads = [_planted(rng, n) for n in rng.permutation(lengths)]
        _check(oracle, oenc, enc, reads, rand_quals(reads, 4, lo=35, hi=80), adaptor)
    pair = [_body(rng, 1), _planted(rng, 300)]
    _check(oracle, oenc, enc, pair, rand_quals(pair, 5, lo=35, hi=80), adaptor)


STAGED = [64 * n + d for n in (1, 2) for d in (0, 1, 2, 3, 63)]


@SCHEDULES
def test_staging_lengths(oracle, oenc, enc, adaptor):
    """Lengths of 64 n + {0, 1, 2, 3, 63}: last refills of one to three positions and a full one, sixteen of a length in a
    wavefront (the steady state runs to the reads' end, through the refills at steps 64 and 128, or 63 and 127) and all lengths mixed;
    zero to three bases in front move every read to another bit offset of the packed bases."""
    rng = np.random.default_rng(5)
    uniform = [_planted(rng, n) for n in STAGED for _ in range(16)]
    _check(oracle, oenc, enc, uniform, rand_quals(uniform, 50, lo=35, hi=80), adaptor)
    mixed = [_planted(rng, n) for n in STAGED + STAGED[:6]]
    for front in range(4):
        reads = ([_body(rng, front)] if front else []) + mixed
        _check(oracle, oenc, enc, reads, rand_quals(reads, 51 + front, lo=35, hi=80), adaptor)


def test_other_characters_in_every_staging_pass(oracle, oenc, enc):
    """A character that is not ACGT in the first and in the last position of the reads of the 4th, 8th, 12th and 16th
    alignment of a wavefront, one per staging pass."""
    rng = np.random.default_rng(6)
    reads = [_planted(rng, 120 + k) for k in range(16)]
    for k, ch in ((3, "N"), (7, "R"), (11, "a"), (15, "-")):
        reads[k] = ch + reads[k][1:-1] + ch
    _check(oracle, oenc, enc, reads, rand_quals(reads, 6, lo=35, hi=80))


@SCHEDULES
def test_hit_rows_at_ring_boundaries(oracle, oenc, enc, adaptor):
    """A copy whose last row is 63, 64, 65, 127, 128, 129 (both residues mod 2, either side of the ring's halves)."""
    rng = np.random.default_rng(7)
    R = len(adaptor)
    reads = [_body(rng, last - R) + FILLED[:R] + _body(rng, 25) for last in (63, 64, 65, 127, 128, 129)]
    quals = rand_quals(reads, 7, lo=50, hi=80)
    c = _check(oracle, oenc, enc, reads, quals, adaptor)
    assert c["oversize"] == 0


def test_two_equal_hits_far_apart(oracle, oenc, enc):
    """Two copies with the same qualities 100 rows apart in a 300-base read: lo and hi are far apart and the read is
    oversize under both shapes."""
    rng = np.random.default_rng(8)
    reads = [_body(rng, 60) + FILLED + _body(rng, 70) + FILLED + _body(rng, 110)]
    assert len(reads[0]) == 300
    q = rand_quals(reads, 8, lo=45, hi=75)[0]
    quals = [q[:160] + q[60:90] + q[190:]]
    c = _check(oracle, oenc, enc, reads, quals)
    assert c["oversize"] == 1


def test_forced_oversize(oracle, oenc, enc):
    """align_locate = 1: every read through the oversize list."""
    rng = np.random.default_rng(9)
    reads = [_planted(rng, 60 + 9 * k) for k in range(21)]
    c = _check(oracle, oenc, enc, reads, rand_quals(reads, 9, lo=35, hi=80), align_locate=1)
    assert c["redo"] == len(reads)


@pytest.mark.parametrize("go,ge", [(5, 1), (0, 1), (2.5, 0.5)])
def test_penalties(oracle, oenc, enc, go, ge):
    rng = np.random.default_rng(10)
    reads = [_planted(rng, 50 + 11 * k) for k in range(20)]
    _check(oracle, oenc, enc, reads, rand_quals(reads, 10, lo=35, hi=80), go=go, ge=ge)


def test_second_encoding(oracle):
    """Phred+64 qualities: another offset and another table."""
    table = BY_NAME["illumina"]
    rng = np.random.default_rng(11)
    reads = [_planted(rng, 70 + 13 * k) for k in range(18)]
    quals = rand_quals(reads, 11, table=table)
    _check(oracle, table.oenc, table.enc, reads, quals)


def test_plain_locator_keeps_four_columns(oracle, oenc, enc):
    """An integer extension of 16 384: no scale of 2^8 or more holds its frame, the call runs the un-framed locator,
    which exists at four columns per lane only."""
    rng = np.random.default_rng(12)
    reads = [_planted(rng, 80 + 10 * k) for k in range(18)]
    c = _check(oracle, oenc, enc, reads, rand_quals(reads, 12, lo=35, hi=80), go=0, ge=16384, cols=4)
    assert c["locate_k"] < 0


@pytest.mark.parametrize("packed", FORMATS)
def test_bad_quality_message(enc, packed):
    """A quality below the offset in the first and in the last position of a read of each staging pass: the same message
    under both shapes and on the snapshot path; with two bad reads the first is reported."""
    from sarlacc_amd import SarlaccError
    rng = np.random.default_rng(13)
    reads = [_planted(rng, 100 + k) for k in range(20)]
    good = rand_quals(reads, 13, lo=35, hi=80)
    broken = ADAPTOR[:15] + "X" + ADAPTOR[16:]

    def message(quals, adaptor, **options):
        with pytest.raises(SarlaccError) as err:
            _dev_align(enc, reads, quals, adaptor, 5, 1, (9,), (21,), packed, **options)
        return str(err.value)

    for k in (3, 7, 11, 15, 19):
        for pos in (0, len(reads[k]) - 1):
            quals = list(good)
            quals[k] = quals[k][:pos] + " " + quals[k][pos + 1:]
            for adaptor in (ADAPTOR, broken):
                new = message(quals, adaptor)
                assert new == message(quals, adaptor, align_locate_shape=-1) == message(quals, adaptor, align_locate=-1)
                if adaptor == ADAPTOR:
                    assert "quality cannot be lower than smallest encoded value" in new
        quals[k - 2] = " " + quals[k - 2][1:]
        assert message(quals, broken) == message(quals, broken, align_locate_shape=-1)
