"""The inputs of tests/align_wide_cases.py on the CPU oracle alone: the paths really run where the groups' names say, so
that tests/test_gpu_align_wide.py asks the banded kernel for both outcomes at every edge it aims at."""
import numpy as np
import pytest

from tests import align_wide_cases as W


def _check_strings(case, want):
    for gr, gq, read in zip(want[2], want[3], case.reads):
        assert W.spells(gr, gq, case.ref, read)


def test_stored_set_restated():
    """The band in numbers: at L = R the steps of wavefront w are [512 w - band - 2, 512 (w + 1) + band + 64] plus its first
    63; lane 0 is tight above the diagonal, lane 63 below it."""
    L = R = 2048
    for band in W.BANDS:
        assert W.band_lo(1, band, L, R) == 512 - band - 2 and W.band_hi(1, band, L, R) == 1024 + band + 64
        for d, want in ((band + 2, True), (band + 3, False)):
            assert bool(W.stored(513 - d, 513, band, L, R)) == want       # lane 0 of wavefront 1, d rows above the diagonal
            assert bool(W.stored(1024 + d, 1024, band, L, R)) == want     # lane 63 of wavefront 1, d rows below it
            assert bool(W.stored(520 - d, 520, band, L, R))               # the lane's last column: further from the edge
        assert bool(W.stored(63, 513, band, L, R)) and not bool(W.stored(64, 513, band, L, R))   # steps 62 | 63 of wavefront 1, far above the diagonal
        assert bool(W.stored(1, 1016, band, L, R)) and not bool(W.stored(2, 1016, band, L, R))   # the same two steps in its lane 62
        assert not bool(W.stored(1, 1017, band, L, R))                                           # lane 63 enters at step 63
    assert bool(W.stored(2000, 1, 0, L, R)) and bool(W.stored(2000, 1, -1, L, R))   # no band: every cell
    # L != R: the diagonal's slope in both bounds, the upper one rounded up
    assert W.band_lo(2, 8, 700, 1100) == 1024 * 700 // 1100 - 10 and W.band_hi(2, 8, 700, 1100) == -(-1536 * 700 // 1100) + 72
    assert not W.leaves("ACGT", "ACGT", 8, 4, 4) and not W.leaves("", "", 8, 0, 0)


@pytest.mark.parametrize("R", W.SWEEP_R)
def test_edge_sweep_on_the_oracle(oracle, R):
    """d <= band + 2 stays, d >= band + 3 leaves: both sides of the diagonal, all three widths, both bands."""
    for band in W.BANDS:
        case = W.edge_sweep(R, band)
        want = W.expected(oracle, case)
        _check_strings(case, want)
        out = W.leaving(oracle, case, band)
        for (side, d), left in zip(case.tags, out):
            assert left == (not W.sweep_stays(d, band)), (R, band, side, d)
        assert sum(out) == 4 and len(out) == 10
        # the other band on the same reads: everything stays in 96 rows at d <= 12, everything leaves 8 rows at d >= 96
        other = W.BANDS[1 - W.BANDS.index(band)]
        assert set(W.leaving(oracle, case, other)) == {other < band}


@pytest.mark.parametrize("R", W.EXCURSION_R)
def test_local_excursions_on_the_oracle(oracle, R):
    for band in W.BANDS:
        case = W.local_excursions(R, band)
        want = W.expected(oracle, case)
        _check_strings(case, want)
        out = dict(zip(case.tags, W.leaving(oracle, case, band)))
        print(R, band, sorted(k for k, v in out.items() if v))
        assert set(out.values()) == {False, True}
        left_at_boundary = {(side, d) for (place, side, d), v in out.items() if place == "boundary" and v}
        assert any(not out[("interior", side, d)] for side, d in left_at_boundary)
        # the excursions really are excursions: d rows off the diagonal half way along
        for (place, side, d), gr, gq in zip(case.tags, want[2], want[3]):
            row, c = W.path_cells(gr, gq)
            mid = W.EXCURSION_X[place] + W.EXCURSION_SPAN // 2
            assert int(row[np.searchsorted(c, mid)]) - mid == (-d if side == "above" else d), (R, band, place, side, d)


@pytest.mark.parametrize("R", W.SKEW_R)
def test_skewed_on_the_oracle(oracle, R):
    case = W.skewed(R)
    want = W.expected(oracle, case)
    _check_strings(case, want)
    assert len({len(r) for r in case.reads} | {R}) == len(case.reads) + 1   # every length its own, none R
    for band in W.BANDS:
        out = dict(zip(case.tags, W.leaving(oracle, case, band)))
        print(R, band, out)
        assert set(out.values()) == {False, True}, (R, band)
        assert out["second_half"] and not out["thinned"] and not out["thickened"]


def test_queue_and_reuse_generators():
    """(their outcomes are read off the oracle in the GPU tests) lengths, sizes and plants as the kernels' constants ask"""
    for R in W.QUEUE_R:
        case = W.queue_edges(R)
        assert len(case.ref) == R and [len(r) for r in case.reads] == list(W.QUEUE_LENGTHS)
        assert all(len(q) == len(r) for q, r in zip(case.quals, case.reads))
    assert {(R - 1) % 8 for R in W.QUEUE_R} >= {0, 7} and {(R - 1) // 8 % 64 for R in W.QUEUE_R} >= {0, 63}
    for (R, per_cu), cus in ((W.REUSE_ONE_STRIP, 5), (W.REUSE_TWO_STRIPS, 4)):
        case, grid = W.reuse(R, per_cu, cus)
        assert grid == cus * per_cu and len(case.reads) == 2 * grid + 40 and max(len(r) for r in case.reads) == 60
        for k, names in W.REUSE_PLANTS.items():
            assert [case.tags[k + j * grid] for j in range(3)] == list(names)
            assert [len(case.reads[k + j * grid]) for j in range(3)] == [{"leaver": 50, "stayer": 6, "long": 60, "empty": 0}[x] for x in names]
