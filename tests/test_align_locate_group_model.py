"""CPU model of the locator's candidate rows under any grouping of column R's row tests (align.hip: the comment above LOC_NEG).

The framed fill (tests/test_align_locate_frame_model.py) decides the candidate rows [lo, hi] from column R once per two-row
block in its steady state and once per row elsewhere.  The rule generalises to groups of G blocks: s = column R before the
group's first row, x = the largest X of its rows, b = column R after its last row, all taken into the frame of the first
row; lo is the first row of the last group with b - D > s, hi the last row of the last group with x + D >= b.  G = 1 is
the kernel's rule.  G = 4 was built and measured: it saved vector instructions that the locator
does not wait for and made every window up to 7 rows taller at each end, so the kernel keeps G = 1; the model keeps the
general rule because it is the cheapest statement of why ANY mixture of groups and single rows is safe, which the kernel
relies on where a work item's steady state ends with its shortest read.  Checked here: for G = 1, 2, 4 and every place a
group can begin relative to a hit, [lo, hi] holds every row whose fp64 X equals the score (the fp64 fill used for that is
itself checked against the oracle's score bits and landing row); G = 1 gives the lo and hi of the two-row model; and the
window plan of the strong-hit reads of tests/test_gpu_align_locate_trim.py, segmented as the kernel segments a batch,
fits the code tile, which is what lets that test demand that none of them is oversize.
"""
import numpy as np
import pytest

from tests import test_align_locate_frame_model as frame
from tests import test_align_locate_model as model

ADAPTOR, FILLED = model.ADAPTOR, model.FILLED
LOC_NEG, LOC_NEG_FRAMED = model.LOC_NEG, frame.LOC_NEG_FRAMED
UNR, W, NG = 2, 8, 8   # steps per block at four columns per lane; lanes and alignments per wavefront


def snap_win(R):
    return (64 + R + R // 4 + 4 + W + 7) // 8 * 8


def column_r(w, lens, plan, R, GO, GE):
    """Column R of the framed int32 fill, row by row and each row in its own frame: X, the column before the row (V) and
    after it (best), [B, Lmax + 1]; I_max out of the frame; and X of the fp64 fill in the kernel's formulation with the
    fp64 score."""
    B, Lmax = len(lens), int(lens.max(initial=0))
    k, GEi = plan["k"], plan["GE"]
    GOO = plan["GO"] - GEi
    fin = np.isfinite(w)
    wi = np.where(fin, np.rint(np.ldexp(np.where(fin, w, 0.0), k)) + 2 * GEi, LOC_NEG_FRAMED).astype(np.int64)
    S = [np.full(B, plan["rz"][c] + GEi * c, np.int64) for c in range(R + 1)]
    UJ = [np.full(B, LOC_NEG, np.int64) for _ in range(R + 1)]
    Sf = [np.full(B, 0.0 if c == 0 else -(GO + GE * (c - 1))) for c in range(R + 1)]
    UJf = [np.full(B, -np.inf) for _ in range(R + 1)]
    Xi, Vi, Bi = (np.zeros((B, Lmax + 1), np.int64) for _ in range(3))
    Xf = np.full((B, Lmax + 1), -np.inf)
    for i in range(1, Lmax + 1):
        act = i <= lens
        left, lj, diag = np.full(B, GEi * i, np.int64), np.full(B, LOC_NEG, np.int64), np.full(B, GEi * (i - 1), np.int64)
        leftf, ljf, diagf = np.zeros(B), np.full(B, -np.inf), np.zeros(B)
        for c in range(1, R + 1):
            last = c == R
            H = np.maximum(lj, left - GOO)
            lj = H
            V = np.maximum(UJ[c], S[c] - (-GEi if last else GOO))
            M = diag + wi[:, i - 1, c - 1]
            diag = S[c]
            X = np.maximum(M, H)
            best = np.maximum(X, V)
            UJ[c] = np.where(act, V, UJ[c])
            S[c] = np.where(act, best, S[c])
            left = best
            Hf = np.maximum(ljf - GE, leftf - GO)
            ljf = Hf
            Vf = np.maximum(UJf[c] - (0.0 if last else GE), Sf[c] - (0.0 if last else GO))
            Mf = diagf + w[:, i - 1, c - 1]
            diagf = Sf[c]
            Xff = np.maximum(Mf, Hf)
            bestf = np.maximum(Xff, Vf)
            UJf[c] = np.where(act, Vf, UJf[c])
            Sf[c] = np.where(act, bestf, Sf[c])
            leftf = bestf
            if last:
                Xi[:, i], Vi[:, i], Bi[:, i] = X, V, best
                Xf[:, i] = np.where(act, Xff, -np.inf)
    imax = S[R] - GEi * (lens + R)
    return Xi, Vi, Bi, imax, Xf, Sf[R]


def grouped(Xi, Vi, Bi, lens, plan, G, first, stop):
    """[lo, hi] by the grouped rule: whole groups of G blocks from row `first` (per read) while they end before row `stop`,
    the test per row everywhere else."""
    rows, D, GEi = G * UNR, plan["D"], plan["GE"]
    D_lo = D + GEi * (rows - 1)
    B = len(lens)
    first, stop = np.broadcast_to(first, (B,)), np.broadcast_to(stop, (B,))
    end = first + np.maximum(stop - first, 0) // rows * rows
    lo, hi = np.zeros(B, np.int64), np.zeros(B, np.int64)
    s, x = np.zeros(B, np.int64), np.zeros(B, np.int64)
    for i in range(1, Xi.shape[1]):
        act = i <= lens
        ingroup = act & (i >= first) & (i < end)
        assert not (ingroup & (end > lens + 1)).any(), "a group leaves its read"
        r = (i - first) % rows
        s = np.where(ingroup & (r == 0), Vi[:, i], s)
        x = np.where(ingroup & (r == 0), Xi[:, i], np.where(ingroup, np.maximum(x, Xi[:, i] - r * GEi), x))
        last = ingroup & (r == rows - 1)
        bd = Bi[:, i] - D_lo
        lo = np.where(last & (bd > s), i - rows + 1, lo)
        hi = np.where(last & (x >= bd), i, hi)
        single = act & ~ingroup
        lo = np.where(single & (Bi[:, i] - D > Vi[:, i]), i, lo)
        hi = np.where(single & (Xi[:, i] + D >= Bi[:, i]), i, hi)
    return lo, hi


def kernel_segments(lens, R, G):
    """first and stop of grouped() as the kernel segments a batch: work items of eight consecutive reads; the steady
    state runs from the first step that is a multiple of a group and at which every lane is inside its read, in whole
    groups, until the item's shortest read ends; column R's lane is at row t - jlast at step t."""
    rows, jlast = G * UNR, (R - 1) // 4
    first, stop = np.zeros(len(lens), np.int64), np.zeros(len(lens), np.int64)
    for a in range(0, len(lens), NG):
        item = lens[a:a + NG]
        nsteps = (int(item.max()) + W + UNR - 1) // UNR * UNR
        t_a = min((W + UNR - 1) // UNR * UNR, nsteps)
        t_b = min(max((int(item.min()) + 1) // UNR * UNR, t_a), nsteps)
        t_sa = min((t_a + rows - 1) // rows * rows, t_b)
        t_sb = t_sa + (t_b - t_sa) // rows * rows
        first[a:a + NG], stop[a:a + NG] = t_sa - jlast, t_sb - jlast
    return first, stop


def window_need(plan, imax, lo, hi, R, GE):
    """align.hip window_plan: the steps of the read's window"""
    f_low = imax * plan["unit"] - plan["slack"]
    over = np.floor((plan["top"] - f_low) / GE) + 1.0
    wc = R + np.where(over > 0, np.minimum(over, 1e6), 0).astype(np.int64)
    r0 = lo - wc
    ts = np.where(r0 < 8, 0, r0 & ~7)
    return hi + W + 1 - ts


def _body(rng, n):
    return "".join(np.array(list("ACGT"))[rng.integers(0, 4, n)])


def strong_hit_reads(n, seed=5):
    """Reads with one clean copy of the adaptor whose last base is the read's base 30, 31, ... (a landing row of every
    residue mod 8, the first ones with a window that starts at row 0), each with 0, 3 or 40 bases behind the copy (0: the hit
    lands on the read's last row)."""
    rng = np.random.default_rng(seed)
    return [_body(rng, k % 61) + FILLED + _body(rng, (0, 3, 40)[(k // 8) % 3]) for k in range(n)]


def strong_hit_quals(reads, seed=6):
    return model._quals(reads, seed, 45, 75)


STRONG_BATCHES = (1, 7, 8, 9, 257)


def _setup(oracle, oenc, reads, quals, ref, gapopen, gapext):
    R, GO, GE = len(ref), gapopen + gapext, gapext
    w, colvals, entries = model.costs(oracle, oenc, ref, reads, quals)
    lens = np.array([len(r) for r in reads])
    plan = frame.plan_locate(colvals, entries, R, GO, GE, int(lens.max(initial=0)))
    assert plan is not None and plan["framed"]
    return w, lens, plan, column_r(w, lens, plan, R, GO, GE)


def _doubles(seed):
    """two equal-scoring hits 4, 8, 12 and 20 rows apart, and hits on every row residue"""
    rng = np.random.default_rng(seed)
    reads = [_body(rng, 20 + k) + FILLED + _body(rng, gap) + FILLED + _body(rng, 9) for k, gap in enumerate((4, 8, 12, 20))]
    reads += [_body(rng, at) + FILLED + _body(rng, tail) for at in range(0, 17) for tail in (0, 5)]
    return reads


@pytest.mark.parametrize("ref,gapopen,gapext", [(ADAPTOR, 5, 1), (ADAPTOR, 2, 0.5), ("ACGTNNNNACGTRYACGTVHAC", 5, 1)])
def test_groups_hold_every_row_with_the_score(oracle, oenc, ref, gapopen, gapext):
    R = len(ref)
    reads = _doubles(3) + model._families(17, 120)
    quals = model._quals(reads, 18, 38, 75)
    for k in range(4):   # the doubles: the second copy with the qualities of the first, so that both rows reach the score
        a, gap = 20 + k, (4, 8, 12, 20)[k]
        quals[k] = quals[k][:a + 30 + gap] + quals[k][a:a + 30] + quals[k][a + 60 + gap:]
    w, lens, plan, (Xi, Vi, Bi, imax, Xf, scoref) = _setup(oracle, oenc, reads, quals, ref, gapopen, gapext)
    # the fp64 fill is the oracle's: score bits and landing row
    want = oracle.adaptor_align(reads, quals, oenc, gapopen, gapext, ref, [], [])
    assert np.array_equal(scoref.view(np.int64), np.asarray(want[0], np.float64).view(np.int64))
    rows_at_score = []
    for b, L in enumerate(lens):
        _, dirs = oracle.align_one(ref, reads[b], quals[b], oenc, gapopen, gapext, True, want_dirs=True)
        row = int(L)
        while row > 0 and dirs[R, row] < 0:
            row += dirs[R, row]
        at = [i for i in range(1, L + 1) if Xf[b, i] == scoref[b]]
        if row > 0:
            assert at and at[0] == row   # the landing row is the first row that reaches the score
        rows_at_score.append(at)
    assert ref != ADAPTOR or all(len(rows_at_score[k]) == 2 for k in range(4)), "the doubles do not tie"
    # un-framed and framed fills agree on I_max, and G = 1 is the two-row model
    for block in (0, 1):
        ref_imax, ref_lo, ref_hi = frame.locate_framed(w, lens, plan, R, block)
        lo, hi = grouped(Xi, Vi, Bi, lens, plan, 1, 2 - block, lens + 1)
        assert np.array_equal(ref_imax, imax) and np.array_equal(ref_lo, lo) and np.array_equal(ref_hi, hi)
    for G in (1, 2, 4):
        rows = G * UNR
        segs = [(1 + p, lens + 1) for p in range(rows)]                  # every phase of the groups against the hits
        segs += [(1 + p, lens // 2) for p in range(rows)]                # ... with the steady state ending early
        segs.append(kernel_segments(lens, R, G))
        for first, stop in segs:
            lo, hi = grouped(Xi, Vi, Bi, lens, plan, G, first, np.minimum(stop, lens + 1))
            for b, at in enumerate(rows_at_score):
                assert all(lo[b] <= i <= hi[b] for i in at), (G, b, at, int(lo[b]), int(hi[b]))
            # the window only grows with the group: at most rows - 1 above and below the rows of the test per row
            lo1, hi1 = grouped(Xi, Vi, Bi, lens, plan, 1, lens + 1, lens + 1)
            assert np.all(hi <= hi1 + rows - 1) and np.all(lo >= lo1 - (rows - 1))


@pytest.mark.parametrize("n", STRONG_BATCHES)
def test_strong_hits_fit_the_code_tile(oracle, oenc, n):
    """The precondition of the GPU test's `align_oversize == 0`: every strong-hit read's window plan, from the rule per
    two-row block as the kernel segments the batch, needs no more steps than the tile has."""
    R = len(ADAPTOR)
    reads = strong_hit_reads(n)
    quals = strong_hit_quals(reads)
    for gapopen, gapext in ((5, 1), (2, 0.5)):
        w, lens, plan, (Xi, Vi, Bi, imax, Xf, scoref) = _setup(oracle, oenc, reads, quals, ADAPTOR, gapopen, gapext)
        for G in (1,):
            first, stop = kernel_segments(lens, R, G)
            lo, hi = grouped(Xi, Vi, Bi, lens, plan, G, first, stop)
            need = window_need(plan, imax, lo, hi, R, gapext)
            assert int(need.max()) <= snap_win(R), (G, int(need.max()))
            landing = np.array([int(np.argmax(Xf[b] == scoref[b])) for b in range(n)])
            assert np.all((lo <= landing) & (landing <= hi))
    # a landing row of every residue mod 8, windows that start at row 0 and below it, hits on the read's last row
    if n >= 257:
        assert {int(x) % 8 for x in landing} == set(range(8))
        assert (landing < 38).any() and (landing > 80).any() and (landing == lens).any()
