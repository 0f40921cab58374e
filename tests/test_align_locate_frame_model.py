"""CPU model of the locator fill in its extension-free frame (align.hip MODE 6, the comment above LOC_NEG).

The framed fill runs the int32 recurrence of tests/test_align_locate_model.py on I'(i, c) = I(i, c) + GE (i + c): both gap
extensions cost 0, an opening costs GO - GE, a diagonal move gains 2 GE (folded into the table), column 0 is GE i and
the free vertical step of column R gains GE.  Restated here in numpy: the host's rule for the scale 2^k (it now depends
on the longest read, because the frame grows by GE 2^k per row), the framed fill with its candidate rows [lo, hi] as the
kernel's blocks compute them, and the way I_max leaves the frame.  Checked: the framed fill returns the integers of the
un-framed fill at the same k, every value it forms stays inside the stated range for reads of up to 10^6 bases, an
"-inf" table entry never wins a cell, and windows placed from its results reproduce the oracle (the un-framed model's
own check, run on the framed plan and fill).
"""
import math

import numpy as np
import pytest

from tests import test_align_locate_model as model
from tests.encodings import TABLE_IDS, TABLES, draw_quals

LOC_NEG = model.LOC_NEG
LOC_NEG_FRAMED = -(1 << 30)
LOC_FRAME_KMIN = 8
ADAPTOR = model.ADAPTOR
_plan_unframed, _locate_unframed = model.plan_locate, model.locate   # (two tests swap the model's own for the frame's)


def plan_locate(colvals, entries, R, GO, GE, max_len, allow_frame=True):
    """align.hip plan_locate: the un-framed plan (the model's), then the frame's k rule.  rz, GO and the table stay in
    un-framed units here; locate_framed() applies the frame as the host does."""
    p = _plan_unframed(colvals, entries, R, GO, GE, max_len)
    if p is None:
        return None
    p["framed"] = False
    if not allow_frame:
        return p
    fin = entries[np.isfinite(entries)]
    wmax = float(np.max(np.abs(fin))) if fin.size else 0.0
    splus = sum(max(0.0, float(np.max(v))) for v in colvals)
    rowzero = [0.0] + [-(GO + GE * (c - 1)) for c in range(1, R + 1)]
    rzplus, rzmag = max(0.0, max(rowzero)), max(abs(v) for v in rowzero)
    bneg = GO + GE * R + rzmag
    bpos = splus + rzplus
    bmag = max(bneg, bpos) + wmax + GO
    nops = 2.0 * R + 4.0 + (2.0 * bpos + bneg) / GE
    eps = 2.0 * nops * bmag * 2.0 ** -53
    lenx = float(max_len) + R + 2.0
    kf = p["k"]
    while kf >= LOC_FRAME_KMIN and (bmag + GE * lenx) * 2.0 ** kf + 2.0 * (R + 4) > 2.0 ** 30:
        kf -= 1
    gof, gef = math.ldexp(GO, kf), math.ldexp(GE, kf)
    if kf < LOC_FRAME_KMIN or gof != math.floor(gof) or gef != math.floor(gef):
        return p
    return dict(k=kf, GO=int(gof), GE=int(gef), D=(R + 1) + int(math.ceil(2.0 * eps * 2.0 ** kf)) + 1,
                unit=2.0 ** -kf, slack=(R + 1) * 2.0 ** -(kf + 1) + eps, top=bpos + 1.0,
                rz=[int(np.rint(math.ldexp(v, kf))) for v in rowzero], framed=True,
                bound=(bmag + GE * lenx) * 2.0 ** kf + 2.0 * (R + 4))


def locate_framed(w, lens, plan, R, block=None, row_origin=0, seen=None):
    """The framed fill as the kernel runs it.  row_origin numbers the rows from there instead of 0 (the frame of the last
    rows of a read that much longer: the recurrence is invariant under a common shift, the int32 range is not).  seen:
    [min, max] of every finite value formed, sentinels excluded, updated in place."""
    B = len(lens)
    k, GEi, D = plan["k"], plan["GE"], plan["D"]
    GOO = plan["GO"] - GEi
    fin = np.isfinite(w)
    wi = np.where(fin, np.rint(np.ldexp(np.where(fin, w, 0.0), k)) + 2 * GEi, LOC_NEG_FRAMED).astype(np.int64)
    rz = [plan["rz"][c] + GEi * (c + row_origin) for c in range(R + 1)]
    S = [np.full(B, rz[c], np.int64) for c in range(R + 1)]
    UJ = [np.full(B, LOC_NEG, np.int64) for _ in range(R + 1)]
    lo = np.zeros(B, np.int64)
    hi = np.zeros(B, np.int64)
    s_before = S[R].copy()
    xacc = np.full(B, LOC_NEG, np.int64)
    inblk = np.zeros(B, bool)
    D_lo = D + GEi   # two-row blocks: the last row's frame lies one GE above the first row's

    def note(*vals):
        if seen is not None:
            for v in vals:
                seen[0], seen[1] = min(seen[0], int(v.min())), max(seen[1], int(v.max()))

    for i in range(1, int(lens.max(initial=0)) + 1):
        act = i <= lens
        col0, col0_up = GEi * (i + row_origin), GEi * (i - 1 + row_origin)
        left, lj, diag = np.full(B, col0, np.int64), np.full(B, LOC_NEG, np.int64), np.full(B, col0_up, np.int64)
        for c in range(1, R + 1):
            last = c == R
            lg = left - GOO
            H = np.maximum(lj, lg)
            lj = H
            # column R: the free vertical step gains GE; its jump score never exceeds the cell above, so it rides free
            V = np.maximum(UJ[c], S[c] - (-GEi if last else GOO))
            M = diag + wi[:, i - 1, c - 1]
            assert int(M.min()) >= -(1 << 31), "diag' + LOC_NEG_FRAMED left int32"
            sentinel = wi[:, i - 1, c - 1] == LOC_NEG_FRAMED
            assert not (sentinel & (M >= H)).any(), "an -inf table entry reached a real cell"
            diag = S[c]
            X = np.maximum(M, H)
            best = np.maximum(X, V)
            note(lg, H, np.where(sentinel, H, M), V, best)   # all of them real: S, column 0 and lg are
            UJ[c] = np.where(act, V, UJ[c])
            S[c] = np.where(act, best, S[c])
            left = best
            if last:
                if block is None:
                    single = act
                elif (i - block) % 2 == 0:
                    inblk = act & (i + 1 <= lens)
                    s_before, xacc = V.copy(), X.copy()          # both in the frame of the block's first row
                    single = act & ~inblk
                else:
                    xacc = np.maximum(xacc, X - GEi)
                    bd = best - D_lo
                    lo = np.where(inblk & (bd > s_before), i - 1, lo)
                    hi = np.where(inblk & (xacc >= bd), i, hi)
                    single = act & ~inblk
                    inblk = np.zeros(B, bool)
                lo = np.where(single & (best - D > V), i, lo)      # one row: one frame
                hi = np.where(single & (X + D >= best), i, hi)
    imax = S[R] - GEi * (lens + row_origin + R)                    # column R's last row is the read's last
    return imax, lo, hi


def _batch(oracle, oenc, seed, nrand, qlo, qhi, ref):
    reads = model._families(seed, nrand)
    quals = model._quals(reads, seed + 1, qlo, qhi)
    w, colvals, entries = model.costs(oracle, oenc, ref, reads, quals)
    return reads, quals, w, colvals, entries, np.array([len(r) for r in reads])


PENALTIES = [(5, 1), (0, 1), (2.5, 0.5), (4, 0.25)]


@pytest.mark.parametrize("gapopen,gapext", PENALTIES)
@pytest.mark.parametrize("ref", [ADAPTOR, "ACGTNNNNACGTRYACGTVHACGT", "ACGTA"])
def test_framed_fill_returns_the_unframed_integers(oracle, oenc, ref, gapopen, gapext):
    R = len(ref)
    _, _, w, colvals, entries, lens = _batch(oracle, oenc, 21, 120, 33, 126, ref)   # '!': match scores of -inf
    plan = plan_locate(colvals, entries, R, gapopen + gapext, gapext, int(lens.max()))
    assert plan is not None and plan["framed"] and plan["k"] >= LOC_FRAME_KMIN
    for block in (None, 0, 1):
        want = _locate_unframed(w, lens, plan, R, block)
        got = locate_framed(w, lens, plan, R, block)
        for a, b in zip(want, got):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("qlo,qhi", [(33, 126), (38, 75)])
def test_framed_model_matches_oracle(oracle, oenc, monkeypatch, qlo, qhi):
    """The un-framed model's whole check (windows from [lo, hi] and I_max against the oracle's score, map and outputs)
    with the frame's plan and fill in place of its own."""
    monkeypatch.setattr(model, "plan_locate", plan_locate)
    monkeypatch.setattr(model, "locate", locate_framed)
    reads = model._families(qlo + qhi + 1, 150)
    quals = model._quals(reads, qhi, qlo, qhi)
    for gapopen, gapext in ((5, 1), (2.5, 0.5)):
        assert model.check(oracle, oenc, reads, quals, ADAPTOR, gapopen, gapext, [9], [21]) == 0


@pytest.mark.parametrize("table", TABLES, ids=TABLE_IDS)
def test_framed_model_under_other_tables(oracle, table, monkeypatch):
    reads = model._families(5, 40)
    quals = draw_quals(table, [len(r) for r in reads], 17)
    if model.locator_plan(oracle, table.oenc, ADAPTOR, 5, 1, max(len(r) for r in reads)) is None:
        return   # the call takes the snapshot path with or without the frame
    monkeypatch.setattr(model, "plan_locate", plan_locate)
    monkeypatch.setattr(model, "locate", locate_framed)
    assert model.check(oracle, table.oenc, reads, quals, ADAPTOR, 5, 1, [9], [21]) == 0


@pytest.mark.parametrize("gapopen,gapext", PENALTIES)
@pytest.mark.parametrize("max_len", [1, 300, 2000, 20_000, 70_000, 1_000_000])
def test_k_rule_keeps_the_frame_in_range(oracle, oenc, max_len, gapopen, gapext):
    """The frame at the rows of a read of max_len bases: every value stays within the stated bound (<= 2^30) and above
    -2^27, and the fill still returns the un-framed integers."""
    R = len(ADAPTOR)
    _, _, w, colvals, entries, lens = _batch(oracle, oenc, 31, 60, 33, 126, ADAPTOR)
    GO, GE = gapopen + gapext, gapext
    plan = plan_locate(colvals, entries, R, GO, GE, max(max_len, int(lens.max())))
    old = _plan_unframed(colvals, entries, R, GO, GE, max(max_len, int(lens.max())))
    assert plan is not None and plan["framed"] and LOC_FRAME_KMIN <= plan["k"] <= old["k"]
    assert plan["bound"] <= 2.0 ** 30
    seen = [0, 0]
    origin = max(0, max_len - int(lens.max()))
    got = locate_framed(w, lens, plan, R, 0, row_origin=origin, seen=seen)
    want = _locate_unframed(w, lens, plan, R, 0)
    for a, b in zip(want, got):
        assert np.array_equal(a, b)
    assert -(1 << 27) < seen[0] and seen[1] <= plan["bound"] <= 2.0 ** 30
    if (gapopen, gapext) == (5, 1) and max_len == 2000:
        assert plan["k"] == 18 and old["k"] == 20   # the benchmark's call


def test_k_rule_falls_back_where_no_k_fits(oracle, oenc):
    """Reads too long (or extensions too dear) for any k >= 8: the plan is the un-framed one, unchanged."""
    R = len(ADAPTOR)
    _, colvals, entries = model.costs(oracle, oenc, ADAPTOR, [""], [""])
    for GO, GE, max_len in ((6, 1, 5_000_000), (128, 64, 70_000)):
        old = _plan_unframed(colvals, entries, R, GO, GE, max_len)
        new = plan_locate(colvals, entries, R, GO, GE, max_len)
        assert old is not None and not new["framed"]
        assert {k: v for k, v in new.items() if k != "framed"} == old
