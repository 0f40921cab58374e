"""CPU model of adaptor_align's locator path (align.hip: MODE 5 locator, MODE 4 window; the argument above LOC_NEG).

Restates in numpy, batched over reads: the host's plan_locate (k, D, slack, top), the integer locator fill with its
candidate rows [lo, hi] (per row and per two-row block, both block phases), the window height Wc, and an fp64 window DP
in the reference's own formulation (oracle/align.c dp_fill: penalty selects, jump lengths) started at r0 from a fresh
boundary.  The reference's backtrack run on the window's directions must give the oracle's score bits and map, and must
never read a row above r0.  The window top is taken both as the kernel rounds it (down to 8 rows) and exactly at r0, the
tallest start the certificate allows.  A window of R rows (the certificate without its score term) must fail on the
adversarial families, so the comparison is shown to be able to see a wrong bound.
"""
import math

import numpy as np
import pytest

from tests.encodings import TABLE_IDS, TABLES, draw_quals

LOC_NEG = -(1 << 29)
ADAPTOR = "ACGATCAGC" + "N" * 12 + "GTCAGTCAG"
FILLED = "ACGATCAGC" + "ACGTTGCAAGTC" + "GTCAGTCAG"


def costs(oracle, oenc, ref, reads, quals):
    """w[b, i, c]: score of read b's base i against reference column c + 1 (oracle/align.c cell_cost); plus the table
    entries each column can address and every entry of the device table (for plan_locate)."""
    errors, names = oenc
    m, mm = oracle.cost_tables(errors)
    n, off = len(errors), int(np.int8(np.uint8(names[0])))   # the first name as the reference reads it: a signed char
    Lmax = max(1, max(len(r) for r in reads))
    w = np.zeros((len(reads), Lmax, len(ref)))
    colvals, used = [], [m[0], mm[0]]
    for c, r in enumerate(ref):
        if r in "ACGT":
            colvals.append(np.concatenate([m[0], mm[0]]))
        else:
            t = (mm[1] if r in "MRWSYK" else m[2] if r in "VHDB" else m[3])
            colvals.append(t)
            used.append(t)
        for b, (s, q) in enumerate(zip(reads, quals)):
            if not s:
                continue
            loc = np.minimum(np.frombuffer(q.encode() if isinstance(q, str) else q, np.int8).astype(int) - off, n - 1)
            if r in "ACGT":
                hit = np.frombuffer(s.encode(), np.uint8) == ord(r)
                w[b, :len(s), c] = np.where(hit, m[0][loc], mm[0][loc])
            else:
                w[b, :len(s), c] = (mm[1] if r in "MRWSYK" else m[2] if r in "VHDB" else m[3])[loc]
    return w, colvals, np.concatenate(used)


def plan_locate(colvals, entries, R, GO, GE, max_len):
    """align.hip plan_locate, statement by statement."""
    if not (GE > 0 and GO >= GE):
        return None
    if np.isnan(entries).any() or (entries == np.inf).any():
        return None
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
    eps_alt = 2.0 * 2.0 * lenx * (bmag + GE * lenx) * 2.0 ** -53
    if not eps + eps_alt < 0.25:
        return None
    k = 24
    while k > 0 and (bmag + GE) * 2.0 ** k + 2.0 * (R + 4) > 2.0 ** 27:
        k -= 1
    if (bmag + GE) * 2.0 ** k + 2.0 * (R + 4) > 2.0 ** 27:
        return None
    go, ge = math.ldexp(GO, k), math.ldexp(GE, k)
    if go != math.floor(go) or ge != math.floor(ge):
        return None
    return dict(k=k, GO=int(go), GE=int(ge), D=(R + 1) + int(math.ceil(2.0 * eps * 2.0 ** k)) + 1,
                unit=2.0 ** -k, slack=(R + 1) * 2.0 ** -(k + 1) + eps, top=bpos + 1.0,
                rz=[int(np.rint(math.ldexp(v, k))) for v in rowzero])


def locator_plan(oracle, oenc, ref, gapopen, gapext, max_len):
    """plan_locate for a call of adaptor_align as the host makes it (None: the call takes the snapshot path)."""
    _, colvals, entries = costs(oracle, oenc, ref, [""], [""])
    return plan_locate(colvals, entries, len(ref), gapopen + gapext, gapext, max_len)


def locate(w, lens, plan, R, block=None):
    """Pass 1 as the kernel runs it: int32 max-plus DP, every penalty opened (gapopen >= 0).  Returns I_max and the
    candidate rows lo / hi; block = None: per row, else two-row blocks starting at rows of that parity."""
    B = len(lens)
    k = plan["k"]
    wi = np.where(np.isfinite(w), np.rint(np.ldexp(np.where(np.isfinite(w), w, 0.0), k)), LOC_NEG).astype(np.int64)
    GOi, GEi, D = plan["GO"], plan["GE"], plan["D"]
    S = [np.full(B, plan["rz"][c], np.int64) for c in range(R + 1)]
    UJ = [np.full(B, LOC_NEG, np.int64) for _ in range(R + 1)]
    lo = np.zeros(B, np.int64)
    hi = np.zeros(B, np.int64)
    s_before = S[R].copy()
    xacc = np.full(B, LOC_NEG, np.int64)
    inblk = np.zeros(B, bool)
    for i in range(1, int(lens.max(initial=0)) + 1):
        act = i <= lens
        left, lj, diag = np.zeros(B, np.int64), np.full(B, LOC_NEG, np.int64), np.zeros(B, np.int64)
        for c in range(1, R + 1):
            last = c == R
            H = np.maximum(lj - GEi, left - GOi)
            lj = H
            V = np.maximum(UJ[c] - (0 if last else GEi), S[c] - (0 if last else GOi))
            M = diag + wi[:, i - 1, c - 1]
            diag = S[c]
            X = np.maximum(M, H)
            best = np.maximum(X, V)
            UJ[c] = np.where(act, V, UJ[c])
            S[c] = np.where(act, best, S[c])
            left = best
            if last:
                if block is None:
                    single = act
                elif (i - block) % 2 == 0:      # first row of a two-row block
                    inblk = act & (i + 1 <= lens)
                    s_before, xacc = V.copy(), X.copy()
                    single = act & ~inblk
                else:                           # its second row: the block's conditions, as the kernel's ballots
                    xacc = np.maximum(xacc, X)
                    lo = np.where(inblk & (best - D > s_before), i - 1, lo)
                    hi = np.where(inblk & (xacc + D >= best), i, hi)
                    single = act & ~inblk
                    inblk = np.zeros(B, bool)
                lo = np.where(single & (best - D > V), i, lo)
                hi = np.where(single & (X + D >= best), i, hi)
    return S[R], lo, hi


def window(w, lens, ts, hi, R, GO, GE):
    """fp64 DP in the reference's formulation from row ts (ts > 0: -inf above, zeros in column 0; ts = 0: the true row
    0) through row hi.  Returns the score at (hi, R) and the directions D[c][t], t = row - base."""
    B = len(lens)
    fresh = ts > 0
    base = np.where(fresh, ts - 1, 0)
    T = int((hi - base).max(initial=0)) + 1
    rows = base[:, None] + np.arange(T + 1)[None, :]
    Lw = w.shape[1]
    wt = np.take_along_axis(w, np.clip(rows - 1, 0, Lw - 1)[:, :, None].repeat(R, 2), 1)
    S = np.zeros((B, T + 1))
    Dp = np.full((B, T + 1), -1, np.int64)
    LJ = np.full((B, T + 1), -np.inf)
    LP = np.zeros((B, T + 1), np.int64)
    Dall = [Dp]
    with np.errstate(invalid="raise"):
        for c in range(1, R + 1):
            pos = c - 1
            last = c == R
            VGO, VGE = (0.0, 0.0) if last else (GO, GE)
            Dc = np.zeros((B, T + 1), np.int64)
            lag = S[:, 0].copy()
            S[:, 0] = np.where(fresh, -np.inf, S[:, 0] - np.where(Dp[:, 0] > 0, GE, GO))
            Dc[:, 0] = 1
            UJ = np.full(B, -np.inf)
            UP = np.zeros(B, np.int64)
            for t in range(1, T + 1):
                H = S[:, t] - np.where(Dp[:, t] > 0, GE, GO)
                LJ[:, t] -= GE
                take = LJ[:, t] > H
                hstep = np.where(take, 1 + pos - LP[:, t], 1)
                H = np.where(take, LJ[:, t], H)
                LJ[:, t] = H
                LP[:, t] = np.where(take, LP[:, t], pos)
                V = S[:, t - 1] - np.where(Dc[:, t - 1] < 0, VGE, VGO)
                UJ = UJ - VGE
                takev = UJ > V
                row = rows[:, t]
                vstep = np.where(takev, 1 + row - UP, 1)
                V = np.where(takev, UJ, V)
                UJ = V
                UP = np.where(takev, UP, row)
                M = lag + wt[:, t, c - 1]
                lag = S[:, t].copy()
                dg = (M > H) & (M > V)
                hz = ~dg & (H > V)
                S[:, t] = np.where(dg, M, np.where(hz, H, V))
                Dc[:, t] = np.where(dg, 0, np.where(hz, hstep, -vstep))
            Dall.append(Dc)
            Dp = Dc
    score = S[np.arange(B), hi - base]
    return score, Dall, base


def backtrack(Dget, R, row, rtop):
    """oracle/align.c backtrack from (row, R); Dget(c, row) -> direction.  None if it reads a row above rtop."""
    pos, diag = [0] * (R + 1), [0] * (R + 1)
    c = R

    def get(cc, rr):
        if rr < rtop:
            raise LookupError
        return Dget(cc, rr)

    try:
        while c > 0:
            while row > 0 and get(c, row) < 0:
                row += get(c, row)
            d = get(c, row)
            if d == 0:
                pos[c], diag[c] = row, 1
                row -= 1
                c -= 1
            else:
                for _ in range(d):
                    pos[c], diag[c] = row + 1, 0
                    c -= 1
    except LookupError:
        return None
    return pos, diag


def outputs(pos, diag, L, R, ss, se):
    """align.hip's interval() + the adaptor_align outputs (unsigned 32-bit wrap as there)."""
    u = lambda v: v & 0xFFFFFFFF
    i32 = lambda v: int(np.uint32(u(v)).view(np.int32))
    s, e = u(pos[1] - 1), u(pos[R] + diag[R] - 1)
    st, en = (i32(s + 1), i32(e)) if s < e else (0, 0)
    secs = []
    for a, b in zip(ss, se):
        s = u((1 if a == 0 else pos[a] + diag[a]) - 1)
        e = u((L + 1 if b + 1 == R + 1 else pos[b + 1]) - 1)
        secs.append((i32(s + 1), i32(u(e - s))))
    return st, en, secs


def check(oracle, oenc, reads, quals, ref, gapopen, gapext, ss, se, wc_override=None):
    """Runs the model on one batch; returns the number of reads whose window differs from the oracle (0 expected)."""
    R = len(ref)
    GO, GE = gapopen + gapext, gapext
    w, colvals, entries = costs(oracle, oenc, ref, reads, quals)
    lens = np.array([len(r) for r in reads])
    plan = plan_locate(colvals, entries, R, GO, GE, int(lens.max(initial=0)))
    assert plan is not None
    ref_out = oracle.adaptor_align(reads, quals, oenc, gapopen, gapext, ref, ss, se)
    bad = 0
    for block in (None, 0, 1):
        imax, lo, hi = locate(w, lens, plan, R, block)
        f_low = imax * plan["unit"] - plan["slack"]
        over = np.floor((plan["top"] - f_low) / GE) + 1.0
        wc = R + np.where(over > 0, np.minimum(over, 1e6), 0).astype(np.int64)
        if wc_override is not None:
            wc = wc_override(wc)
        r0 = lo - wc
        for ts in (np.where(r0 < 8, 0, r0 & ~7), np.maximum(r0, 0)):
            score, Dall, base = window(w, lens, ts, hi, R, GO, GE)
            for b in range(len(reads)):
                L = int(lens[b])
                full_score, dirs = oracle.align_one(ref, reads[b], quals[b], oenc, gapopen, gapext, True, want_dirs=True)
                # candidate rows hold every row of column R whose X is the score, in particular the landing row
                row = L
                while row > 0 and dirs[R, row] < 0:
                    row += dirs[R, row]
                assert lo[b] <= row <= hi[b] or (L == 0 and row == 0)
                ok = np.float64(score[b]).view(np.int64) == np.float64(ref_out[0][b]).view(np.int64)
                ok = ok and np.float64(full_score).view(np.int64) == np.float64(ref_out[0][b]).view(np.int64)
                got = backtrack(lambda c, r: int(Dall[c][b, r - base[b]]), R, int(hi[b]), int(ts[b]) if ts[b] > 0 else 0)
                want = backtrack(lambda c, r: int(dirs[c, r]), R, L, 0)
                ok = ok and got is not None and got == want
                if ok:
                    st, en, secs = outputs(*got, L, R, ss, se)
                    ok = st == ref_out[1][b] and en == ref_out[2][b]
                    ok = ok and all(x == (ref_out[3][k][b], ref_out[4][k][b]) for k, x in enumerate(secs))
                bad += not ok
    return bad


def _families(seed, nrand):
    rng = np.random.default_rng(seed)
    nuc = np.array(list("ACGT"))

    def body(n):
        return "".join(nuc[rng.integers(0, 4, n)])

    reads = []
    for gap in (0, 1, 3, 7, 20, 45):                       # two identical adaptor copies
        reads.append(body(30) + FILLED + body(gap) + FILLED + body(20))
    for n in (10, 11, 12, 13, 14):                         # ties through the N run
        reads.append(body(40) + FILLED[:9] + body(n) + FILLED[21:] + body(30))
    for ins in (3, 8, 15, 25, 40, 60):                     # long vertical gaps inside the hit
        reads.append(body(50) + FILLED[:15] + body(ins) + FILLED[15:] + body(10))
        reads.append(body(20) + FILLED[:6] + body(ins) + FILLED[6:24] + body(ins // 2) + FILLED[24:])
    reads += [FILLED[:5], FILLED[:29], FILLED, FILLED + body(60), "", "N" * 40, body(7), "N" * 9 + FILLED[9:]]
    for _ in range(nrand):                                 # random reads, with and without a planted hit
        b = body(int(rng.integers(0, 160)))
        if rng.random() < 0.6:
            e = int(rng.integers(0, len(b) + 1))
            a = list(FILLED)
            for _ in range(int(rng.integers(0, 4))):      # a few edits in the hit
                p = int(rng.integers(0, len(a)))
                op = rng.integers(0, 3)
                if op == 0:
                    a[p] = str(nuc[rng.integers(0, 4)])
                elif op == 1:
                    del a[p]
                else:
                    a.insert(p, str(nuc[rng.integers(0, 4)]) * int(rng.integers(1, 6)))
            b = b[:e] + "".join(a) + b[e:]
        reads.append(b)
    return reads


def _quals(reads, seed, lo, hi):
    rng = np.random.default_rng(seed)
    return [rng.integers(lo, hi + 1, len(r)).astype(np.uint8).tobytes().decode() for r in reads]


@pytest.mark.parametrize("qlo,qhi", [(33, 126), (38, 75), (33, 33), (126, 126)])
def test_model_matches_oracle(oracle, oenc, qlo, qhi):
    reads = _families(qlo + qhi, 300)
    quals = _quals(reads, qhi, qlo, qhi)
    assert check(oracle, oenc, reads, quals, ADAPTOR, 5, 1, [9], [21]) == 0


# Tables the model's plan_locate refuses at (ADAPTOR, 5 / 1); every other table of tests/encodings.py is eligible.  The
# GPU test (tests/test_gpu_encodings.py) expects the locator path exactly where this says so.
REFUSED = ()


@pytest.mark.parametrize("table", TABLES, ids=TABLE_IDS)
def test_model_matches_oracle_under_other_tables(oracle, table):
    """The exactness argument's constants (k, D, slack, top) come from the table: the same families under every table
    of tests/encodings.py, qualities drawn from the first name to six past the last."""
    reads = _families(5, 60)
    quals = draw_quals(table, [len(r) for r in reads], 17)
    plan = locator_plan(oracle, table.oenc, ADAPTOR, 5, 1, max(len(r) for r in reads))
    if table.name in REFUSED:
        assert plan is None
        return
    assert plan is not None and 0 < plan["k"] <= 24
    assert check(oracle, table.oenc, reads, quals, ADAPTOR, 5, 1, [9], [21]) == 0


@pytest.mark.parametrize("ref,go,ge", [("ACGTACGTAC", 2, 0.5), (ADAPTOR, 0, 1), ("ACGTNNNNACGTRYACGTVHACGT", 5, 1), ("A", 3, 1)])
def test_model_other_adaptors(oracle, oenc, ref, go, ge):
    reads = _families(7, 150)
    quals = _quals(reads, 8, 35, 80)
    assert check(oracle, oenc, reads, quals, ref, go, ge, [0], [len(ref)]) == 0


def test_window_without_the_score_term_fails(oracle, oenc):
    """Wc = R (no vertical steps allowed above the candidates): the comparison above must catch it."""
    reads = _families(11, 0)
    quals = _quals(reads, 12, 38, 75)
    assert check(oracle, oenc, reads, quals, ADAPTOR, 5, 1, [9], [21], wc_override=lambda wc: wc * 0 + len(ADAPTOR)) > 0
