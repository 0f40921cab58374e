"""Alignment builders shared by tests/test_oracle_consensus_columns.py (CPU: the builders against the oracle, so the
columns are where they claim to be) and tests/test_gpu_consensus_columns.py (GPU: every vote kernel against the oracle).

The vote decides three things in floating point: the Phred character round(x), the base (first maximum of four fp64
sums) and whether a column is kept (!(incidence < nrows * mincov)).  The families put columns where each decision is
close: A and B next to k + 0.5 (engineered and searched), C on equal or nearly equal sums, D on the coverage products,
E on more boundary columns than the device's list held at first.

numpy and the standard library only; every draw is seeded."""
import functools
import math
from decimal import Decimal, getcontext

import numpy as np

BASES = "ACGT"
LN10 = math.log(10.0)
PREC = 50                      # decimal digits of the solvers
E_LO, E_HI = 1e-8, 0.74        # below 1e-8 the vote clamps the error, above 0.75 the agreed base is not the maximum
FILL = 8                       # agreeing columns between two engineered ones (keeps the MSA stage from moving them)
DEFAULT_SCORES = (0, -1, -5, -1, 100)   # match, mismatch, gap extension, gap opening, bandwidth

A_ROWS = (1, 2, 3, 5, 8, 13, 64)
A_ROWS_ODD = (3, 8, 64)
_D = (3e-10, 1e-8, 1e-7, 1e-6, 1e-5, 1e-4, 1.9e-4, 2.1e-4, 3.9e-4, 4.1e-4, 1e-3)
DELTAS = (0.0,) + tuple(s * d for d in _D for s in (1, -1))
# basic vote: (rows, Phred level) -- the pseudo-count is per call
BASIC_PAIRS = ((1, 2), (2, 5), (3, 9), (5, 14), (5, 20), (8, 25), (13, 30), (20, 36), (33, 41), (64, 47), (100, 53), (7, 60))


def phred_table():
    """(errors, names) of Phred+33, '!' .. '~'"""
    return np.power(10.0, -np.arange(94) / 10.0), bytes(range(33, 127))


def phred_values(lerr):
    """log errors -> the Phred values whose rounding gives the character"""
    return -10.0 * np.asarray(lerr, dtype=np.float64) / LN10


def boundary_distance(x):
    """signed distance of x from the nearest k + 0.5"""
    x = np.asarray(x, dtype=np.float64)
    return (x - np.floor(x)) - 0.5


# ---------------------------------------------------------------------------
# Family A: engineered boundaries

def _dec(v):
    return Decimal(repr(float(v))) if not isinstance(v, Decimal) else v


def solve_agree(n, x):
    """Error e with 10 log10(1 + (3 (1 - e) / e)^n / 3) = x: n rows agree at one quality."""
    getcontext().prec = PREC
    t = Decimal(10) ** (_dec(x) / 10)
    r = (3 * (t - 1)) ** (Decimal(1) / Decimal(n))
    return float(Decimal(3) / (r + 3))


def solve_odd(n, x):
    """Error e at which n - 1 rows with one base and one row with another, all at quality e, have the Phred value x.
    With a = 3 (1 - e) / e the four scores are, up to a common term, log of (a^(n-1), a, 1, 1), so
    10^(x/10) = (a^(n-1) + a + 2) / (a + 2).  h(a) = a^(n-1) + a + 2 - T (a + 2) is convex for a > 0 and positive at
    a0 = (3 T)^(1/(n-2)) >= 1 (a + 2 <= 3 a there), so Newton's iteration from a0 descends onto the root."""
    assert n >= 3
    getcontext().prec = PREC
    t = Decimal(10) ** (_dec(x) / 10)
    a = max(Decimal(1), (3 * t) ** (Decimal(1) / Decimal(n - 2)))
    tol = Decimal(10) ** (-(PREC - 8))
    for _ in range(200):
        h = a ** (n - 1) + a + 2 - t * (a + 2)
        step = h / ((n - 1) * a ** (n - 2) + 1 - t)
        a -= step
        if abs(step) <= tol * a:
            break
    else:
        raise AssertionError("solve_odd did not converge")
    return float(Decimal(3) / (a + 3))


@functools.lru_cache(maxsize=None)
def boundary_table(n, delta, odd=False):
    """The encoding table of one (rows, offset): for every level k = 1 .. 92 whose error lies inside (E_LO, E_HI) the
    error that puts the column on k + 0.5 + delta.  Returns (levels, errors, names); the errors decrease with k."""
    solve = solve_odd if odd else solve_agree
    levels, errors = [], []
    for k in range(1, 93):
        e = solve(n, Decimal(k) + Decimal("0.5") + _dec(delta))
        if E_LO < e < E_HI:
            levels.append(k)
            errors.append(e)
    errors = np.array(errors)
    assert len(levels) <= 92 and np.all(np.diff(errors) < 0)
    return tuple(levels), errors, bytes(range(33, 33 + len(levels)))


def _other_base(rng, base):
    return BASES[(BASES.index(base) + int(rng.integers(1, 4))) % 4]


@functools.lru_cache(maxsize=None)
def boundary_alignment(n, delta, odd=False):
    """One alignment of n gap-free rows for boundary_table(n, delta, odd): per table entry one engineered column at
    that quality (all rows agree; odd: one row, another one from column to column, carries another base), each
    followed by FILL columns in which all rows agree, at a quality from the middle of the table.  The bases depend on
    (n, odd) only.  Returns (rows, quals, (errors, names), levels, engineered column indices)."""
    levels, errors, names = boundary_table(n, delta, odd)
    rng = np.random.default_rng(1000 * n + int(odd))
    ncol = len(levels) * (1 + FILL)
    truth = [BASES[i] for i in rng.integers(0, 4, ncol)]
    rows = [list(truth) for _ in range(n)]
    cols = np.arange(len(levels)) * (1 + FILL)
    if odd:
        for j, c in enumerate(cols):
            rows[(3 * j + 1) % n][c] = _other_base(rng, truth[c])
    q = [names[len(levels) // 2]] * ncol
    for j, c in enumerate(cols):
        q[c] = names[j]
    qual = bytes(q).decode("latin-1")
    return ["".join(r) for r in rows], [qual] * n, (errors, names), levels, cols


def basic_pseudo_count(n, x):
    """Pseudo-count at which n agreeing rows have the basic vote's Phred value 10 log10((n + pc) / (0.75 pc)) = x."""
    getcontext().prec = PREC
    return float(Decimal(n) / (Decimal("0.75") * Decimal(10) ** (_dec(x) / 10) - 1))


def basic_alignment(n, width=40):
    rng = np.random.default_rng(77 + n)
    return ["".join(BASES[i] for i in rng.integers(0, 4, width))] * n


# ---------------------------------------------------------------------------
# the reference's chain, vectorised (fp64, same branches as R's log1pexp)

def _log1pexp(x):
    with np.errstate(over="ignore"):
        return np.where(x <= 18.0, np.log1p(np.exp(np.minimum(x, 18.0))), np.where(x > 33.3, x, x + np.exp(-x)))


def column_sums(codes, quals, errors, order=None):
    """codes, quals: int arrays [rows, columns] (base 0..3, index into errors) -> the four sums [4, columns], rows added
    in `order` (default: row order, which is the reference's)."""
    e = np.clip(np.asarray(errors, dtype=np.float64), 1e-8, 0.99999999)
    right, wrong = np.log1p(-e), np.log(e / 3)
    s = np.zeros((4, codes.shape[1]))
    for r in (range(codes.shape[0]) if order is None else order):
        rq, wq = right[quals[r]], wrong[quals[r]]
        for b in range(4):
            s[b] += np.where(codes[r] == b, rq, wq)
    return s


def chain_phred(s):
    """Phred value of columns from their four sums [4, columns]"""
    t = np.sort(s, axis=0)
    denom = t[0] + _log1pexp(t[1] - t[0])
    denom = denom + _log1pexp(t[2] - denom)
    err3 = denom
    denom = denom + _log1pexp(t[3] - denom)
    return -10.0 * (err3 - denom) / LN10


def _strings(codes, quals, names):
    lut = np.frombuffer(BASES.encode(), np.uint8)
    qlut = np.frombuffer(names, np.uint8)
    return [lut[r].tobytes().decode() for r in codes], [qlut[r].tobytes().decode("latin-1") for r in quals]


def interleave(rows, quals, fill_qual, seed):
    """FILL agreeing columns (random base, quality character fill_qual) after every column of a gap-free alignment"""
    rng = np.random.default_rng(seed)
    w = len(rows[0])
    fill = ["".join(BASES[i] for i in rng.integers(0, 4, FILL)) for _ in range(w)]
    out_r = ["".join(r[c] + fill[c] for c in range(w)) for r in rows]
    out_q = ["".join(q[c] + fill_qual * FILL for c in range(w)) for q in quals]
    return out_r, out_q


# ---------------------------------------------------------------------------
# Family B: searched boundaries

# rows -> largest quality drawn (0 .. qmax): the deeper the alignment the lower the qualities have to be for the Phred
# value to stay below the cap of 93 (0 .. 29 leaves 41 % of the columns of 8 rows and 5 % of those of 20 rows below it).
# Kept of 10^6 draws, within 1e-3 / within 4e-4: 2 787 / 794, 905 / 339, 1 498 / 629, 761 / 358.
B_QMAX = {3: 29, 8: 29, 20: 8, 64: 4}
B_ROWS = tuple(B_QMAX)
B_DRAWS = 1_000_000
B_WIDTH = 300


@functools.lru_cache(maxsize=None)
def searched_columns(n):
    """Columns of n rows (each row agrees with the column's truth with probability 0.85, qualities uniform over
    0 .. B_QMAX[n]) whose Phred value is below 93.4 and within 1e-3 of a boundary, out of B_DRAWS seeded draws.
    Returns (codes [n, kept], quals [n, kept], Phred values [kept])."""
    rng = np.random.default_rng(4242 + n)
    errors, _ = phred_table()
    truth = rng.integers(0, 4, B_DRAWS, dtype=np.int8)
    codes = np.empty((n, B_DRAWS), np.int8)
    for r in range(n):
        miss = rng.random(B_DRAWS) >= 0.85
        codes[r] = np.where(miss, (truth + rng.integers(1, 4, B_DRAWS, dtype=np.int8)) & 3, truth)
    quals = rng.integers(0, B_QMAX[n] + 1, (n, B_DRAWS), dtype=np.int8)
    x = chain_phred(column_sums(codes, quals, errors))
    keep = (x < 93.4) & (np.abs(boundary_distance(x)) < 1e-3)
    return codes[:, keep].astype(np.int64), quals[:, keep].astype(np.int64), x[keep]


def searched_alignments(n, width=B_WIDTH, limit=None):
    """The kept columns of searched_columns(n) (the first `limit`) as gap-free alignments of `width` columns:
    (list of rows, list of quality strings), Phred+33."""
    codes, quals, _ = searched_columns(n)
    if limit is not None:
        codes, quals = codes[:, :limit], quals[:, :limit]
    _, names = phred_table()
    alns, qs = [], []
    for c0 in range(0, codes.shape[1], width):
        r, q = _strings(codes[:, c0:c0 + width], quals[:, c0:c0 + width], names)
        alns.append(r)
        qs.append(q)
    return alns, qs


def searched_fused(n, columns=60, per_group=30):
    """The first `columns` kept columns of searched_columns(n), FILL agreeing columns (quality '5') after each, as
    alignments of per_group searched columns: what the fused routes get as reads."""
    alns, qs = searched_alignments(n, per_group, columns)
    out = [interleave(r, q, "5", 600 + n + g) for g, (r, q) in enumerate(zip(alns, qs))]
    return [o[0] for o in out], [o[1] for o in out]


# ---------------------------------------------------------------------------
# Family C: near-ties between bases

C_ROWS = (4, 6, 10, 16, 32, 64, 66, 130, 400)
C_WIDTH = 300
C_QRANGE = (2, 41)


@functools.lru_cache(maxsize=None)
def tie_columns(n, width=C_WIDTH):
    """Columns of n rows: half carry base X with qualities q, the others base Y with a permutation of q, the rows
    shuffled.  The two sums hold the same addends in different orders.  Returns (codes, quals), [n, width]."""
    assert n % 2 == 0
    rng = np.random.default_rng(99 + n)
    codes = np.empty((n, width), np.int64)
    quals = np.empty((n, width), np.int64)
    for c in range(width):
        x = int(rng.integers(0, 4))
        y = (x + int(rng.integers(1, 4))) % 4
        q = rng.integers(C_QRANGE[0], C_QRANGE[1], n // 2)
        col_c = np.array([x] * (n // 2) + [y] * (n // 2))
        col_q = np.concatenate([q, rng.permutation(q)])
        p = rng.permutation(n)
        codes[:, c], quals[:, c] = col_c[p], col_q[p]
    return codes, quals


def tie_alignment(n, width=C_WIDTH):
    codes, quals = tie_columns(n, width)
    return _strings(codes, quals, phred_table()[1])


def tie_statistics(n, width=C_WIDTH):
    """(columns whose first maximum changes when the rows are added in reverse or even rows first then odd rows,
    columns whose two largest sums are equal in row order), as boolean arrays"""
    codes, quals = tie_columns(n, width)
    errors, _ = phred_table()
    s = column_sums(codes, quals, errors)
    rev = column_sums(codes, quals, errors, order=range(n - 1, -1, -1))
    even = column_sums(codes, quals, errors, order=list(range(0, n, 2)))
    odd = column_sums(codes, quals, errors, order=list(range(1, n, 2)))
    split = even + odd
    best = np.argmax(s, axis=0)                      # first maximum
    changes = (np.argmax(rev, axis=0) != best) | (np.argmax(split, axis=0) != best)
    top = np.sort(s, axis=0)
    return changes, top[3] == top[2]


def tie_fused(per_group=10, groups=3):
    """For every row count up to 64: `groups` alignments of per_group tie columns, FILL agreeing columns after each"""
    alns, qs = [], []
    for n in C_ROWS:
        if n > 64:
            continue
        rows, quals = tie_alignment(n, per_group * groups)
        for g in range(groups):
            sl = slice(g * per_group, (g + 1) * per_group)
            r, q = interleave([x[sl] for x in rows], [x[sl] for x in quals], "5", 800 + n + g)
            alns.append(r)
            qs.append(q)
    return alns, qs


# ---------------------------------------------------------------------------
# Family D: coverage products

D_ROWS = tuple(range(1, 65)) + (65, 100, 257)


def coverage_values(nrows):
    """The minimum coverages of one row count, as the doubles the call receives"""
    vals = [k / 10 for k in range(11)] + [1 / 3, 2 / 3, 0.35, 0.6] + [j / nrows for j in range(nrows + 1)] + [1.0000001, -0.1]
    return sorted(set(vals))


@functools.lru_cache(maxsize=None)
def coverage_alignment(nrows, with_n=True):
    """One alignment of nrows rows whose columns realise every incidence count 0 .. nrows (the non-gap rows chosen at
    random, bases mostly the column's truth), then columns whose only non-gap characters are N with counts 1,
    nrows // 2 and nrows, the columns shuffled.  Returns (rows, quals); the qualities are Phred+33 '5' .. 'S'.
    with_n = False: without the columns of N (an N anywhere makes k_consensus_qf hand the group to k_consensus_q4)."""
    rng = np.random.default_rng(5000 + nrows)
    counts = list(range(nrows + 1)) + (sorted({1, max(nrows // 2, 1), nrows}) if with_n else [])
    only_n = [False] * (nrows + 1) + [True] * (len(counts) - nrows - 1)
    order = rng.permutation(len(counts))
    grid = np.full((nrows, len(counts)), "-", dtype="U1")
    for c, k in enumerate(order):
        truth = BASES[int(rng.integers(0, 4))]
        for r in rng.permutation(nrows)[:counts[k]]:
            grid[r, c] = "N" if only_n[k] else (truth if rng.random() < 0.8 else BASES[int(rng.integers(0, 4))])
    rows = ["".join(g) for g in grid]
    quals = ["".join(chr(int(v)) for v in rng.integers(53, 84, len(r.replace("-", "")))) for r in rows]
    return rows, quals


def coverage_batches():
    """minimum coverage -> the row counts whose set holds it: one loop call per value"""
    out = {}
    for n in D_ROWS:
        for v in coverage_values(n):
            out.setdefault(v, []).append(n)
    return out


@functools.lru_cache(maxsize=None)
def coverage_reads(nrows, length=36):
    """nrows reads of one template with substitutions, insertions and deletions: the MSA stage's rows have gaps, so the
    fused call meets many incidence counts.  Returns (reads, quals)."""
    rng = np.random.default_rng(7000 + nrows)
    t = [BASES[i] for i in rng.integers(0, 4, length)]
    reads = []
    for _ in range(nrows):
        r = []
        for ch in t:
            u = rng.random()
            if u < 0.06:
                continue
            if u < 0.12:
                r.append(BASES[int(rng.integers(0, 4))])
            r.append(BASES[int(rng.integers(0, 4))] if rng.random() < 0.08 else ch)
        reads.append("".join(r) or "A")
    quals = ["".join(chr(int(v)) for v in rng.integers(53, 84, len(r))) for r in reads]
    return reads, quals


# ---------------------------------------------------------------------------
# Family E: more boundary columns than the device's list holds at first (4 096 entries)

E_ROWS, E_COLUMNS, E_GROUPS = 5, 6000, 40


def flood_basic():
    """(rows, pseudo-count): 5 equal rows of 6 000 columns, every column's basic Phred value on 20.5"""
    rng = np.random.default_rng(31)
    row = "".join(BASES[i] for i in rng.integers(0, 4, E_COLUMNS))
    return [row] * E_ROWS, E_ROWS / (0.75 * 10 ** 2.05 - 1)


def flood_quality():
    """(rows, quals, (errors, names)): 5 equal rows of 6 000 columns at quality '%', whose error puts every column's
    Phred value on 25.5; the rest of the table is Phred+33"""
    rng = np.random.default_rng(32)
    e = 3 / ((3 * (10 ** 2.55 - 1)) ** (1 / E_ROWS) + 3)
    errors, names = phred_table()
    errors[ord("%") - 33] = e
    row = "".join(BASES[i] for i in rng.integers(0, 4, E_COLUMNS))
    return [row] * E_ROWS, ["%" * E_COLUMNS] * E_ROWS, (errors, names)


def split_groups(rows, quals, ngroups=E_GROUPS):
    """the columns of one gap-free alignment dealt to `ngroups` alignments"""
    w = len(rows[0]) // ngroups
    return ([[r[g * w:(g + 1) * w] for r in rows] for g in range(ngroups)],
            [[q[g * w:(g + 1) * w] for q in quals] for g in range(ngroups)])


def with_n(rows, at=-1):
    """the alignment with row 0's character at column `at` replaced by N (k_consensus_qf hands such a group over)"""
    r0 = list(rows[0])
    r0[at] = "N"
    return ["".join(r0)] + list(rows[1:])


def handover_extras(rows, quals):
    """Two more groups for a loop call on (rows, quals), gap-free: the alignment with an N in its last column, and the
    alignment repeated until it has more than 64 rows -- k_consensus_qf hands both to k_consensus_q4."""
    times = 64 // len(rows) + 1
    return [with_n(rows), list(rows) * times], [list(quals), list(quals) * times]


def flat_groups(alns):
    """alignments of gap-free rows -> (group offsets, 1-based read ids, reads) as msa_consensus_flat takes them"""
    sizes = [len(a) for a in alns]
    goff = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return goff, np.arange(1, goff[-1] + 1, dtype=np.int32), [r for a in alns for r in a]
