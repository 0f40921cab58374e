"""Inputs aimed at the wide aligner (references beyond 1 024 columns: k_align_wide_q and k_align_wide, csrc/align.hip), with
the outcome a banded call must show read off the oracle's strings alone.

k_align_wide_q's first launch stores traceback codes only near the main diagonal i = c L / R; a walk that needs a cell
without codes gives up and its read goes on a redo list, whose length `sarlacc_stage_count("align_wide_redo")` reports.
`stored()` restates WHICH cells carry codes -- from the comment on `struct WideBand` and DESIGN.md ("Codes near the main
diagonal only"), not from the kernel -- and `leaves()` says whether the path two gapped strings spell needs a cell that
does not.  The groups below put paths along the band's edges (lane 0 of a wavefront for paths above the diagonal, lane 63
for paths below), excursions at a wavefront boundary and in a wavefront's interior, alignments with L != R, the read
lengths around the queue protocol's constants (16, 47/48, 64, 128) against reference widths around a wavefront's 512 and a
lane's 8 columns, and more reads than the launch has workgroups.  Seeded, no GPU, nothing of the library under test:
shared by tests/test_align_wide_cases.py (the inputs on the oracle) and tests/test_gpu_align_wide.py (the kernels)."""
import collections

import numpy as np

GO, GE = 5, 1                 # gap penalties of the banded groups
DEFAULT_BAND = 96             # WIDE_BAND: what the option value 0 stands for
BANDS = (8, DEFAULT_BAND)
HIGH = "I"                    # Phred 40 under Phred+33: "constant and high"
COLS_PER_LANE, LANES = 8, 64  # a lane owns 8 consecutive columns, a wavefront 512

SWEEP_R = (1100, 1536, 2048)
EXCURSION_R = (1536, 2048)
EXCURSION_SPAN = 300
# (column x behind which the excursion starts) boundary: columns 363 .. 662, across 512 | 513; interior: columns 595 .. 894,
# lanes 10 .. 47 of wavefront 1 -- 300 columns do not fit in fewer lanes
EXCURSION_X = {"boundary": 362, "interior": 594}
SKEW_R = (1100, 2048)
QUEUE_LENGTHS = (1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 62, 63, 64, 65, 79, 80, 81, 111, 112, 113, 126, 127, 128, 129, 143, 144,
                 145, 191, 192, 193, 255, 256, 257)
QUEUE_R = (1025, 1032, 1033, 1536, 1537, 8191, 8192)   # a last wavefront of one column; kR = 7; kR = 0; full last wavefronts
REUSE_ONE_STRIP = (1100, 2048 // 192)    # R, workgroups per CU: 192 threads
REUSE_TWO_STRIPS = (8200, 2)             # 1 024 threads, two strips of columns

Case = collections.namedtuple("Case", "key ref reads quals tags")


def band_option(band):
    """the value of the option `align_wide_band` that selects `band` rows"""
    return 0 if band == DEFAULT_BAND else band


def sweep_d(band):
    return tuple(range(band, band + 5))


def _bases(rng, n):
    return "".join("ACGT"[v] for v in rng.integers(0, 4, max(n, 0)))


_COMPLEMENT = str.maketrans("ACGT", "TGCA")


def complemented(reads):
    """reads of the same lengths that align differently: what primes the code tiles before a banded call"""
    return [r.translate(_COMPLEMENT) for r in reads]


# ---- the stored set ----

def band_lo(w, band, L, R):
    return 512 * w * L // R - band - 2


def band_hi(w, band, L, R):
    return -((-512 * (w + 1) * L) // R) + band + 64


def stored(row, c, band, L, R):
    """does the cell (row, c), 1 <= row <= L, 1 <= c <= R, carry codes after the first launch?  (arrays or scalars)"""
    row, c = np.asarray(row, dtype=np.int64), np.asarray(c, dtype=np.int64)
    if band <= 0:
        return np.ones(np.broadcast(row, c).shape, dtype=bool)
    t = (c - 1) // COLS_PER_LANE
    w, sg = t // LANES, row + t % LANES - 1
    return (sg < 63) | ((band_lo(w, band, L, R) <= sg) & (sg <= band_hi(w, band, L, R)))


def path_cells(gapped_ref, gapped_read):
    """(rows, columns) of the DP cells behind every column of the two gapped strings"""
    a = np.frombuffer(gapped_ref.encode(), dtype=np.uint8) != ord("-")
    b = np.frombuffer(gapped_read.encode(), dtype=np.uint8) != ord("-")
    assert a.size == b.size and not (~a & ~b).any(), "gap opposite gap"
    return np.cumsum(b), np.cumsum(a)


def leaves(gapped_ref, gapped_read, band, L, R):
    """does the walk of this path give up in a first launch with `band` rows of codes?  True iff some cell of the path with
    row >= 1 and c >= 1 is not stored: a diagonal run ends in front of a cell without codes, a gap run breaks at the first
    such cell, and both are cells of the path."""
    row, c = path_cells(gapped_ref, gapped_read)
    assert (int(row[-1]), int(c[-1])) == (L, R) if row.size else (L, R) == (0, 0)
    inside = (row >= 1) & (c >= 1)
    return bool((~stored(row[inside], c[inside], band, L, R)).any())


def spells(gapped_ref, gapped_read, ref, read):
    return (len(gapped_ref) == len(gapped_read) and gapped_ref.replace("-", "") == ref and gapped_read.replace("-", "") == read)


# ---- the oracle's answers, once per case ----

_EXPECTED = {}


def expected(oracle, case, what="general", go=GO, ge=GE, **kw):
    """the oracle's result of one call on a case, computed once per session: "general" (scores, edits, gapped references,
    gapped reads), "barcode" (scores), "adaptor" (scores, starts, ends, section starts, section widths; sections in kw)"""
    key = (case.key, what, go, ge, tuple(sorted((k, tuple(v)) for k, v in kw.items())))
    if key not in _EXPECTED:
        enc = oracle.phred_encoding()
        if what == "general":
            out = oracle.general_align(case.reads, case.quals, enc, go, ge, case.ref)
        elif what == "barcode":
            out = oracle.barcode_align(case.reads, case.quals, enc, go, ge, case.ref)
        else:
            out = oracle.adaptor_align(case.reads, case.quals, enc, go, ge, case.ref, kw["sec_starts"], kw["sec_ends"])
        _EXPECTED[key] = out
    return _EXPECTED[key]


def leaving(oracle, case, band, go=GO, ge=GE):
    """per read of the case: does it leave a band of `band` rows?"""
    want = expected(oracle, case, "general", go, ge)
    return [leaves(r, q, band, len(read), len(case.ref)) for r, q, read in zip(want[2], want[3], case.reads)]


def subset(case, keep, name):
    idx = [i for i, k in enumerate(keep) if k]
    return Case(case.key + (name,), case.ref, [case.reads[i] for i in idx], [case.quals[i] for i in idx], [case.tags[i] for i in idx])


def _high(reads):
    return [HIGH * len(r) for r in reads]


# ---- group 1: paths along the band's edges, L = R ----

def edge_sweep(R, band):
    """For d = band .. band + 4: `ref[d:] + d random bases`, whose path runs d rows above the main diagonal (tight at lane 0
    of a wavefront: d <= band + 2 stays), and `d random bases + ref[:R - d]`, d rows below it (tight at lane 63).  Tags
    (side, d)."""
    rng = np.random.default_rng(1000 * R + band)
    ref = _bases(rng, R)
    reads, tags = [], []
    for d in sweep_d(band):
        reads += [ref[d:] + _bases(rng, d), _bases(rng, d) + ref[:R - d]]
        tags += [("above", d), ("below", d)]
    return Case(("sweep", R, band), ref, reads, _high(reads), tags)


def sweep_stays(d, band):
    return d <= band + 2


# ---- group 2: local excursions, L = R ----

def local_excursions(R, band):
    """`ref` with d bases deleted behind column x and d random bases inserted EXCURSION_SPAN columns later (the path runs d rows
    above the diagonal in between), and the mirror image (insertion first: d rows below), for x at a wavefront boundary and in
    a wavefront's interior.  Tags (placement, side, d)."""
    rng = np.random.default_rng(2000 * R + band)
    ref = _bases(rng, R)
    reads, tags = [], []
    for place, x in EXCURSION_X.items():
        y = x + EXCURSION_SPAN
        for d in sweep_d(band):
            reads += [ref[:x] + ref[x + d:y] + _bases(rng, d) + ref[y:], ref[:x] + _bases(rng, d) + ref[x:y - d] + ref[y:]]
            tags += [(place, "above", d), (place, "below", d)]
    assert all(len(r) == R for r in reads)
    return Case(("excursion", R, band), ref, reads, _high(reads), tags)


# ---- group 3: L != R ----

def skewed(R):
    """A 400-base deletion, a 400-base insertion, the reference's second half, R - 40 unrelated bases -- and, for reads that
    stay at either band, every 50th base dropped and every 50th base followed by a random one.  Tags: names."""
    rng = np.random.default_rng(3000 + R)
    ref = _bases(rng, R)
    m = (R - 400) // 2
    thin = "".join(ch for k, ch in enumerate(ref) if k % 50 != 25)
    thick = "".join(ch + ("ACGT"[rng.integers(0, 4)] if k % 50 == 25 else "") for k, ch in enumerate(ref))
    reads = [ref[:m] + ref[m + 400:], ref[:R // 2] + _bases(rng, 400) + ref[R // 2:], ref[R // 2:], _bases(rng, R - 40), thin, thick]
    tags = ["deletion400", "insertion400", "second_half", "unrelated", "thinned", "thickened"]
    return Case(("skewed", R), ref, reads, _high(reads), tags)


# ---- group 4: the queue protocol's constants ----

def _lightly_mutated(rng, piece):
    """same length: a substitution in about one base of 20 and, from 8 bases on, one base dropped and one inserted elsewhere"""
    s = ["ACGT"[rng.integers(0, 4)] if rng.random() < 0.05 else ch for ch in piece]
    if len(s) >= 8:
        del s[int(rng.integers(0, len(s)))]
        s.insert(int(rng.integers(0, len(s) + 1)), "ACGT"[rng.integers(0, 4)])
    return "".join(s)


def _rand_quals(rng, reads, lo=35, hi=90):
    return [rng.integers(lo, hi + 1, len(r)).astype(np.uint8).tobytes().decode() for r in reads]


def queue_edges(R):
    """One read of every length in QUEUE_LENGTHS: a lightly mutated piece of the reference from a random place.  Tags: lengths."""
    rng = np.random.default_rng(4000 + R)
    ref = _bases(rng, R)
    reads = []
    for n in QUEUE_LENGTHS:
        p = int(rng.integers(0, R - n + 1))
        reads.append(_lightly_mutated(rng, ref[p:p + n]))
    assert tuple(len(r) for r in reads) == QUEUE_LENGTHS
    return Case(("queue", R), ref, reads, _rand_quals(rng, reads), list(QUEUE_LENGTHS))


# ---- groups 5 and 6: more reads than workgroups ----

REUSE_PLANTS = {3: ("leaver", "stayer", "leaver"), 7: ("long", "empty", "long"), 11: ("stayer", "leaver", "stayer")}


def reuse(R, per_cu, cus):
    """A launch of grid = cus * per_cu workgroups, workgroup k taking the reads k, k + grid, k + 2 grid.  Reads 0 .. grid + 39
    and 2 grid .. 2 grid + 39: 0 to 60 bases, about one in fifty empty, lightly mutated pieces of the reference; the reads in
    between (up to 8 bases) only give the workgroups 0 .. 39 a third read.  Planted in the workgroups of REUSE_PLANTS, first to third read:
    "leaver" (50 bases from column 41 on: the gap behind them runs along row 50 through lane 63 of wavefront 0, outside a
    band of 8 rows), "stayer" (6 bases), "long" (60 bases), "empty".  Tags: the plant's name or ""."""
    rng = np.random.default_rng(5000 + R)
    ref = _bases(rng, R)
    grid = cus * per_cu
    n = 2 * grid + 40
    reads = []
    for i in range(n):
        top = 60 if i < grid + 40 or i >= 2 * grid else 8
        ln = 0 if rng.random() < 0.02 else int(rng.integers(0, top + 1))
        p = int(rng.integers(0, R - ln + 1))
        reads.append(_lightly_mutated(rng, ref[p:p + ln]))
    tags = [""] * n
    plant = {"leaver": ref[40:90], "stayer": ref[500:506], "long": ref[300:360], "empty": ""}
    for k, names in REUSE_PLANTS.items():
        for j, name in enumerate(names):
            reads[k + j * grid], tags[k + j * grid] = plant[name], name
    return Case(("reuse", R, cus), ref, reads, _rand_quals(rng, reads), tags), grid
