"""Plain restatement of the small kernels every pipeline path runs through -- csrc/resident.hip (k_windows, k_realize,
k_subseq, k_scramble, k_choose_strand) and k_unmask of csrc/mask.hip -- and the builders of the cases that
tests/test_resident_cases.py pins on the CPU and tests/test_gpu_resident.py runs on the device.  Python and NumPy
only, nothing compiled is imported.  Reads, qualities and alignment rows are `bytes`; everything is bytes, int32 and
bit-compared fp64, so nothing here has a tolerance.

A builder returns a list of cases; the first entry of a case names the boundary it is for."""
import functools

import numpy as np

# ---- the complement rule ------------------------------------------------------------------------------------------
# Biostrings' reverseComplement on the DNA alphabet: six pairs are swapped, every other letter of the alphabet
# (W, S, N, '-', '+', '.') is its own complement.  A byte outside the alphabet is kept as well.
SWAPPED = (b"AT", b"CG", b"MK", b"RY", b"VB", b"HD")
COMPLEMENT = np.arange(256, dtype=np.uint8)
for _a, _b in SWAPPED:
    COMPLEMENT[_a], COMPLEMENT[_b] = _b, _a

ALL_BYTES = bytes(range(256))
ALPHABET = b"ACGTMRWSYKVHDBN-+.acgtnU"      # the DNA alphabet and a few bytes outside it


def revcomp(seq):
    return COMPLEMENT[np.frombuffer(seq, np.uint8)][::-1].tobytes()


def quality(length):
    """The quality string in which a moved byte shows: position p holds p & 0xff."""
    return bytes(p & 0xff for p in range(length))


def text_quality(length):
    """The same idea within '!'..'~', for the routes that decode their strings."""
    return bytes(33 + p % 94 for p in range(length))


def read(rng, length, alphabet=ALPHABET):
    return np.frombuffer(alphabet, np.uint8)[rng.integers(0, len(alphabet), length)].tobytes()


def batch(lengths, seed, empty_last=False, qual=quality):
    """(seqs, quals) of the given lengths; with `empty_last` an empty read follows them."""
    rng = np.random.default_rng(seed)
    lengths = list(lengths) + ([0] if empty_last else [])
    return [read(rng, n) for n in lengths], [qual(n) for n in lengths]


def both_ends(lengths, seed, qual=quality):
    """The batch twice: ending in a non-empty read and ending in an empty one."""
    assert lengths[-1] > 0
    return [("last read of %d bases" % lengths[-1],) + batch(lengths, seed, False, qual),
            ("last read empty",) + batch(lengths, seed, True, qual)]


# ---- windows ------------------------------------------------------------------------------------------------------
def windows(seqs, quals, tol):
    """((front seqs, front quals), (back seqs, back quals)): the first min(tol, L) bases, and the reverse complement
    of the last min(tol, L) bases with their qualities reversed, not complemented."""
    fs, fq, bs, bq = [], [], [], []
    for s, q in zip(seqs, quals):
        k = min(tol, len(s))
        fs.append(s[:k])
        fq.append(q[:k])
        bs.append(revcomp(s[len(s) - k:]))
        bq.append(q[len(q) - k:][::-1])
    return (fs, fq), (bs, bq)


WINDOW_LENGTHS = (0, 1, 9, 10, 11, 63, 64, 65, 129, 1000)     # around the tolerances and k_windows' 64 threads
WINDOW_TOLERANCES = (0, 1, 10, 64, 65, 10 ** 6)


def window_cases(qual=quality):
    """(what, seqs, quals, tolerance)."""
    out = []
    for what, seqs, quals in both_ends(WINDOW_LENGTHS, 101, qual):
        out += [("tolerance %d, %s" % (tol, what), seqs, quals, tol) for tol in WINDOW_TOLERANCES]
    out += [("no reads, tolerance %d" % tol, [], [], tol) for tol in (0, 64)]
    return out


def complement_case():
    """The read of all 256 byte values (and, in front of it, a short one, so that it does not start at offset 0)."""
    return "all 256 byte values", [b"ACGT", ALL_BYTES], [quality(4), quality(256)]


# ---- realize ------------------------------------------------------------------------------------------------------
def realize(seqs, quals, idx, rev, ts=None, te=None):
    """(seqs, quals): read idx[r], reverse-complemented where rev[r] (qualities reversed), cut to the 1-based inclusive
    [ts[r], te[r]] of the oriented read (the whole read when None)."""
    os_, oq = [], []
    for r, i in enumerate(idx):
        s, q = seqs[i], quals[i]
        if rev[r]:
            s, q = revcomp(s), q[::-1]
        a, b = (1, len(s)) if ts is None else (int(ts[r]), int(te[r]))
        assert 1 <= a and b <= len(s)
        os_.append(s[a - 1:max(b, a - 1)])
        oq.append(q[a - 1:max(b, a - 1)])
    return os_, oq


REALIZE_LENGTHS = (0, 1, 2, 5, 127, 128, 129, 130, 300, 301)      # around k_realize's 128 threads


def realize_cases():
    """(what, idx, rev, ts, te) on a batch of REALIZE_LENGTHS (an empty read may follow: no case selects it)."""
    L = REALIZE_LENGTHS
    n = len(L)
    out = [("permuted, mixed strands", [9, 3, 0, 7, 1, 8, 2, 6, 4, 5], [r % 2 for r in range(n)], None, None),
           ("repeated", [8, 8, 4, 8, 4, 0, 0], [0, 1, 1, 0, 0, 1, 0], None, None),
           ("a strict subset", [2, 5, 9], [1, 0, 1], None, None),
           ("nothing selected", [], [], None, None)]
    some = [i for i in range(n) if L[i] >= 1]
    for rev in (0, 1):
        tag = "reversed" if rev else "forward"
        out.append(("[1, L] %s" % tag, some, [rev] * len(some), [1] * len(some), [L[i] for i in some]))
        out.append(("[1, 1] %s" % tag, some, [rev] * len(some), [1] * len(some), [1] * len(some)))
        out.append(("[L, L] %s" % tag, some, [rev] * len(some), [L[i] for i in some], [L[i] for i in some]))
        # [k, k - 1] is empty: k = 1 (the only one an empty read allows), k in the middle, k = L + 1
        every = list(range(n))
        out.append(("[1, 0] %s" % tag, every, [rev] * n, [1] * n, [0] * n))
        out.append(("[k, k - 1] %s" % tag, every, [rev] * n, [L[i] // 2 + 1 for i in every], [L[i] // 2 for i in every]))
        out.append(("[L + 1, L] %s" % tag, every, [rev] * n, [L[i] + 1 for i in every], [L[i] for i in every]))
        two = [i for i in range(n) if L[i] >= 2]
        out.append(("[2, L] %s" % tag, two, [rev] * len(two), [2] * len(two), [L[i] for i in two]))
        out.append(("[1, L - 1] %s" % tag, two, [rev] * len(two), [1] * len(two), [L[i] - 1 for i in two]))
    # outputs of 127, 128, 129 and 300 bases cut out of the read of 301, on both strands, and mixed with empty outputs
    widths = (127, 128, 129, 300)
    out.append(("outputs of 127, 128, 129, 300 bases", [9] * 8 + [0, 9], [0, 1] * 4 + [0, 1],
                [2] * 8 + [1, 100], [w + 1 for w in widths for _ in (0, 1)] + [0, 99]))
    return out


# ---- subseq -------------------------------------------------------------------------------------------------------
def subseq(a, b, from_b, start, width):
    """The strings, or ("outside", r) for the lowest read r (0-based) whose range leaves its read.  A width <= 0
    gives the empty string, and its start is not looked at."""
    out = []
    for r in range(len(a)):
        src = b[r] if from_b is not None and from_b[r] else a[r]
        w, q0 = int(width[r]), int(start[r]) - 1
        if w <= 0:
            out.append(b"")
            continue
        if q0 < 0 or q0 + w > len(src):
            return "outside", r
        out.append(src[q0:q0 + w])
    return out


SUBSEQ_COUNTS = (255, 256, 257, 700)      # around k_subseq's 256 threads
WILD = (-2 ** 31, 2 ** 31 - 1, 0, -1)     # starts a width <= 0 must not look at


def subseq_batches(n, empty_last=False):
    """Two batches of n reads whose lengths differ read for read."""
    la = [(7 * r + 3) % 41 for r in range(n)]
    lb = [(5 * r + 11) % 23 + 1 for r in range(n)]
    if empty_last:
        la[-1] = 0
    else:
        la[-1] = max(la[-1], 1)
    rng = np.random.default_rng(200 + n)
    return [read(rng, k) for k in la], [read(rng, k) for k in lb]


def subseq_request(a, b, mixed):
    """(from_b, start, width) inside the reads: the kinds cycle over the reads."""
    n = len(a)
    from_b = [1 if mixed and r % 3 == 1 else 0 for r in range(n)]
    start, width = [], []
    for r in range(n):
        L = len(b[r] if from_b[r] else a[r])
        kind = r % 7 if L else r % 2
        if kind == 0:
            s, w = WILD[r % 4], 0               # width 0 with a wild start
        elif kind == 1:
            s, w = WILD[(r + 1) % 4], -(r % 5) - 1      # a negative width
        elif kind == 2:
            s, w = 1, L
        elif kind == 3:
            s, w = L, 1
        elif kind == 4:
            s, w = L // 2 + 1, L - L // 2       # start + width - 1 == L
        elif kind == 5:
            s, w = 1, 1
        else:
            s, w = (L + 1) // 2, 1
        start.append(s)
        width.append(w)
    return from_b, start, width


def subseq_cases():
    """(what, a, b, from_b, start, width): requests that are served."""
    out = []
    for n in SUBSEQ_COUNTS:
        for empty_last in (False, True):
            a, b = subseq_batches(n, empty_last)
            for mixed in (False, True):
                what = "%d reads, %s, last read %s" % (n, "two batches" if mixed else "one batch", "empty" if empty_last else "not empty")
                out.append((what, a, b if mixed else None) + subseq_request(a, b, mixed))
    return out


def subseq_refusals():
    """(what, a, b, from_b, start, width, read named, 0-based): every range outside its read is refused by the
    kernel's own test before a byte is read."""
    out = []
    a, b = subseq_batches(700)
    from_b, start, width = subseq_request(a, b, True)

    def bad(pairs, what, named):
        s, w = list(start), list(width)
        for r, (sr, wr) in pairs.items():
            s[r], w[r] = sr, wr
        out.append((what, a, b, from_b, s, w, named))
    L = lambda r: len(b[r] if from_b[r] else a[r])
    bad({400: (2, L(400))}, "start + width - 1 == L + 1", 400)
    bad({403: (L(403) + 1, 1)}, "start == L + 1, in the second batch", 403)
    bad({5: (0, 1)}, "start == 0", 5)
    bad({699: (-3, 2), 299: (1, L(299) + 1)}, "reads 700 and 300 in different workgroups", 299)
    bad({256: (1, L(256) + 1), 255: (0, 1)}, "reads 256 and 257 either side of a workgroup", 255)
    return out


# ---- scramble -----------------------------------------------------------------------------------------------------
M64 = (1 << 64) - 1
SEEDS = (0, 1, 1 << 32, 1 << 63, M64)
SCRAMBLE_LENGTHS = (0, 1, 2, 3, 64, 1000)
SCRAMBLE_COUNTS = (63, 64, 65, 129)       # around k_scramble's 64 threads
LONG_READ = 70000


def splitmix64(state):
    """(next state, output) of the splitmix64 generator."""
    state = (state + 0x9E3779B97F4A7C15) & M64
    z = state
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return state, z ^ (z >> 31)


def permutation(seed, r, length):
    """Where every position of read r comes from: Fisher-Yates from the end; the stream of read r is splitmix64 seeded
    with seed ^ (r + 1) * 0xD1342543DE82EF95, and position k swaps with ((next >> 32) * (k + 1)) >> 32."""
    perm = list(range(length))
    state = (seed ^ (((r + 1) * 0xD1342543DE82EF95) & M64)) & M64
    for k in range(length - 1, 0, -1):
        state, z = splitmix64(state)
        j = ((z >> 32) * (k + 1)) >> 32
        perm[k], perm[j] = perm[j], perm[k]
    return perm


def scramble(seqs, quals, seed):
    os_, oq = [], []
    for r, (s, q) in enumerate(zip(seqs, quals)):
        perm = permutation(seed, r, len(s))
        os_.append(bytes(s[p] for p in perm))
        oq.append(bytes(q[p] for p in perm))
    return os_, oq


def scramble_batch(n, empty_last=False, long_at=None, seed=300):
    """n reads of the SCRAMBLE_LENGTHS in turn, read `long_at` of LONG_READ bases."""
    lengths = [SCRAMBLE_LENGTHS[(r + 1) % len(SCRAMBLE_LENGTHS)] for r in range(n)]
    if long_at is not None:
        lengths[long_at] = LONG_READ
    lengths[-1] = 0 if empty_last else max(lengths[-1], 3)
    rng = np.random.default_rng(seed + n)
    return [read(rng, k, b"ACGTN") for k in lengths], [quality(k) for k in lengths]


@functools.lru_cache(maxsize=None)
def scramble_cases():
    """(what, seqs, quals, seed, restated seqs, restated quals), restated once.  The read of 70 000 bases is the last
    thread of the first workgroup, in one batch."""
    out = []
    for n in SCRAMBLE_COUNTS:
        for empty_last in (False, True):
            seqs, quals = scramble_batch(n, empty_last, 63 if n == 65 and not empty_last else None)
            for seed in SEEDS:
                what = "%d reads, last %s, seed %#x" % (n, "empty" if empty_last else "not empty", seed)
                out.append((what, seqs, quals, seed) + scramble(seqs, quals, seed))
    return out


def oracle_scramble(O, seqs, quals, seed):
    """oracle.scramble on bytes (its own front-end decodes the strings as text)."""
    import ctypes as C
    sb, so = O.pack(seqs)
    qb, _ = O.pack(quals)
    os_, oq = np.zeros_like(sb), np.zeros_like(qb)
    rc = O.lib().orc_scramble(sb.ctypes.data_as(C.c_void_p), qb.ctypes.data_as(C.c_void_p), so.ctypes.data_as(C.c_void_p),
                              C.c_int64(len(so) - 1), C.c_uint64(seed), os_.ctypes.data_as(C.c_void_p), oq.ctypes.data_as(C.c_void_p))
    assert rc == 0
    cut = lambda buf: [buf[so[i]:so[i + 1]].tobytes() for i in range(len(so) - 1)]
    return cut(os_), cut(oq)


# ---- strand choice ------------------------------------------------------------------------------------------------
# A result block of n alignments with S sections: double scores[n] | int32 starts[n] | int32 ends[n] |
# int32 section starts[max(S, 1)][n] | int32 section widths[max(S, 1)][n].  As host tuples:
# (scores, starts, ends, [section starts], [section widths]).
STRAND_COUNTS = (1, 255, 256, 257, 1000)      # around k_choose_strand's 256 threads
STRAND_SECTIONS = ((0, 0), (0, 3), (2, 1))
UP = float(np.nextafter(1.0, 2.0))
# (what, cs, ce, rs, re, reversed)
STRAND_SCORES = (
    ("both sums negative: a tie", -1.0, -2.0, -3.0, -4.0, False),
    ("-0.0 against 0.0", -0.0, -0.0, 0.0, 0.0, False),
    ("0.0 against -0.0", 0.0, 0.0, -0.0, -0.0, False),
    ("one ulp below", 1.0, -7.0, UP, -1.0, True),
    ("one ulp above", UP, -7.0, 1.0, -1.0, False),
    ("0.3 below 0.1 + 0.2 in fp64", 0.3, -1.0, 0.1, 0.2, True),
    ("0.1 + 0.2 above 0.3 in fp64", 0.1, 0.2, -1.0, 0.3, False),
    ("an exact tie", 3.0, 4.0, 4.0, 3.0, False),
    ("a tie of equal parts", 2.5, 2.5, 2.5, 2.5, False),
    ("the clamp decides", -5.0, 3.0, 2.0, 0.5, False),
    ("the clamp decides, other way", 2.0, 0.5, -5.0, 3.0, True),
    ("plainly reversed", 1.0, 1.0, 5.0, 5.0, True),
    ("plainly forward", 5.0, 5.0, 1.0, 1.0, False),
)


def strand_blocks(n, s1, s2):
    """The four blocks cs, ce, rs, re as flat uint8 arrays (what lies in HBM).  Read r has the scores of
    STRAND_SCORES[r % 13]; the int32 cell of (block, row, read) holds block << 28 | row << 20 | read, hidden section
    row of a block without sections included."""
    blocks = []
    for b, sections in enumerate((s1, s2, s1, s2)):
        rows = 2 + 2 * max(sections, 1)
        scores = np.array([STRAND_SCORES[r % len(STRAND_SCORES)][1 + b] for r in range(n)], np.float64)
        cells = ((b + 1) << 28) | (np.arange(rows, dtype=np.int32)[:, None] << 20) | np.arange(n, dtype=np.int32)[None, :]
        blocks.append(np.concatenate([scores.view(np.uint8), cells.astype(np.int32).reshape(-1).view(np.uint8)]))
    return blocks


def block_tuple(raw, n, sections, hidden=False):
    """A block's bytes as the host tuple; with `hidden` the section row of a block without sections is listed too."""
    scores = raw[:8 * n].view(np.float64)
    cells = raw[8 * n:].view(np.int32).reshape(2 + 2 * max(sections, 1), n)
    k = max(sections, 1)
    shown = k if hidden else sections
    return scores, cells[0], cells[1], [cells[2 + i] for i in range(shown)], [cells[2 + k + i] for i in range(shown)]


def choose_strand(cs, ce, rs, re):
    """(rows of adaptor 1, rows of adaptor 2, reversed) from four host tuples: read r is reversed iff
    max(cs, 0) + max(ce, 0) < max(rs, 0) + max(re, 0), strictly, in fp64; rows 1 come from rs or cs, rows 2 from re
    or ce."""
    fs = np.maximum(np.asarray(cs[0], np.float64), 0.0) + np.maximum(np.asarray(ce[0], np.float64), 0.0)
    bs = np.maximum(np.asarray(rs[0], np.float64), 0.0) + np.maximum(np.asarray(re[0], np.float64), 0.0)
    rev = fs < bs

    def pick(cur, rc):
        return (np.where(rev, rc[0], cur[0]), np.where(rev, rc[1], cur[1]), np.where(rev, rc[2], cur[2]),
                [np.where(rev, y, x) for x, y in zip(cur[3], rc[3])], [np.where(rev, y, x) for x, y in zip(cur[4], rc[4])])
    return pick(cs, rs), pick(ce, re), rev


def same_rows(got, want):
    """Two host tuples, scores compared by their bits."""
    return (np.array_equal(np.asarray(got[0]).view(np.int64), np.asarray(want[0]).view(np.int64))
            and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
            and len(got[3]) == len(want[3]) and len(got[4]) == len(want[4])
            and all(np.array_equal(x, y) for x, y in zip(got[3], want[3]))
            and all(np.array_equal(x, y) for x, y in zip(got[4], want[4])))


# ---- unmask -------------------------------------------------------------------------------------------------------
ENTRIES = "alignment and original sequences should have the same number of entries"
WIDTHS = "alignment strings should have the same length"
LONGER = "sequence in alignment string is longer than the original"
LENGTHS = "original sequence and that in the alignment string have different lengths"


def unmask(rows, originals):
    """The rows with every 'N' / 'n' replaced by the original's base at the same ungapped position, or the message of
    the first check that fails: entry counts, row widths, then row by row -- a masked base at or past the end of the
    original (LONGER) before a different number of bases (LENGTHS)."""
    if len(rows) != len(originals):
        return ENTRIES
    if any(len(row) != len(rows[0]) for row in rows):
        return WIDTHS
    out = []
    for row, orig in zip(rows, originals):
        c = np.frombuffer(row, np.uint8)
        base = c != ord("-")
        p = np.cumsum(base) - base              # bases in front of each column
        masked = (c == ord("N")) | (c == ord("n"))
        if (masked & (p >= len(orig))).any():
            return LONGER
        if int(base.sum()) != len(orig):
            return LENGTHS
        res = c.copy()
        res[masked] = np.frombuffer(orig, np.uint8)[p[masked]]
        out.append(res.tobytes())
    return out


UNMASK_WIDTHS = (1, 63, 64, 65, 127, 128, 129, 200)       # around k_unmask's steps of 64 columns


def mask_row(rng, width, gaps=0.15, masked=0.3, at=()):
    """(masked row, original): a random row with gaps, a share of its bases masked by 'N' / 'n', and the columns `at`
    (inside the row) made masked bases."""
    truth = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, width)]
    truth[rng.random(width) < gaps] = ord("-")
    at = [c for c in at if 0 <= c < width]
    truth[at] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, len(at))]
    row = truth.copy()
    hit = (rng.random(width) < masked) & (truth != ord("-"))
    hit[at] = True
    row[hit] = np.frombuffer(b"Nn", np.uint8)[rng.integers(0, 2, int(hit.sum()))]
    return row.tobytes(), truth[truth != ord("-")].tobytes()


def step_edges(width):
    """First and last column of every step of 64."""
    return sorted({c for c in list(range(0, width, 64)) + list(range(63, width, 64)) + [width - 1]})


def unmask_cases():
    """(what, rows, originals): served batches and refused ones; what the result is says unmask()."""
    rng = np.random.default_rng(400)
    out = []
    for w in UNMASK_WIDTHS:
        rows, origs = zip(*[mask_row(rng, w), mask_row(rng, w, at=step_edges(w)), mask_row(rng, w, gaps=0.0, masked=0.0, at=step_edges(w)),
                            (b"-" * w, b""), (b"N" * w, rng.choice(list(b"ACGT"), w).astype(np.uint8).tobytes()),
                            mask_row(rng, w, gaps=0.6)])
        out.append(("width %d" % w, list(rows), list(origs)))
    # the carry of the running count at exact multiples of 64: rows without a gap, masked at columns 64 and 128
    for w in (65, 128, 129, 200):
        row, orig = mask_row(rng, w, gaps=0.0, masked=0.0, at=[c for c in (64, 128) if c < w])
        out.append(("no gaps, width %d, masked at the first column of a step" % w, [row], [orig]))
    # refusals that only show past column 64
    for w in (129, 200):
        row, orig = mask_row(rng, w, gaps=0.2, masked=0.0)
        L = len(orig)
        assert L > 70
        cols = np.flatnonzero(np.frombuffer(row, np.uint8) != ord("-"))
        last = int(cols[-1])
        assert last >= 64
        tail = row[:last] + b"N" + row[last + 1:]                    # the masked base has the ungapped index L - 1
        out.append(("width %d: masked base at index L - 1" % w, [tail], [orig]))
        out.append(("width %d: masked base at index L" % w, [tail], [orig[:-1]]))
        out.append(("width %d: one base more than the original" % w, [row], [orig[:-1]]))
        out.append(("width %d: one base fewer than the original" % w, [row], [orig + b"A"]))
    # 64 bases in the first step, the masked base at column 64 is the 65th
    full = mask_row(rng, 64, gaps=0.0, masked=0.2)
    out.append(("width 65: masked base at index L == 64", [full[0] + b"N"], [full[1]]))
    out.append(("width 65: masked base at index L - 1 == 64", [full[0] + b"n"], [full[1] + b"G"]))
    # precedence between rows, and within one
    good = mask_row(rng, 70)
    short = (b"A" * 66 + b"-" * 4, b"A" * 65)                            # LENGTHS
    long_ = (b"A" * 66 + b"---N", b"A" * 66)                             # LONGER, at column 69
    out.append(("a row of different lengths before a longer one", *zip(good, short, long_)))
    out.append(("a longer row before one of different lengths", *zip(good, long_, short)))
    out.append(("within a row: masked base past the end and two bases too many", [b"A" * 66 + b"--NA"], [b"A" * 66]))
    out.append(("row widths differ", [b"ACGT", b"ACG"], [b"ACGT", b"ACG"]))
    out.append(("entry counts differ", [b"ACGT", b"ACGT"], [b"ACGT"]))
    out.append(("no rows", [], []))
    return [(what, list(rows), list(origs)) for what, rows, origs in out]


def unmask_many(nrows, bad_row=None, width=70):
    """(rows, originals): `nrows` rows of `width` columns; row `bad_row` has one base fewer than its original."""
    rng = np.random.default_rng(500)
    mat = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (nrows, width))]
    mat[rng.random((nrows, width)) < 0.1] = ord("-")
    masked = mat.copy()
    hit = (rng.random((nrows, width)) < 0.3) & (mat != ord("-"))
    masked[hit] = ord("N")
    masked[hit & (rng.random((nrows, width)) < 0.5)] = ord("n")
    rows = [masked[r].tobytes() for r in range(nrows)]
    origs = [mat[r][mat[r] != ord("-")].tobytes() for r in range(nrows)]
    if bad_row is not None:
        origs[bad_row] += b"T"
    return rows, origs


# ---- mask ---------------------------------------------------------------------------------------------------------
def mask_batch(total, nreads=40, seed=600):
    """(seqs, quals): `nreads` reads of unequal lengths with `total` bases together, qualities over all of '!'..'~'."""
    rng = np.random.default_rng(seed)
    cuts = np.sort(rng.choice(np.arange(1, total), nreads - 1, replace=False))
    lengths = np.diff(np.concatenate([[0], cuts, [total]]))
    seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, total)]
    qual = rng.integers(33, 127, total).astype(np.uint8)
    off = np.concatenate([[0], np.cumsum(lengths)])
    return ([seq[off[i]:off[i + 1]].tobytes() for i in range(nreads)], [qual[off[i]:off[i + 1]].tobytes() for i in range(nreads)])


def with_byte(strings, position, value):
    """The strings with the byte at `position` of their concatenation replaced; also the read it falls in."""
    out, at = list(strings), position
    for r, s in enumerate(out):
        if at < len(s):
            out[r] = s[:at] + bytes([value]) + s[at + 1:]
            return out, r
        at -= len(s)
    raise IndexError(position)
