"""tests/resident_cases.py, the restatement the device tests of the resident read helpers and of unmask_alignment
compare with, pinned without a GPU: against the CPU oracle and the host routes of the package where there is one,
against literal answers worked out by hand so that it cannot drift together with the code, and every builder's case
is shown to sit on the boundary it names."""
import numpy as np
import pytest

from tests import resident_cases as R


def _strings(ss):
    """A StringSet as a list of bytes."""
    return [ss.chars[ss.off[i]:ss.off[i + 1]].tobytes() for i in range(len(ss))]


# ---- complement ---------------------------------------------------------------------------------------------------
def test_complement_table():
    pairs = {"A": "T", "C": "G", "M": "K", "R": "Y", "V": "B", "H": "D"}
    want = list(range(256))
    for a, b in pairs.items():
        want[ord(a)], want[ord(b)] = ord(b), ord(a)
    assert R.COMPLEMENT.tolist() == want and R.COMPLEMENT.dtype == np.uint8
    assert (R.COMPLEMENT != np.arange(256)).sum() == 12
    assert (R.COMPLEMENT[R.COMPLEMENT] == np.arange(256)).all()
    assert R.revcomp(b"AC+.acgtNU-WSB") == b"VSW-UNtgca.+GT"
    assert R.revcomp(b"ACGTMRWSYKVHDBN") == b"NVHDBMRSWYKACGT"


def test_the_package_complements_as_the_restatement():
    from sarlacc_amd import generics, mock
    assert np.array_equal(mock._COMP, R.COMPLEMENT)
    assert mock.revcomp("AC+.acgtNU-WSB") == "VSW-UNtgca.+GT"
    front, back = generics._get_front_and_back(generics.Reads(["AC+.acgtNU-WSB"], ["0123456789abcd"]), 100)
    assert back.seq.to_strings() == ["VSW-UNtgca.+GT"] and back.qual.to_strings() == ["dcba9876543210"]
    assert front.seq.to_strings() == ["AC+.acgtNU-WSB"]
    assert 0 not in back.seq.chars[:14]


# ---- windows ------------------------------------------------------------------------------------------------------
def test_windows_known_answers():
    (fs, fq), (bs, bq) = R.windows([b"AACGTTTV", b"AC", b""], [b"01234567", b"ab", b""], 3)
    assert fs == [b"AAC", b"AC", b""] and fq == [b"012", b"ab", b""]
    assert bs == [b"BAA", b"GT", b""] and bq == [b"765", b"ba", b""]
    (fs, fq), (bs, bq) = R.windows([b"AACGTTTV"], [b"01234567"], 0)
    assert fs == fq == bs == bq == [b""]


def test_window_cases_sit_on_their_boundaries():
    cases = R.window_cases()
    lengths = {len(s) for _, seqs, _, _ in cases for s in seqs}
    assert lengths == set(R.WINDOW_LENGTHS)
    for tol in (10, 64):     # a read one below, at and one above the tolerance
        assert {tol - 1, tol, tol + 1} <= lengths and tol in R.WINDOW_TOLERANCES
    assert {len(seqs[-1]) > 0 for _, seqs, _, _ in cases if seqs} == {True, False}
    assert any(not seqs for _, seqs, _, _ in cases)
    assert max(R.WINDOW_TOLERANCES) > max(lengths)
    _, seqs, quals = R.complement_case()
    assert sorted(seqs[1]) == list(range(256)) and quals[1] == bytes(range(256))


def test_windows_equal_the_host_route():
    from sarlacc_amd import generics
    cases = R.window_cases() + [R.complement_case() + (tol,) for tol in (0, 100, 256, 1000)]
    for what, seqs, quals, tol in cases:
        front, back = generics._get_front_and_back(generics.Reads(seqs, quals), tol)
        (fs, fq), (bs, bq) = R.windows(seqs, quals, tol)
        assert _strings(front.seq) == fs and _strings(front.qual) == fq, what
        assert _strings(back.seq) == bs and _strings(back.qual) == bq, what


# ---- realize ------------------------------------------------------------------------------------------------------
def test_realize_known_answers():
    seqs, quals = [b"AACGT", b"", b"GV"], [b"01234", b"", b"xy"]
    assert R.realize(seqs, quals, [2, 0, 1, 0], [1, 1, 1, 0]) == ([b"BC", b"ACGTT", b"", b"AACGT"], [b"yx", b"43210", b"", b"01234"])
    # on a reversed read [2, L] drops the original's last base and [1, L - 1] its first
    assert R.realize(seqs, quals, [0, 0], [1, 1], [2, 1], [5, 4]) == ([b"CGTT", b"ACGT"], [b"3210", b"4321"])
    assert R.realize(seqs, quals, [0, 0], [1, 1], [2, 1], [5, 4])[0] == [R.revcomp(b"AACG"), R.revcomp(b"ACGT")]
    assert R.realize(seqs, quals, [0, 0, 0, 0], [0, 0, 0, 1], [1, 5, 3, 6], [1, 5, 2, 5]) == ([b"A", b"T", b"", b""], [b"0", b"4", b"", b""])


def test_realize_cases_sit_on_their_boundaries():
    seqs, quals = R.batch(R.REALIZE_LENGTHS, 102)
    widths = set()
    kinds = set()
    for what, idx, rev, ts, te in R.realize_cases():
        assert len(idx) == len(rev) and all(0 <= i < len(seqs) for i in idx)
        got = R.realize(seqs, quals, idx, rev, ts, te)
        widths |= {len(s) for s in got[0]}
        kinds.add("empty" if not idx else "repeated" if len(set(idx)) < len(idx) else "subset" if len(idx) < len(seqs) else "all")
        if ts is not None:
            assert all(len(s) == max(b - a + 1, 0) for s, a, b in zip(got[0], ts, te)), what
        if what.startswith("[k, k - 1]") or what.startswith("[1, 0]") or what.startswith("[L + 1, L]"):
            assert all(s == b"" for s in got[0]), what
    assert {0, 127, 128, 129, 300} <= widths and kinds == {"empty", "repeated", "subset", "all"}
    assert any(0 < sum(rev) < len(rev) for _, _, rev, _, _ in R.realize_cases())


# ---- subseq -------------------------------------------------------------------------------------------------------
def test_subseq_known_answers():
    a, b = [b"ACGTAC", b"TTT", b""], [b"GG", b"CAGT", b"AAAAA"]
    assert R.subseq(a, None, None, [1, 3, 9], [6, 1, 0]) == [b"ACGTAC", b"T", b""]
    assert R.subseq(a, b, [0, 1, 1], [6, 2, 5], [1, 3, 1]) == [b"C", b"AGT", b"A"]
    assert R.subseq(a, b, [0, 1, 1], [-7, 2 ** 31 - 1, 0], [0, -1, -9]) == [b"", b"", b""]
    assert R.subseq(a, None, None, [1, 3, 1], [6, 2, 0]) == ("outside", 1)        # start + width - 1 == L + 1
    assert R.subseq(a, None, None, [1, 0, 1], [6, 1, 1]) == ("outside", 1)        # start 0, reported before read 3
    assert R.subseq(a, b, [0, 1, 0], [7, 4, 1], [1, 1, 1]) == ("outside", 0)


def test_subseq_cases_sit_on_their_boundaries():
    cases = R.subseq_cases()
    assert {len(a) for _, a, *_ in cases} == set(R.SUBSEQ_COUNTS)
    ends = set()
    for what, a, b, from_b, start, width in cases:
        got = R.subseq(a, b, from_b if b is not None else None, start, width)
        assert isinstance(got, list), what
        src = [b[r] if b is not None and from_b[r] else a[r] for r in range(len(a))]
        ends |= {"whole" for r, s in enumerate(src) if s and (start[r], width[r]) == (1, len(s))}
        ends |= {"last base" for r, s in enumerate(src) if s and (start[r], width[r]) == (len(s), 1)}
        ends |= {"ends at L" for r, s in enumerate(src) if width[r] > 0 and start[r] > 1 and start[r] + width[r] - 1 == len(s)}
        ends |= {"wild" for r in range(len(a)) if width[r] <= 0 and not 1 <= start[r] <= len(src[r])}
        ends |= {"negative" for w in width if w < 0}
        if b is not None:
            assert 0 < sum(from_b) < len(a) and any(len(x) != len(y) for x, y in zip(a, b))
        else:
            assert not any(from_b)
    assert ends == {"whole", "last base", "ends at L", "wild", "negative"}
    for what, a, b, from_b, start, width, named in R.subseq_refusals():
        assert R.subseq(a, b, from_b, start, width) == ("outside", named), what
        bad = [r for r in range(len(a)) if width[r] > 0
               and not (1 <= start[r] and start[r] + width[r] - 1 <= len(b[r] if from_b[r] else a[r]))]
        assert bad[0] == named, what
        if "different workgroups" in what:
            assert bad == [299, 699] and bad[0] // 256 != bad[1] // 256
        if "L + 1" in what and "start +" in what:
            r = named
            assert start[r] + width[r] - 1 == len(b[r] if from_b[r] else a[r]) + 1


# ---- scramble -----------------------------------------------------------------------------------------------------
def test_splitmix64_known_answers():
    # the first outputs of splitmix64 from state 0, as published with the generator
    state, out = 0, []
    for _ in range(3):
        state, z = R.splitmix64(state)
        out.append(z)
    assert out == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    assert R.permutation(5, 0, 0) == [] and R.permutation(5, 3, 1) == [0]
    # two positions: one draw; the partner of position 1 is (high half * 2) >> 32, the top bit of the output
    for seed in R.SEEDS:
        for r in (0, 1, 70):
            _, z = R.splitmix64(seed ^ (((r + 1) * 0xD1342543DE82EF95) & R.M64))
            assert R.permutation(seed, r, 2) == ([0, 1] if z >> 63 else [1, 0])


def test_scramble_equals_the_oracle(oracle):
    rng = np.random.default_rng(7)
    lengths = (0, 1, 2, 3, 64, 1000)
    seqs = [R.read(rng, n) for n in lengths]
    quals = [R.quality(n) for n in lengths]
    for seed in R.SEEDS:
        got = R.scramble(seqs, quals, seed)
        assert got == R.oracle_scramble(oracle, seqs, quals, seed), seed
        text = [R.text_quality(n) for n in lengths]
        want = oracle.scramble([s.decode() for s in seqs], [q.decode() for q in text], seed)
        assert [s.decode() for s in got[0]] == want[0] and [q.decode() for q in R.scramble(seqs, text, seed)[1]] == want[1]
    assert len({tuple(R.permutation(seed, 4, 64)) for seed in R.SEEDS}) == len(R.SEEDS)


def test_scramble_cases_sit_on_their_boundaries(oracle):
    cases = R.scramble_cases()
    assert {len(seqs) for _, seqs, *_ in cases} == set(R.SCRAMBLE_COUNTS)
    assert {seed for _, _, _, seed, _, _ in cases} == {0, 1, 2 ** 32, 2 ** 63, 2 ** 64 - 1}
    lengths = {len(s) for _, seqs, *_ in cases for s in seqs}
    assert lengths == set(R.SCRAMBLE_LENGTHS) | {R.LONG_READ}
    assert {len(seqs[-1]) > 0 for _, seqs, *_ in cases} == {True, False}
    for what, seqs, quals, seed, ws, wq in cases:
        for s, q, a, b in zip(seqs, quals, ws, wq):
            assert sorted(a) == sorted(s) and len(a) == len(b) == len(s), what
        assert all(len(s) < 4 or a != s for s, a in zip(seqs, ws) if len(set(s)) > 1 and len(s) >= 64), what
        if len(seqs) == 65 and seed in (0, 2 ** 64 - 1):      # the long read too, once per end of the seed range
            assert (ws, wq) == R.oracle_scramble(oracle, seqs, quals, seed), what


# ---- strand choice ------------------------------------------------------------------------------------------------
def test_strand_scores_known_answers():
    from sarlacc_amd import generics
    cs, ce, rs, re = (np.array([row[k] for row in R.STRAND_SCORES]) for k in (1, 2, 3, 4))
    want = [row[5] for row in R.STRAND_SCORES]
    assert want == [False, False, False, True, False, True, False, False, False, False, True, True, False]
    blocks = [(x, np.zeros(len(x), np.int32), np.zeros(len(x), np.int32), [], []) for x in (cs, ce, rs, re)]
    assert R.choose_strand(*blocks)[2].tolist() == want
    rev, best = generics._resolve_strand(cs, ce, rs, re)
    assert rev.tolist() == want
    assert (cs + ce < rs + re).tolist() != want        # without the clamp the rule differs
    clamp = [row[0] for row in R.STRAND_SCORES].index("the clamp decides")
    assert R.STRAND_SCORES[clamp][1:5] == (-5.0, 3.0, 2.0, 0.5) and not want[clamp] and cs[clamp] + ce[clamp] < rs[clamp] + re[clamp]
    assert np.float32(0.3) == np.float32(0.1) + np.float32(0.2) and 0.3 < 0.1 + 0.2     # what fp32 would tie


def test_strand_blocks_and_choice():
    from sarlacc_amd import generics
    for n in R.STRAND_COUNTS:
        for s1, s2 in R.STRAND_SECTIONS:
            raw = R.strand_blocks(n, s1, s2)
            assert [b.size for b in raw] == [16 * n + 8 * n * max(s, 1) for s in (s1, s2, s1, s2)]
            cells = np.concatenate([b[8 * n:].view(np.int32) for b in raw])
            assert np.unique(cells).size == cells.size                 # unique to (block, row, read)
            cs, ce, rs, re = (R.block_tuple(b, n, s) for b, s in zip(raw, (s1, s2, s1, s2)))
            assert len(cs[3]) == len(cs[4]) == s1 and len(ce[3]) == s2
            assert len(R.block_tuple(raw[0], n, s1, hidden=True)[3]) == max(s1, 1)
            rows1, rows2, rev = R.choose_strand(cs, ce, rs, re)
            assert rev.tolist() == generics._resolve_strand(cs[0], ce[0], rs[0], re[0])[0].tolist()
            assert rev.tolist() == [R.STRAND_SCORES[r % len(R.STRAND_SCORES)][5] for r in range(n)]
            for rows, cur, rc in ((rows1, cs, rs), (rows2, ce, re)):
                for r in range(0, n, 7):
                    src = rc if rev[r] else cur
                    assert rows[0][r].tobytes() == src[0][r].tobytes() and rows[1][r] == src[1][r] and rows[2][r] == src[2][r]
                    assert all(x[r] == y[r] for x, y in zip(rows[3] + rows[4], src[3] + src[4]))
    # a literal: two reads, one section
    cur = (np.array([1.0, 9.0]), np.array([1, 2], np.int32), np.array([3, 4], np.int32), [np.array([5, 6], np.int32)], [np.array([7, 8], np.int32)])
    rc = (np.array([2.0, 0.0]), np.array([11, 12], np.int32), np.array([13, 14], np.int32), [np.array([15, 16], np.int32)], [np.array([17, 18], np.int32)])
    zero = (np.zeros(2), np.zeros(2, np.int32), np.zeros(2, np.int32), [], [])
    rows1, rows2, rev = R.choose_strand(cur, zero, rc, zero)
    assert rev.tolist() == [True, False]
    assert R.same_rows(rows1, (np.array([2.0, 9.0]), [11, 2], [13, 4], [[15, 6]], [[17, 8]])) and R.same_rows(rows2, zero)


# ---- unmask -------------------------------------------------------------------------------------------------------
def test_unmask_known_answers():
    assert R.unmask([b"AN-nT", b"--N--"], [b"ACGT", b"G"]) == [b"AC-GT", b"--G--"]
    assert R.unmask([b"-----"], [b""]) == [b"-----"] and R.unmask([], []) == []
    assert R.unmask([b"AA-AA"], [b"AAA"]) == R.LENGTHS and R.unmask([b"AA-A"], [b"AAAA"]) == R.LENGTHS
    assert R.unmask([b"AAAN"], [b"AAA"]) == R.LONGER and R.unmask([b"AAAN"], [b"AAAC"]) == [b"AAAC"]
    assert R.unmask([b"AANA"], [b"AA"]) == R.LONGER                  # both hold: the masked base past the end wins
    assert R.unmask([b"AAAA", b"NNNN", b"AA-A"], [b"AAAA", b"GG", b"A"]) == R.LONGER
    assert R.unmask([b"AAAA", b"AA-A", b"NNNN"], [b"AAAA", b"A", b"GG"]) == R.LENGTHS
    assert R.unmask([b"AAAA", b"GGG"], [b"AAAA", b"GGG"]) == R.WIDTHS and R.unmask([b"A", b"C"], [b"A"]) == R.ENTRIES


def _oracle_unmask(oracle, rows, origs):
    try:
        return [s.encode() for s in oracle.unmask_alignment([r.decode() for r in rows], [o.decode() for o in origs])]
    except oracle.OracleError as e:
        return str(e)


def test_unmask_equals_the_oracle(oracle):
    results = {}
    for what, rows, origs in R.unmask_cases():
        got = R.unmask(rows, origs)
        assert got == _oracle_unmask(oracle, rows, origs), what
        results[what] = got
    for bad in (None, 0, 57, 99):
        rows, origs = R.unmask_many(100, bad)
        got = R.unmask(rows, origs)
        assert got == _oracle_unmask(oracle, rows, origs) and isinstance(got, str) == (bad is not None)
    # every case gives what its name says
    for what, got in results.items():
        if "index L - 1" in what or what.startswith("width ") and ":" not in what or what.startswith("no gaps"):
            assert isinstance(got, list), what
        if "masked base at index L" in what and "L - 1" not in what:
            assert got == R.LONGER, what
        if "than the original" in what:
            assert got == R.LENGTHS, what
    assert results["a row of different lengths before a longer one"] == R.LENGTHS
    assert results["a longer row before one of different lengths"] == R.LONGER
    assert results["within a row: masked base past the end and two bases too many"] == R.LONGER
    assert results["row widths differ"] == R.WIDTHS and results["entry counts differ"] == R.ENTRIES and results["no rows"] == []


def test_unmask_cases_sit_on_their_boundaries():
    cases = {what: (rows, origs) for what, rows, origs in R.unmask_cases()}
    assert len(cases) == len(R.unmask_cases())
    for w in R.UNMASK_WIDTHS:
        rows, origs = cases["width %d" % w]
        assert {len(r) for r in rows} == {w}
        assert all(rows[1][c] in b"Nn" and rows[2][c] in b"Nn" for c in R.step_edges(w))
        assert b"-" not in rows[2] and rows[3] == b"-" * w and origs[3] == b"" and rows[4] == b"N" * w and len(origs[4]) == w
    assert R.step_edges(129) == [0, 63, 64, 127, 128] and R.step_edges(64) == [0, 63] and R.step_edges(1) == [0]
    assert 128 in R.UNMASK_WIDTHS and len(cases["width 128"][0][0]) == 128
    for w in (129, 200):
        for name, kept in (("width %d: masked base at index L - 1" % w, 0), ("width %d: masked base at index L" % w, 1)):
            (row,), (orig,) = cases[name]
            col = max(c for c in range(w) if row[c] != ord("-"))
            assert row[col] == ord("N") and col >= 64 and b"N" not in row[:col] and b"n" not in row
            assert sum(ch != ord("-") for ch in row[:col]) == len(orig) - 1 + kept        # its ungapped index: L - 1, or L
            assert sum(ch != ord("-") for ch in row[:64]) < len(orig)                     # the first step alone shows nothing
        for name, d in (("width %d: one base more than the original" % w, 1), ("width %d: one base fewer than the original" % w, -1)):
            (row,), (orig,) = cases[name]
            assert sum(ch != ord("-") for ch in row) == len(orig) + d and sum(ch != ord("-") for ch in row[:64]) < len(orig)
    (row,), (orig,) = cases["width 65: masked base at index L == 64"]
    assert len(row) == 65 and b"-" not in row and row[64] == ord("N") and len(orig) == 64
    for w in (65, 128, 129, 200):
        (row,), (orig,) = cases["no gaps, width %d, masked at the first column of a step" % w]
        assert b"-" not in row and [c for c in range(w) if row[c] in b"Nn"] == [c for c in (64, 128) if c < w] and len(orig) == w


# ---- mask ---------------------------------------------------------------------------------------------------------
def test_mask_batch_and_with_byte():
    seqs, quals = R.mask_batch(5000, 40)
    assert len(seqs) == 40 and sum(map(len, seqs)) == 5000 and [len(s) for s in seqs] == [len(q) for q in quals]
    assert min(map(len, seqs)) > 0 and min(min(q) for q in quals) == 33 and max(max(q) for q in quals) == 126
    changed, r = R.with_byte(quals, 4321, 32)
    flat = b"".join(changed)
    assert flat[4321] == 32 and flat[:4321] + flat[4322:] == b"".join(quals)[:4321] + b"".join(quals)[4322:]
    assert sum(map(len, quals[:r])) <= 4321 < sum(map(len, quals[:r + 1])) and [len(q) for q in changed] == [len(q) for q in quals]
