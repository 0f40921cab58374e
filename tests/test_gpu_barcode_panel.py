"""A whole barcode panel in one call (sarlacc_barcode_panel / sarlacc_dev_barcode_panel, align_panel.hip) against the CPU
oracle: every score of the matrix is oracle.barcode_align of that barcode alone, and best / score / next best are the loop
of R/barcodeAlign.R:20-37 restated in numpy over those scores.  Scores are compared on their bits; where the expected
value is NaN (-inf minus -inf in the generic's gap) the NaN positions are compared.
"""
import numpy as np
import pytest

from tests.encodings import BY_NAME, TABLE_IDS, TABLES, draw_quals

pytestmark = pytest.mark.gpu

PENALTIES = [(5, 1), (0, 1), (2.5, 0.5), (5, 0), (-1, 2)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def fold(matrix):
    """R/barcodeAlign.R:20-37 on a (barcodes, reads) score matrix: (best, 1-based and 0 for none; score; next best)."""
    n = matrix.shape[1]
    best, cur, nxt = np.zeros(n, np.int32), np.full(n, -np.inf), np.full(n, -np.inf)
    for b, s in enumerate(matrix):
        keep = s > cur
        second = ~keep & (s > nxt)
        best[keep] = b + 1
        nxt[keep] = cur[keep]
        cur[keep] = s[keep]
        nxt[second] = s[second]
    return best, cur, nxt


def expect(oracle, oenc, seqs, quals, barcodes, go, ge):
    m = np.zeros((len(barcodes), len(seqs)))
    for b, bc in enumerate(barcodes):
        m[b] = oracle.barcode_align(seqs, quals, oenc, go, ge, bc)
    return (m,) + fold(m)


def same(got, want, what=""):
    """(best, score, next[, matrix]) against (matrix, best, score, next)"""
    m, best, cur, nxt = want
    assert np.array_equal(got[0], best), what + " best barcode"
    assert got[0].dtype == np.int32
    assert np.array_equal(bits(got[1]), bits(cur)), what + " score"
    assert np.array_equal(bits(got[2]), bits(nxt)), what + " next best"
    if len(got) > 3:
        assert got[3].shape == m.shape and np.array_equal(bits(got[3]), bits(m)), what + " score matrix"


def counters():
    from sarlacc_amd import _lib
    return {k: _lib.stage_count("panel_" + k) for k in ("fused_barcodes", "single_barcodes", "launches")}


def resident(seqs, quals, enc=None):
    from sarlacc_amd import generics
    from sarlacc_amd.resident import DeviceReads
    return DeviceReads.upload(generics.Reads(seqs, quals, encoding=enc))


# ---- the mixed panel of tests 1, 2 and 5 ---------------------------------------------------------------------------
def _rand(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(list(alphabet), n))


def _mixed():
    """203 reads (three wavefronts and a tail of 11) of 0 to 40 bases, several empty, some N and X; a panel of 0, 1, 7, 8, 9,
    16, 31, 32, 33, 64 and 1 030 columns in an order that interleaves short and long barcodes, with a copy of the 7-column
    one after the 33-column one and a copy of the 64-column one; the 8- and 16-column barcodes hold N, R and V."""
    rng = np.random.default_rng(2024)
    lengths = rng.integers(0, 41, 203)
    lengths[[0, 5, 63, 64, 130, 202]] = 0
    lengths[[1, 65]] = 40
    seqs = [_rand(rng, int(n), "ACGTACGTACGTACGTNX") for n in lengths]
    quals = ["".join(chr(c) for c in rng.integers(33, 127, int(n))) for n in lengths]
    b = {n: _rand(rng, n) for n in (1, 7, 9, 31, 32, 33, 64, 1030)}
    b[8] = "ACNGRTVA"
    b[16] = "NACGTRRGTVACNTGA"
    # reads that match a short barcode: ties between the copies and a clear best
    seqs[2], seqs[66] = b[7], b[7] + "A"
    quals[2], quals[66] = "I" * 7, "5" * 8
    panel = [b[7], "", b[33], b[7], b[1], b[64], b[8], b[9], b[1030], b[16], b[31], b[64], b[32]]
    assert [len(x) for x in panel] == [7, 0, 33, 7, 1, 64, 8, 9, 1030, 16, 31, 64, 32]
    return seqs, quals, panel


_cache = {}


def mixed(oracle, oenc, go, ge):
    """The inputs and the oracle's (matrix, best, score, next) for a pair of penalties, computed once."""
    if "inputs" not in _cache:
        _cache["inputs"] = _mixed()
    seqs, quals, panel = _cache["inputs"]
    if (go, ge) not in _cache:
        _cache[(go, ge)] = expect(oracle, oenc, seqs, quals, panel, go, ge)
    return seqs, quals, panel, _cache[(go, ge)]


@pytest.mark.parametrize("go,ge", PENALTIES)
def test_matrix_and_reduction(oracle, oenc, go, ge):
    seqs, quals, panel, want = mixed(oracle, oenc, go, ge)
    assert (want[1][[2, 66]] == 1).all(), "the earlier copy of a duplicate wins its ties"
    got = resident(seqs, quals).barcode_panel(panel, go, ge, all_scores=True)
    same(got, want)
    c = counters()
    assert c["fused_barcodes"] == sum(1 <= len(b) <= 32 for b in panel) == 8
    assert c["single_barcodes"] == 5
    assert c["launches"] < len(panel)


@pytest.mark.parametrize("go,ge", PENALTIES)
def test_fallback_equals_fused(oracle, oenc, go, ge):
    from sarlacc_amd import calls
    seqs, quals, panel, want = mixed(oracle, oenc, go, ge)
    calls.set_option("align_panel", -1)
    try:
        got = resident(seqs, quals).barcode_panel(panel, go, ge, all_scores=True)
        c = counters()
    finally:
        calls.set_option("align_panel", 0)
    same(got, want)
    assert c["fused_barcodes"] == 0 and c["single_barcodes"] == len(panel) == c["launches"]


# ---- every encoding ------------------------------------------------------------------------------------------------
ENC_PANEL = ["ACGTTGCAAGCT", "ACGTNGCAAGCA", "ACGTTGCAAGCTACGTACGA", "ACGTTGCAAGCTACGTACGAGGATCCATTGCA"]


@pytest.mark.parametrize("table", TABLES, ids=TABLE_IDS)
def test_every_encoding(oracle, table):
    """70 reads with qualities drawn over the whole table, 4 barcodes of 12, 12, 20 and 32 columns (one with N), penalties
    (5, 1).

    The issue asked for -inf scores from `zero_tail` and `one_head` at these penalties.  There are none: a global
    alignment can always pay for gaps alone, so with finite penalties every cell is finite whatever the table holds
    (checked on the oracle below: no expected score is infinite).  The -inf costs of the two tables reach a score only
    where no gap can be paid for, so that part is tested with an infinite gap opening penalty in
    test_minus_infinity_scores."""
    assert [len(b) for b in ENC_PANEL] == [12, 12, 20, 32]
    rng = np.random.default_rng(77)
    lengths = rng.integers(0, 31, 70)
    seqs = [_rand(rng, int(n), "ACGTACGTACGTN") for n in lengths]
    quals = draw_quals(table, lengths, seed=78)
    want = expect(oracle, table.oenc, seqs, quals, ENC_PANEL, 5, 1)
    assert np.isfinite(want[0]).all()
    same(resident(seqs, quals, table.enc).barcode_panel(ENC_PANEL, 5, 1, all_scores=True), want, table.name)
    assert counters()["fused_barcodes"] == 4 and counters()["launches"] == 1


@pytest.mark.parametrize("name", ["zero_tail", "one_head"])
def test_minus_infinity_scores(oracle, name):
    """-inf costs (a mismatch at error probability 0, a match at error probability 1) with gapopen = inf, where no path
    can avoid them through a gap.  Under `one_head` a read made only of the first quality name scores -inf against every
    barcode: no best barcode, score -inf, and the generic's gap is NaN."""
    from sarlacc_amd import generics
    table = BY_NAME[name]
    first, last = bytes([table.names[0]]), bytes([table.names[-1]])
    seqs = ["ACGTTGCAAGCT", "ACGTTGCAAGCT", "ACGTAGCAAGCA", "ACGTTGCAAGCTACGTACGA", ""]
    quals = [first * 12, last * 12, last * 12, last * 20, b""]
    go, ge = float("inf"), 1
    want = expect(oracle, table.oenc, seqs, quals, ENC_PANEL, go, ge)
    assert np.isneginf(want[0]).any() and np.isfinite(want[0]).any()
    got = resident(seqs, quals, table.enc).barcode_panel(ENC_PANEL, go, ge, all_scores=True)
    same(got, want, name)
    out = generics.barcodeAlign(generics.Reads(seqs, quals, encoding=table.enc), ENC_PANEL, gapOpening=go, gapExtension=ge)
    assert np.array_equal(out["barcode"], np.where(want[1] == 0, -1, want[1]))
    assert np.array_equal(bits(out["score"]), bits(want[2]))
    gap = want[2] - want[3]
    assert np.array_equal(np.isnan(out["gap"]), np.isnan(gap))
    assert np.array_equal(bits(out["gap"][~np.isnan(gap)]), bits(gap[~np.isnan(gap)]))
    if name == "one_head":
        assert np.isneginf(want[0][:, 0]).all(), "the read of first names scores -inf against every barcode"
        assert got[0][0] == 0 and np.isneginf(got[1][0]) and np.isneginf(got[2][0])
        assert out["barcode"][0] == -1 and np.isneginf(out["score"][0]) and np.isnan(out["gap"][0])


# ---- degenerate panels ---------------------------------------------------------------------------------------------
def test_degenerate_panels(oracle, oenc, enc):
    from sarlacc_amd import calls, generics
    seqs, quals = ["ACGTACGTAC", "", "TTGCA"], ["IIIIIIIIII", "", "55555"]
    dev = resident(seqs, quals)
    # no barcode
    for got in (dev.barcode_panel([], 5, 1, all_scores=True), calls.barcode_panel(seqs, quals, enc, 5, 1, [], all_scores=True)):
        assert got[0].tolist() == [0, 0, 0] and np.isneginf(got[1]).all() and np.isneginf(got[2]).all() and got[3].shape == (0, 3)
    out = generics.barcodeAlign(generics.Reads(seqs, quals), [])
    assert out["barcode"].tolist() == [-1, -1, -1] and np.isneginf(out["score"]).all() and np.isnan(out["gap"]).all()
    # one barcode: nothing is next best
    want = expect(oracle, oenc, seqs, quals, ["ACGTACGTAC"], 5, 1)
    same(dev.barcode_panel(["ACGTACGTAC"], 5, 1, all_scores=True), want)
    out = generics.barcodeAlign(generics.Reads(seqs, quals), ["ACGTACGTAC"])
    assert out["barcode"].tolist() == [1, 1, 1] and np.array_equal(bits(out["score"]), bits(want[2]))
    assert (out["gap"] == np.inf).all()
    # no read
    for got in (resident([], []).barcode_panel(["ACGT", "TTTT"], 5, 1, all_scores=True),
                calls.barcode_panel([], [], enc, 5, 1, ["ACGT", "TTTT"], all_scores=True)):
        assert [x.size for x in got] == [0, 0, 0, 0] and got[3].shape == (2, 0)
    # every read empty
    panel = ["ACGT", "", "ACGTTGCAAGCTACGTACGAGGATCCATTGCAG", "AC"]
    want = expect(oracle, oenc, ["", "", ""], ["", "", ""], panel, 5, 1)
    same(resident(["", "", ""], ["", "", ""]).barcode_panel(panel, 5, 1, all_scores=True), want)
    assert want[1].tolist() == [2, 2, 2]


# ---- host-pointer entry --------------------------------------------------------------------------------------------
def test_host_entry_equals_resident(oracle, oenc, enc):
    from sarlacc_amd import calls
    seqs, quals, panel, (m, _, _, _) = mixed(oracle, oenc, 5, 1)
    seqs, quals = seqs[:100], quals[:100]
    want = (m[:, :100],) + fold(m[:, :100])
    host = calls.barcode_panel(seqs, quals, enc, 5, 1, panel, all_scores=True)
    same(host, want, "host entry")
    same(resident(seqs, quals).barcode_panel(panel, 5, 1, all_scores=True), want, "resident entry")
    same(calls.barcode_panel(seqs, quals, enc, 5, 1, panel), want, "host entry without the matrix")


# ---- errors --------------------------------------------------------------------------------------------------------
def _raised(fn):
    from sarlacc_amd import SarlaccError
    with pytest.raises(SarlaccError) as e:
        fn()
    return str(e.value)


def test_errors(enc):
    from sarlacc_amd import calls
    seqs = ["ACGTACGT", "", "TTGCATGCA", "ACGT", "GGGTTTAAAC", "ACGTAC"]
    quals = ["I" * len(s) for s in seqs]
    panel = ["ACGTACGT", "TTGCATGC", "ACGXACGT", "ACGTTTTT", "GGGTTTAA"]

    def both(s, q, p):
        return (_raised(lambda: calls.barcode_panel(s, q, enc, 5, 1, p)), _raised(lambda: resident(s, q).barcode_panel(p, 5, 1)))

    # an unrecognised character in barcode 3 of 5
    assert both(seqs, quals, panel) == ("unrecognized base in reference sequence",) * 2
    # ... and a quality below the table's first name: barcode 1 meets it first
    low = list(quals)
    low[2] = "IIII IIII"
    assert both(seqs, low, panel) == ("quality cannot be lower than smallest encoded value",) * 2
    # barcode 1 empty (it meets no quality), barcode 2 with the bad character as its first column: what the loop raises
    low0 = ["II II II"] + quals[1:]
    panel2 = ["", "XCGTACGT", "ACGTACGT"]
    for s, q in ((seqs, low0), (seqs, low)):
        def loop():
            for bc in panel2:
                calls.barcode_align(s, q, enc, 5, 1, bc)
        msg = _raised(loop)
        assert msg in ("unrecognized base in reference sequence", "quality cannot be lower than smallest encoded value")
        assert both(s, q, panel2) == (msg, msg)
    # an empty barcode alone meets no quality error
    assert calls.barcode_panel(seqs, low, enc, 5, 1, [""])[0].tolist() == [1] * 6
    # a length mismatch through the host entry
    short = list(quals)
    short[3] = "III"
    assert _raised(lambda: calls.barcode_panel(seqs, short, enc, 5, 1, panel[:2])) == "sequence and quality strings should have the same length"


# ---- more reads than one resident grid -----------------------------------------------------------------------------
def test_more_reads_than_the_grid(oracle, oenc):
    """n = 40 000 reads of 10 to 20 bases with align_waves_per_cu = 1, which the kernel honours: 256 CUs then hold 64
    workgroups of 4 wavefronts, 16 384 reads per pass, so every wavefront takes a second batch and some a third."""
    from sarlacc_amd import calls
    rng = np.random.default_rng(40000)
    n = 40000
    lengths = rng.integers(10, 21, n)
    flat = rng.choice(np.frombuffer(b"ACGT", np.uint8), int(lengths.sum())).tobytes().decode()
    qflat = rng.integers(40, 90, int(lengths.sum())).astype(np.uint8).tobytes().decode()
    off = np.concatenate([[0], np.cumsum(lengths)])
    seqs = [flat[off[i]:off[i + 1]] for i in range(n)]
    quals = [qflat[off[i]:off[i + 1]] for i in range(n)]
    panel = ["ACGTTGCAAGCT", "TTGACCGTAAGC", "ACGTTGCATGCT"]
    want = expect(oracle, oenc, seqs, quals, panel, 5, 1)
    calls.set_option("align_waves_per_cu", 1)
    try:
        got = resident(seqs, quals).barcode_panel(panel, 5, 1, all_scores=True)
    finally:
        calls.set_option("align_waves_per_cu", 0)
    same(got, want)
    assert counters()["launches"] == 1


# ---- the generic uses it -------------------------------------------------------------------------------------------
def test_generic_uses_the_panel(oracle, oenc):
    """generics.barcodeAlign against R/barcodeAlign.R:20-36 restated read by read and barcode by barcode (as
    test_barcode_align_generic_read_by_read does), the single scores from the oracle."""
    from sarlacc_amd import generics
    from sarlacc_amd.mock import random_reads
    seqs, quals = random_reads(30, 8, 16, seed=11, qual_lo=40, qual_hi=80)
    rng = np.random.default_rng(12)
    barcodes = [_rand(rng, 12) for _ in range(10)]
    barcodes = barcodes[:4] + [barcodes[1]] + barcodes[4:] + [seqs[3][:12].ljust(12, "A")]   # a duplicate; one near a read
    assert len(barcodes) == 12 and all(len(b) == 12 for b in barcodes)
    out = generics.barcodeAlign(generics.Reads(seqs, quals), barcodes)
    assert counters()["launches"] == 1 and counters()["fused_barcodes"] == 12
    for i, (s, q) in enumerate(zip(seqs, quals)):
        cur, nxt, cid = -np.inf, -np.inf, None
        for b, bc in enumerate(barcodes):
            sc = float(oracle.barcode_align([s], [q], oenc, 5, 1, bc)[0])
            if sc > cur:
                cid, nxt, cur = b + 1, cur, sc
            elif sc > nxt:
                nxt = sc
        assert out["barcode"][i] == cid and out["score"][i] == cur and out["gap"][i] == cur - nxt
