"""GPU parity of the locator's trimmed fill loop (align.hip: lane_shr1_max, RAWPF, k_align's LTRIM; option align_locate_trim).

In its steady state the framed locator hands the horizontal jump score over inside the max that consumes it, and its
staging keeps a refill's prefetch as the raw results of the loads until the next refill decodes them, the read's last
positions taken from its last four bytes.  Neither changes a result: every case is compared bit for bit with the CPU
oracle, with the snapshot path (align_locate = -1), with the loop without the trims (align_locate_trim = -1) and with each
trim alone (1, 2), on resident ASCII reads and on the 2-bit packed format.  The shapes are those at which the loop and the
staging take another path: reads of one to three bases, reads too short for a steady state, lengths around the 64-step
refills, a last refill of one to three positions, packed reads starting at every bit offset of their bytes, characters
that are not ACGT, hits landing on every row residue mod 8, batches that leave a wavefront partly filled, a quality below
the offset in a read's first and last position.  tests/test_align_locate_group_model.py shows on the CPU that the
strong-hit reads used here fit the window's code tile, so none of them may be oversize.
"""
import numpy as np
import pytest

from tests.test_align_locate_group_model import STRONG_BATCHES, strong_hit_quals, strong_hit_reads
from tests.test_gpu_align import bits, rand_quals
from tests.test_gpu_align_locate import ADAPTOR, FILLED, _families

pytestmark = pytest.mark.gpu

PENALTIES = ((5, 1), (2, 0.5))
SPECIAL = (63, 64, 65, 127, 128, 129, 130, 131, 191, 192, 193, 194, 195)   # (66 and 67 are among the lengths 1 to 80)


def _counters():
    from sarlacc_amd import _lib
    return {k: _lib.stage_count("align_" + k) for k in ("redo", "stalls", "oversize", "window_steps", "locate_k")}


def _body(rng, n):
    return "".join(np.array(list("ACGT"))[rng.integers(0, 4, n)])


def _dev_align(enc, reads, quals, adaptor, go, ge, ss, se, packed, **options):
    """adaptor_align on device-resident reads (ASCII, or 2-bit packed with the exception mask) under the given options;
    outputs in the layout of calls.adaptor_align, and the counters of the call"""
    import torch

    from sarlacc_amd import calls
    from sarlacc_amd import device as sdev
    from sarlacc_amd.strset import StringSet
    s, q = StringSet.from_strings(reads), StringSet.from_strings(quals)
    dev = torch.device("cuda", 0)
    n, total = len(s), s.total
    d_seq = torch.from_numpy(s.chars).to(dev) if total else torch.zeros(1, dtype=torch.uint8, device=dev)
    d_qual = torch.from_numpy(q.chars).to(dev) if total else torch.zeros(1, dtype=torch.uint8, device=dev)
    d_off = torch.from_numpy(s.off).to(dev)
    stream = torch.cuda.current_stream().cuda_stream
    mask = None
    if packed:
        d_pack = torch.zeros(total // 4 + 2, dtype=torch.uint8, device=dev)
        mask = torch.zeros(total // 8 + 1, dtype=torch.uint8, device=dev)
        sdev.dev_pack_reads(d_seq, total, d_pack, mask, stream)
        d_seq = d_pack
    sc = torch.zeros(n, dtype=torch.float64, device=dev)
    st, en, so, sw = (torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(4))
    for name, value in options.items():
        calls.set_option(name, value)
    try:
        sdev.dev_align(d_seq, d_qual, d_off, n, int(s.widths().max(initial=0)), enc, go, ge, adaptor, True, list(ss), list(se),
                       sc, st, en, so, sw, stream, d_nmask=mask)
        torch.cuda.synchronize()
        return (sc.cpu().numpy(), st.cpu().numpy(), en.cpu().numpy(), [so.cpu().numpy()], [sw.cpu().numpy()]), _counters()
    finally:
        for name in options:
            calls.set_option(name, 0)


def _same(want, got, what):
    assert np.array_equal(bits(want[0]), bits(got[0])), "scores differ: " + what
    assert np.array_equal(want[1], got[1]) and np.array_equal(want[2], got[2]), "positions differ: " + what
    for a, b in zip(list(want[3]) + list(want[4]), list(got[3]) + list(got[4])):
        assert np.array_equal(a, b), "sections differ: " + what


def _all_paths(oracle, oenc, enc, reads, quals, adaptor=ADAPTOR, go=5, ge=1, ss=(9,), se=(21,), formats=(False, True)):
    """The oracle against the trimmed loop, the loop without the trims and the snapshot path, per resident format.
    Returns the counters of the trimmed loop and of the loop without the trims (of the last format)."""
    want = oracle.adaptor_align(reads, quals, oenc, go, ge, adaptor, list(ss), list(se))
    for packed in formats:
        what = "packed" if packed else "ASCII"
        new, cn = _dev_align(enc, reads, quals, adaptor, go, ge, ss, se, packed)
        _same(want, new, what)
        old, co = _dev_align(enc, reads, quals, adaptor, go, ge, ss, se, packed, align_locate_trim=-1)
        _same(want, old, what + ", align_locate_trim = -1")
        for part in (1, 2):
            one, c1 = _dev_align(enc, reads, quals, adaptor, go, ge, ss, se, packed, align_locate_trim=part)
            _same(want, one, what + ", align_locate_trim = %d" % part)
            assert c1["stalls"] <= 0
        snap, cs = _dev_align(enc, reads, quals, adaptor, go, ge, ss, se, packed, align_locate=-1)
        _same(want, snap, what + ", align_locate = -1")
        assert cs["redo"] == -1.0
        assert cn["stalls"] <= 0 and co["stalls"] <= 0
        assert (cn["redo"] >= 0) == (co["redo"] >= 0)
    return cn, co


def _planted(rng, n):
    """a read of n bases holding a copy of the adaptor where one fits"""
    b = _body(rng, n)
    if n < 30:
        return b
    e = int(rng.integers(0, n - 29))
    return b[:e] + FILLED + b[e + 30:]


def test_read_lengths(oracle, oenc, enc):
    """Lengths 1 to 80 and those around the staging refills, in index order (work items of mixed lengths: the steady
    state ends with the item's shortest read) and eight reads of a length in a row (it runs to the reads' last whole block)."""
    rng = np.random.default_rng(41)
    lengths = list(range(1, 81)) + list(SPECIAL)
    mixed = [_planted(rng, n) for n in lengths]
    uniform = [_planted(rng, n) for n in (7, 8, 9, 14, 15, 16, 17, 22, 23, 24, 25, 31) + SPECIAL for _ in range(8)]
    for reads in (mixed, uniform):
        quals = rand_quals(reads, len(reads), lo=35, hi=80)
        for go, ge in PENALTIES:
            cn, co = _all_paths(oracle, oenc, enc, reads, quals, go=go, ge=ge)
            assert cn["redo"] >= 0 and cn["locate_k"] > 0, "the call did not take the framed locator"
            assert cn["stalls"] == 0 and co["stalls"] == 0


@pytest.mark.parametrize("n", STRONG_BATCHES)
def test_strong_hits_on_every_row_residue(oracle, oenc, enc, n):
    """One clean copy landing on every row residue mod 8, in windows that start at row 0 and on the read's last row;
    batches that fill a wavefront partly, exactly, and with one read over.  None is oversize (the CPU model shows that
    their windows fit the tile)."""
    reads = strong_hit_reads(n)
    quals = strong_hit_quals(reads)
    for go, ge in PENALTIES:
        cn, co = _all_paths(oracle, oenc, enc, reads, quals, go=go, ge=ge)
        assert cn["redo"] >= 0 and cn["locate_k"] > 0
        assert cn["stalls"] == 0 and co["stalls"] == 0
        assert cn["oversize"] == 0 and co["oversize"] == 0 and cn["redo"] == 0


def test_equal_hits(oracle, oenc, enc):
    """Two copies with the same qualities, so that both rows reach the score and the candidate rows span both: 4 to 20 rows
    apart, and 300 and 1 500 rows apart, where the read is oversize with and without the trims."""
    rng = np.random.default_rng(43)
    near, far = (4, 8, 12, 20), (300, 1500)
    reads, at = [], []
    for k, gap in enumerate(near + far):
        a = 100 + k
        reads.append(_body(rng, a) + FILLED + _body(rng, gap) + FILLED + _body(rng, 50))
        at.append(a)
    quals = rand_quals(reads, 44, lo=45, hi=75)
    for k, gap in enumerate(near + far):
        a = at[k]
        quals[k] = quals[k][:a + 30 + gap] + quals[k][a:a + 30] + quals[k][a + 60 + gap:]
    for go, ge in PENALTIES:
        cn, co = _all_paths(oracle, oenc, enc, reads, quals, go=go, ge=ge)
        assert cn["stalls"] == 0 and co["stalls"] == 0
        assert cn["oversize"] >= len(far) and co["oversize"] >= len(far)
        cn, co = _all_paths(oracle, oenc, enc, reads[len(near):], quals[len(near):], go=go, ge=ge)
        assert cn["oversize"] == len(far) == co["oversize"] and cn["stalls"] == 0 and co["stalls"] == 0


@pytest.mark.parametrize("adaptor", ["ACGTNNNNACGTRYACG", "ACGTNNNNACGTRYACGTVHAC", ADAPTOR, "ACGATCAGCNNNNNNNNNNNNGTCAGTCAGTC"])
def test_adaptors(oracle, oenc, enc, adaptor):
    """17, 22, 30 and 32 columns (17 columns take sixteen-lane alignments and with them the snapshot path: there the options
    change nothing)."""
    R = len(adaptor)
    assert R in (17, 22, 30, 32)
    rng = np.random.default_rng(R)
    reads = [r[:400] for r in _families(R)]
    reads += [_body(rng, int(rng.integers(0, 120))) + adaptor.replace("N", "A").replace("R", "G").replace("Y", "C").replace("V", "A").replace("H", "T") +
              _body(rng, int(rng.integers(0, 60))) for _ in range(40)]
    quals = rand_quals(reads, R + 1, lo=35, hi=80)
    for go, ge in PENALTIES:
        cn, co = _all_paths(oracle, oenc, enc, reads, quals, adaptor, go, ge, (0,), (R,))
        assert (cn["redo"] >= 0) == (R != 17)
        assert cn["stalls"] <= 0 and co["stalls"] <= 0


def test_packed_offsets_and_other_characters(oracle, oenc, enc):
    """Reads of 1 to 8 bases in front put the following reads at every offset mod 8 of the packed bases and of the mask;
    characters that are not ACGT at positions 0, 3, 4, 7, 8 and the last."""
    rng = np.random.default_rng(47)
    reads = []
    for n in range(1, 9):
        reads.append(_body(rng, n))
        r = list(_planted(rng, 90 + n))
        for p in (0, 3, 4, 7, 8, len(r) - 1):
            r[p] = "NRYacgt-"[(p + n) % 8]
        reads.append("".join(r))
        r = list(_body(rng, 40) + FILLED)
        r[-1] = "N"
        reads.append("".join(r))
    quals = rand_quals(reads, 48, lo=35, hi=80)
    for go, ge in PENALTIES:
        cn, co = _all_paths(oracle, oenc, enc, reads, quals, go=go, ge=ge)
        assert cn["redo"] >= 0 and cn["stalls"] == 0 and co["stalls"] == 0


@pytest.mark.parametrize("packed", [False, True])
def test_bad_quality_read_index(enc, packed):
    """A quality below the offset in the first and in the last position of a read: the call reports the same read with and
    without the trims.  With an adaptor character that is not IUPAC the quality error is raised only where the read
    reported is the first read with a base, so the message shows which index came back."""
    from sarlacc_amd import SarlaccError
    reads = strong_hit_reads(40)
    good = strong_hit_quals(reads)
    broken = ADAPTOR[:15] + "X" + ADAPTOR[16:]

    def message(quals, adaptor, **options):
        with pytest.raises(SarlaccError) as err:
            _dev_align(enc, reads, quals, adaptor, 5, 1, (9,), (21,), packed, **options)
        return str(err.value)

    for k, pos in ((0, 0), (0, len(reads[0]) - 1), (17, 0), (17, len(reads[17]) - 1), (39, len(reads[39]) - 1)):
        quals = list(good)
        quals[k] = quals[k][:pos] + " " + quals[k][pos + 1:]
        for adaptor in (ADAPTOR, broken):
            new = message(quals, adaptor)
            assert new == message(quals, adaptor, align_locate_trim=-1) == message(quals, adaptor, align_locate=-1)
            if adaptor == ADAPTOR or k == 0:
                assert "quality cannot be lower than smallest encoded value" in new
        # two bad reads: the first one is reported
        if k:
            quals[k - 1] = " " + quals[k - 1][1:]
            assert message(quals, broken) == message(quals, broken, align_locate_trim=-1)
