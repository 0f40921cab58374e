"""GPU parity of adaptor_align's integer locator path (align.hip MODE 4, see LOC_NEG).

The locator fills the DP in int32, and an fp64 window with traceback codes starts a few dozen rows above the candidate
landing rows from a fresh boundary.  Reads it cannot certify go on a redo list that the snapshot kernel (MODE 3) aligns.
Every case is compared with the CPU oracle bit for bit, and the two device paths are compared with each other
(align_locate = -1: the snapshot path alone; 1: every read on the redo list).
"""
import numpy as np
import pytest

from tests.test_gpu_align import bits, compare_adaptor, rand_quals

pytestmark = pytest.mark.gpu

ADAPTOR = "ACGATCAGC" + "N" * 12 + "GTCAGTCAG"
FILLED = "ACGATCAGC" + "ACGTTGCAAGTC" + "GTCAGTCAG"


def _stats():
    from sarlacc_amd import _lib
    return _lib.stage_count("align_redo"), _lib.stage_count("align_stalls")


def _families(seed):
    rng = np.random.default_rng(seed)
    nuc = np.array(list("ACGT"))

    def body(n):
        return "".join(nuc[rng.integers(0, 4, n)])

    reads = []
    # two identical adaptor copies, near and far apart (equal hits: the first row reaching the maximum wins)
    for gap in (0, 1, 5, 40, 90, 300, 1500):
        b = body(2000)
        reads.append(b[:100] + FILLED + b[130:130 + gap] + FILLED + b[160 + gap:])
    # ties through the N run: the same fixed parts around N runs of different lengths
    for n in (10, 11, 12, 13, 14):
        b = body(400)
        reads.append(b[:150] + FILLED[:9] + body(n) + FILLED[21:] + b[150 + 18 + n:])
    # long vertical gaps: read bases inserted inside the adaptor
    for ins in (5, 20, 40, 80):
        b = body(1200)
        reads.append(b[:600] + FILLED[:15] + body(ins) + FILLED[15:] + b[630 + ins:])
    # reads shorter than the adaptor, hits at row 1, empty reads, all-N reads
    reads += [FILLED[:5], FILLED[:29], FILLED, FILLED + body(500), "", "N" * 50, "N" * 2000, body(7)]
    # plain random reads and reads with a planted hit anywhere
    for _ in range(40):
        b = body(int(rng.integers(30, 2500)))
        e = int(rng.integers(0, len(b)))
        reads.append(b[:e] + FILLED + b[e:])
    reads += [body(int(rng.integers(0, 3000))) for _ in range(20)]
    return reads


def test_locator_families(oracle, oenc, enc):
    from sarlacc_amd import calls
    reads = _families(3)
    for lo, hi in ((33, 126), (40, 75), (33, 33), (126, 126)):   # '!' is a match score of -inf, '~' the largest
        quals = rand_quals(reads, lo + hi, lo=lo, hi=hi)
        compare_adaptor(oracle, oenc, enc, reads, quals, ADAPTOR, 5, 1, [9], [21])
        redo, stalls = _stats()
        assert redo >= 0, "the call did not take the locator path"
        assert stalls == 0
    # the same reads against other adaptors, penalties and sections; the locator serves the shape of eight alignments
    # per wavefront (here 1, 10, 24 and 30 columns; 18 columns take sixteen-lane alignments and the snapshot path)
    quals = rand_quals(reads, 11, lo=35, hi=80)
    for adaptor, go, ge in (("ACGTNNNNACGTRYACGTVHACGT", 5, 1), ("ACGTACGTAC", 2, 0.5), (ADAPTOR, 0, 1), ("A", 3, 1),
                            ("ACGTNNNNACGTRYACGT", 5, 1)):
        compare_adaptor(oracle, oenc, enc, reads, quals, adaptor, go, ge, [0], [len(adaptor)])
        redo, stalls = _stats()
        assert (redo >= 0) == (len(adaptor) != 18) and stalls <= 0
    # all of them through the redo list
    calls.set_option("align_locate", 1)
    try:
        compare_adaptor(oracle, oenc, enc, reads, quals, ADAPTOR, 5, 1, [9], [21])
        redo, stalls = _stats()
        assert redo == len(reads) and stalls == 0
    finally:
        calls.set_option("align_locate", 0)


def test_non_dyadic_penalties_take_the_snapshot_path(oracle, oenc, enc):
    reads = _families(4)[:40]
    quals = rand_quals(reads, 5, lo=35, hi=90)
    compare_adaptor(oracle, oenc, enc, reads, quals, ADAPTOR, 0.3, 0.7, [9], [21])
    assert _stats() == (-1.0, -1.0)


@pytest.mark.parametrize("n", [100_000, 1_000_000])
def test_locator_matches_snapshot_path_on_device_reads(n):
    """The benchmark's reads (devsynth.make_reads, 2 kb): the locator path and the snapshot path output for output, and
    the share of reads the locator hands to the snapshot kernel."""
    import torch

    from sarlacc_amd import calls, devsynth
    from sarlacc_amd import device as sdev
    from sarlacc_amd.encoding import phred_encoding
    dev = torch.device("cuda")
    a2 = "CACACTGAGCAGCGACTAGACA"
    seq, qual, off, max_len = devsynth.make_reads(n, 2000, ADAPTOR, a2, seed=1000, device=dev)
    enc = phred_encoding()

    def run():
        out = [torch.empty(n, dtype=torch.float64, device=dev)] + [torch.empty(n, dtype=torch.int32, device=dev) for _ in range(4)]
        sdev.dev_align(seq, qual, off, n, max_len, enc, 5.0, 1.0, ADAPTOR, True, [9], [21], *out)
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in out]

    new = run()
    redo, stalls = _stats()
    calls.set_option("align_locate", -1)
    try:
        old = run()
        assert _stats() == (-1.0, -1.0)
    finally:
        calls.set_option("align_locate", 0)
    assert np.array_equal(bits(old[0]), bits(new[0])), "scores differ"
    for a, b in zip(old[1:], new[1:]):
        assert np.array_equal(a, b)
    print("locator redo list: %d of %d reads, %d stalls" % (redo, n, stalls))
    assert stalls == 0
    assert redo <= 0.01 * n
