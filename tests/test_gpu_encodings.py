"""GPU parity of the quality-aware kernels under encodings other than Phred+33.

The encoding is an input of every quality-aware routine, and on the device its length and first name decide table strides
in LDS, the clamp to the last entry, the constants of adaptor_align's integer locator and which vote kernel runs.  Every
case here is compared with the CPU oracle called with the same table (tests/encodings.py), as strictly as the Phred tests
compare: score bits, positions and sections, strings, and the error message for a quality below the first name.  The last
test hands the oracle a wrong table (shifted by one entry, or cut short by one) and demands a difference from every entry
point: a comparison that still passed there would not be testing the table.
"""
import numpy as np
import pytest

from tests.encodings import BY_NAME, REJECTED, TABLE_IDS, TABLES, draw_quals
from tests.test_align_locate_model import locator_plan
from tests.test_gpu_align import bits, compare_adaptor, rand_quals
from tests.test_gpu_align_locate import ADAPTOR, FILLED, _families

pytestmark = pytest.mark.gpu

tables = pytest.mark.parametrize("table", TABLES, ids=TABLE_IDS)

A18 = "ACGTNNNNACGTRYACGT"                                   # sixteen-lane alignments, every ambiguity class but 3-fold
A70 = "ACGATCAGCVH" + "N" * 12 + "GTCAGTCAGRY" + "ACGTTGCAAGTCCATGGATCCGATTACAGGCTAACGTC"[:36]   # one alignment per wavefront
assert len(A18) == 18 and len(A70) == 70


def _stats():
    from sarlacc_amd import _lib
    return _lib.stage_count("align_redo"), _lib.stage_count("align_stalls")


def _reads():
    """The locator families, long reads cut to 700 bases (the tables matter here, not the read counts) and every fourth
    random one dropped."""
    reads = _families(3)
    return [r[:700] for i, r in enumerate(reads) if i < 24 or i % 4 != 3]


def _short(reads):
    return [r for r in reads if len(r) <= 120][:24] + [FILLED + "ACGTTGCA", "ACGT" + FILLED[:20] + "TT" + FILLED[20:]]


def _check_path(table, adaptor, go, ge, max_len, locator_shape, oracle, what):
    """The call took the locator path exactly when the model's plan_locate accepts the table (and the shape is the
    locator's: eight alignments per wavefront); nothing stalled."""
    redo, stalls = _stats()
    want = locator_shape and locator_plan(oracle, table.oenc, adaptor, go, ge, max_len) is not None
    print("ENC %-12s %-22s %s redo=%d stalls=%d" % (table.name, what, "locator" if redo >= 0 else "snapshot", redo, stalls))
    assert (redo >= 0) == want, "%s: %s path" % (what, "snapshot" if want else "locator")
    assert stalls == (0 if want else -1)
    return redo


@tables
def test_adaptor_align(oracle, table):
    from sarlacc_amd import calls
    reads = _reads()
    quals = rand_quals(reads, 101, table=table)
    max_len = max(len(r) for r in reads)
    # the locator's shape: 30 columns, at two pairs of penalties
    for go, ge in ((5, 1), (2, 0.5)):
        compare_adaptor(oracle, table.oenc, table.enc, reads, quals, ADAPTOR, go, ge, [9], [21])
        _check_path(table, ADAPTOR, go, ge, max_len, True, oracle, "30 columns %g/%g" % (go, ge))
    # sixteen-lane alignments, one alignment per wavefront: the snapshot path
    for adaptor in (A18, A70):
        compare_adaptor(oracle, table.oenc, table.enc, reads, quals, adaptor, 5, 1, [0, 4], [len(adaptor), 8])
        _check_path(table, adaptor, 5, 1, max_len, False, oracle, "%d columns 5/1" % len(adaptor))
    # every read through the redo list
    calls.set_option("align_locate", 1)
    try:
        compare_adaptor(oracle, table.oenc, table.enc, reads, quals, ADAPTOR, 5, 1, [9], [21])
        redo = _check_path(table, ADAPTOR, 5, 1, max_len, True, oracle, "30 columns, all redone")
        assert redo == len(reads)
    finally:
        calls.set_option("align_locate", 0)


@tables
def test_adaptor_align_beyond_1024_columns(oracle, table):
    rng = np.random.default_rng(1100)
    nuc = list("ACGT")
    ref = "".join(rng.choice(nuc, 1100))
    ref = ref[:300] + "NNRYVB" + ref[306:]
    core = ref.replace("N", "A").replace("R", "G").replace("Y", "T").replace("V", "C").replace("B", "T")
    reads = ["".join(c for c in core if rng.random() > 0.03) + "".join(rng.choice(nuc, 60)), core[100:700], "", core[:37],
             "".join(rng.choice(nuc, 40)) + core[250:1100]]
    quals = rand_quals(reads, 102, table=table)
    compare_adaptor(oracle, table.oenc, table.enc, reads, quals, ref, 5, 1, [300, 0], [306, 1100])
    _check_path(table, ref, 5, 1, max(len(r) for r in reads), False, oracle, "1100 columns 5/1")


@tables
def test_barcode_and_general_align(oracle, table):
    """Global scores, edit distances and gapped strings on the same reads at the small shapes."""
    from sarlacc_amd import calls
    reads = _short(_reads())
    quals = rand_quals(reads, 103, table=table)
    for ref, go, ge in ((FILLED, 5, 1), (A18, 2, 0.5), (A70, 5, 1), (FILLED, -0.5, 0.5)):
        assert np.array_equal(bits(oracle.barcode_align(reads, quals, table.oenc, go, ge, ref)),
                              bits(calls.barcode_align(reads, quals, table.enc, go, ge, ref))), "barcode scores differ"
        a = oracle.general_align(reads, quals, table.oenc, go, ge, ref)
        b = calls.general_align(reads, quals, table.enc, go, ge, ref, False)
        assert np.array_equal(bits(a[0]), bits(b[0])), "general scores differ"
        assert np.array_equal(a[1], b[1]), "edit distances differ"
        assert a[2] == b[2] and a[3] == b[3], "gapped strings differ"
        c = calls.general_align(reads, quals, table.enc, go, ge, ref, True)
        assert np.array_equal(a[1], c[1])


@pytest.mark.parametrize("name", ["solexa", "n128_high", "n256"])
def test_device_resident_and_packed_paths(oracle, name):
    """dev_align on resident ASCII reads and on the 2-bit packed format: the staged read format carries the quality
    index (up to 255 here) in its own 16-bit entries."""
    torch = pytest.importorskip("torch")
    from sarlacc_amd import device as sdev
    from sarlacc_amd.mock import random_reads
    from sarlacc_amd.strset import StringSet
    table = BY_NAME[name]
    reads, _ = random_reads(201, 0, 400, seed=77, alphabet=b"ACGTACGTACGTNR")
    quals = rand_quals(reads, 104, table=table)
    dev = torch.device("cuda", 0)
    s, q = StringSet.from_strings(reads), StringSet.from_strings(quals)
    n, total = len(s), s.total
    d_seq = torch.from_numpy(s.chars).to(dev)
    d_qual = torch.from_numpy(q.chars).to(dev)
    d_off = torch.from_numpy(s.off).to(dev)
    max_len = int(s.widths().max())
    stream = torch.cuda.current_stream().cuda_stream
    packed = torch.zeros(total // 4 + 2, dtype=torch.uint8, device=dev)
    nmask = torch.zeros(total // 8 + 1, dtype=torch.uint8, device=dev)
    sdev.dev_pack_reads(d_seq, total, packed, nmask, stream)
    for adaptor, ss, se in ((A18, [4], [8]), (ADAPTOR, [9], [21])):
        want = oracle.adaptor_align(reads, quals, table.oenc, 5, 1, adaptor, ss, se)
        want_global = oracle.barcode_align(reads, quals, table.oenc, 5, 1, adaptor)
        for seq_buf, mask in ((d_seq, None), (packed, nmask)):
            sc = torch.zeros(n, dtype=torch.float64, device=dev)
            st = torch.zeros(n, dtype=torch.int32, device=dev)
            en, so, sw = torch.zeros_like(st), torch.zeros_like(st), torch.zeros_like(st)
            sdev.dev_align(seq_buf, d_qual, d_off, n, max_len, table.enc, 5, 1, adaptor, True, ss, se, sc, st, en, so, sw,
                           stream, d_nmask=mask)
            torch.cuda.synchronize()
            assert np.array_equal(bits(sc.cpu().numpy()), bits(want[0]))
            assert np.array_equal(st.cpu().numpy(), want[1]) and np.array_equal(en.cpu().numpy(), want[2])
            assert np.array_equal(so.cpu().numpy(), want[3][0]) and np.array_equal(sw.cpu().numpy(), want[4][0])
            sc2 = torch.zeros(n, dtype=torch.float64, device=dev)
            sdev.dev_align(seq_buf, d_qual, d_off, n, max_len, table.enc, 5, 1, adaptor, False, (), (), sc2, None, None, None,
                           None, stream, d_nmask=mask)
            torch.cuda.synchronize()
            assert np.array_equal(bits(sc2.cpu().numpy()), bits(want_global))


def _mask_case(table, seed=105):
    rng = np.random.default_rng(seed)
    seqs = ["".join(rng.choice(list("ACGTN"), int(n))) for n in rng.integers(0, 90, 40)]
    seqs[0] = "ACGT" * 80                      # long enough for one pass over the whole pool
    return seqs, draw_quals(table, [len(s) for s in seqs], seed)


def _thresholds(table):
    e = table.errors
    return [0.0, 1.0, float(e[0]), float(e[-1]), float(e[len(e) // 2]), float(e[len(e) // 3]), float((e[0] + e[-1]) / 2)]


@tables
def test_mask_bad_bases(oracle, table):
    """error > threshold, strictly: thresholds equal to table entries, 0 and 1."""
    from sarlacc_amd import calls
    seqs, quals = _mask_case(table)
    for thr in _thresholds(table):
        assert calls.mask_bad_bases(seqs, quals, table.enc, thr) == oracle.mask_bad_bases(seqs, quals, table.oenc, thr), thr


def _alignments(table, seed, with_n):
    """Groups of up to 64 rows (the byte-parallel kernel where the table allows it) and of more than 64 rows."""
    rng = np.random.default_rng(seed)
    alns, quals = [], []
    for nrows, W in ((1, 40), (7, 300), (30, 530), (64, 260), (65, 130), (90, 257), (0, 0), (12, 0), (3, 1)):
        truth = rng.choice(list("ACGT"), W) if W else np.array([], dtype="<U1")
        rows = []
        for _ in range(nrows):
            r = truth.copy()
            if W:
                sub = rng.random(W) < 0.15
                r[sub] = rng.choice(list("ACGT"), int(sub.sum()))
                if with_n:
                    r[rng.random(W) < 0.04] = "N"
                r[rng.random(W) < rng.choice([0.05, 0.4])] = "-"
            rows.append("".join(r))
        alns.append(rows)
        quals.append(draw_quals(table, [len(r.replace("-", "")) for r in rows], int(rng.integers(1 << 30))))
    return alns, quals


@tables
@pytest.mark.parametrize("with_n", [False, True], ids=["acgt", "with_n"])
def test_consensus_quality(oracle, table, with_n):
    """By default (k_consensus_qf where the table is eligible, k_consensus_q4 while its table fits, k_consensus<true>
    beyond) and with consensus_generic = 1: both equal the oracle."""
    from sarlacc_amd import calls
    alns, quals = _alignments(table, 106 + with_n, with_n)
    want = oracle.create_consensus_quality_loop(alns, 0.6, quals, table.oenc)
    try:
        for generic in (0, 1):
            calls.set_option("consensus_generic", generic)
            got = calls.create_consensus_quality_loop(alns, 0.6, quals, table.enc)
            assert got[0] == want[0], "consensus differs (consensus_generic = %d)" % generic
            assert got[1] == want[1], "qualities differ (consensus_generic = %d)" % generic
    finally:
        calls.set_option("consensus_generic", 0)
    # the log errors of one alignment (k_consensus<true>), to the bound the Phred tests hold them to (the device's log1p
    # and exp are not the host's: tests/test_gpu_consensus.py)
    one = calls.create_consensus_quality(alns[2], 0.6, quals[2], table.enc)
    ref = oracle.create_consensus_quality(alns[2], 0.6, quals[2], table.oenc)
    assert one[0] == ref[0] and np.allclose(one[1], ref[1], rtol=1e-11, atol=1e-300)


def _fused_case(table, seed=108):
    from sarlacc_amd.mock import NUC, mutate
    rng = np.random.default_rng(seed)
    reads, groups = [], []
    for L, m in ((60, 5), (300, 8), (0, 2), (150, 1), (90, 20), (200, 3)):
        truth = NUC[rng.integers(0, 4, L)]
        idx = []
        for _ in range(m):
            reads.append(mutate(truth, rng, 0.08, 0.03).tobytes().decode() if L else "")
            idx.append(len(reads))
        groups.append(idx)
    reads = ["".join("N" if rng.random() < 0.02 else c for c in r) for r in reads]
    return reads, groups, draw_quals(table, [len(r) for r in reads], seed)


@tables
def test_fused_msa_consensus(oracle, table):
    """msa_consensus_flat with qualities: rows written as 16-bit vote codes (tables of up to 149 entries) or as characters
    (beyond, and with consensus_chars = 1), against the oracle's quick_msa followed by its consensus, both MSA specs."""
    from sarlacc_amd import calls
    from sarlacc_amd.strset import csr_from_lists
    reads, groups, quals = _fused_case(table)
    goff, gvals = csr_from_lists(groups)
    try:
        for spec in (2, 1):
            rows = oracle.quick_msa(groups, reads, 0, -1, -5, -1, 100, spec=spec)
            want = oracle.create_consensus_quality_loop(rows, 0.6, [[quals[i - 1] for i in g] for g in groups], table.oenc)
            calls.set_msa_spec(spec)
            for chars in (0, 1):
                calls.set_option("consensus_chars", chars)
                got = calls.msa_consensus_flat(goff, gvals, reads, 0, -1, -5, -1, 100, 0.6, quals=quals, encoding=table.enc)
                assert got[0].to_strings() == want[0] and got[1].to_strings() == want[1], (spec, chars)
    finally:
        calls.set_msa_spec(0)
        calls.set_option("consensus_chars", 0)


# ---- every entry point as (name, device call, oracle call) on one small input ----
def _entry_points(oracle, table, oenc, bad=None, enc=None):
    """Callables of every quality-aware entry point on the same input, drawn for `table`: the device with `enc` (the
    table's own unless given), the oracle with `oenc`.  `bad` replaces one quality character of a base that every routine
    looks at."""
    from sarlacc_amd import calls
    from sarlacc_amd.strset import csr_from_lists
    enc = table.enc if enc is None else enc
    reads = _short(_reads())[-12:]
    quals = rand_quals(reads, 109, table=table)
    seqs, mquals = _mask_case(table)
    alns, cquals = _alignments(table, 110, False)
    alns, cquals = alns[1:4], cquals[1:4]
    freads, groups, fquals = _fused_case(table)
    if bad is not None:
        quals[-1] = quals[-1][:3] + bad + quals[-1][4:]
        mquals[0] = mquals[0][:3] + bad + mquals[0][4:]
        cquals[0][1] = bad + cquals[0][1][1:]
        k = groups[1][1] - 1
        freads[k] = "A" + freads[k][1:]
        fquals[k] = bad + fquals[k][1:]
    goff, gvals = csr_from_lists(groups)
    thr = float(table.errors[min(1, len(table) - 1)])

    def fused_oracle():
        rows = oracle.quick_msa(groups, freads, 0, -1, -5, -1, 100)
        return oracle.create_consensus_quality_loop(rows, 0.6, [[fquals[i - 1] for i in g] for g in groups], oenc)

    def fused_device():
        got = calls.msa_consensus_flat(goff, gvals, freads, 0, -1, -5, -1, 100, 0.6, quals=fquals, encoding=enc)
        return got[0].to_strings(), got[1].to_strings()

    return [
        ("adaptor_align", lambda: calls.adaptor_align(reads, quals, enc, 5, 1, ADAPTOR, [9], [21]),
         lambda: oracle.adaptor_align(reads, quals, oenc, 5, 1, ADAPTOR, [9], [21])),
        ("adaptor_align_score_only", lambda: calls.adaptor_align_score_only(reads, quals, enc, 5, 1, A18),
         lambda: oracle.adaptor_align_score_only(reads, quals, oenc, 5, 1, A18)),
        ("barcode_align", lambda: calls.barcode_align(reads, quals, enc, 5, 1, FILLED),
         lambda: oracle.barcode_align(reads, quals, oenc, 5, 1, FILLED)),
        ("general_align", lambda: calls.general_align(reads, quals, enc, 5, 1, FILLED, False),
         lambda: oracle.general_align(reads, quals, oenc, 5, 1, FILLED)),
        ("mask_bad_bases", lambda: calls.mask_bad_bases(seqs, mquals, enc, thr),
         lambda: oracle.mask_bad_bases(seqs, mquals, oenc, thr)),
        ("create_consensus_quality_loop", lambda: calls.create_consensus_quality_loop(alns, 0.6, cquals, enc),
         lambda: oracle.create_consensus_quality_loop(alns, 0.6, cquals, oenc)),
        ("msa_consensus_flat", fused_device, fused_oracle),
    ]


def _flat(x):
    """Any entry point's result as a list of comparable pieces (floats by their bits)."""
    if isinstance(x, np.ndarray):
        return [bits(x).tolist()] if x.dtype == np.float64 else [x.tolist()]
    if isinstance(x, (list, tuple)):
        return [p for y in x for p in _flat(y)]
    return [x]


@tables
def test_quality_below_the_first_name(oracle, table):
    """The reference's error and message, from every entry point.  A table whose first name is the signed char -128 has
    no character below it."""
    from sarlacc_amd import SarlaccError
    if table.below() is None:
        assert table.first == -128
        return
    for name, dev, orc in _entry_points(oracle, table, table.oenc, bad=table.below()):
        with pytest.raises(oracle.OracleError) as want:
            orc()
        assert str(want.value) == "quality cannot be lower than smallest encoded value", name
        with pytest.raises(SarlaccError) as got:
            dev()
        assert str(got.value) == str(want.value), name


@pytest.mark.parametrize("case", REJECTED, ids=[c[0] for c in REJECTED])
def test_rejected_tables(oracle, case):
    """Tables the reference's check refuses -- empty, names not consecutive (257 names never are), probabilities
    increasing -- through every entry point, with the oracle's message."""
    from sarlacc_amd import SarlaccError
    from sarlacc_amd.encoding import Encoding
    _, errors, names, message = case
    for name, dev, orc in _entry_points(oracle, BY_NAME["phred"], (errors, names), enc=Encoding(errors, names)):
        with pytest.raises(oracle.OracleError) as want:
            orc()
        assert str(want.value) == message, name
        with pytest.raises(SarlaccError) as got:
            dev()
        assert str(got.value) == message, name


@pytest.mark.parametrize("name,wrong", [("phred", "shifted"), ("solexa", "shifted"), ("n128_high", "shifted"),
                                        ("n256", "shifted"), ("two", "cut")])
def test_a_wrong_table_is_seen(oracle, name, wrong):
    """The oracle with the same table shifted by one entry (or cut short by one): every entry point's output must differ
    from the device's, which the tests above show equal to the oracle's under the right table."""
    table = BY_NAME[name]
    for ep, dev, orc in _entry_points(oracle, table, getattr(table, wrong)()):
        assert _flat(dev()) != _flat(orc()), "%s gives the same output under a wrong table" % ep
    for ep, dev, orc in _entry_points(oracle, table, table.oenc):
        assert _flat(dev()) == _flat(orc()), ep
