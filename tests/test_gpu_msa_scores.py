"""The MSA stage across its scoring domain: which pairwise kernel a scoring takes (bit-vector, packed 16-bit with linear or
affine gaps, 32-bit at 4, 8 or 16 cells per lane -- asserted by the library's counters, not by restating its rules), rows
equal to the CPU statement character for character under each, the stated scoring domain at its edge, and spec v2's
guard for weights that do not fit their fields.  The CPU statement's own pairwise DP is checked against an independent
one under the same scoring sets in tests/test_oracle_msa_scores.py.

Every call prints its counters (pytest -s) before anything is asserted on them."""
import numpy as np
import pytest

from tests import msa_score_cases as K

pytestmark = pytest.mark.gpu

COUNTERS = ("msa_pairs", "msa_pairs_bitvector", "msa_pairs_packed", "msa_pairs_packed_linear", "msa_pairs_int32", "msa_pairs_packed_c4", "msa_pairs_packed_c8",
            "msa_pairs_packed_c16", "msa_pairs_int32_c4", "msa_pairs_int32_c8", "msa_pairs_int32_c16")


@pytest.fixture(params=[2, 1], ids=["spec2", "spec1"])
def spec(request):
    from sarlacc_amd import calls
    calls.set_msa_spec(request.param)
    yield request.param
    calls.set_msa_spec(0)


def run(spec, groups, reads, scores, bw, options=()):
    """calls.quick_msa under `options`; returns (rows, counters by their names without the msa_pairs_ prefix)."""
    from sarlacc_amd import _lib, calls
    for name, val in options:
        calls.set_option(name, val)
    try:
        got = calls.quick_msa(groups, reads, *scores, bw)
        c = {n[len("msa_pairs_"):] if n != "msa_pairs" else "pairs": int(_lib.stage_count(n)) for n in COUNTERS}
    finally:
        for name, _ in options:
            calls.set_option(name, 0)
    print("counters", scores, bw, dict(options), "spec", spec, c)
    assert c["bitvector"] + c["packed"] + c["int32"] == c["pairs"] > 0
    assert c["packed"] == c["packed_c4"] + c["packed_c8"] + c["packed_c16"] and c["int32"] == c["int32_c4"] + c["int32_c8"] + c["int32_c16"]
    return got, c


def check(oracle, spec, read_groups, scores, bw, options=()):
    reads, groups = K.flatten(read_groups)
    want = oracle.quick_msa(groups, reads, *scores, bw, spec=spec)
    got, c = run(spec, groups, reads, scores, bw, options)
    for g, (a, b) in enumerate(zip(got, want)):
        assert a == b, "group %d differs (%r, bandwidth %d)" % (g, scores, bw)
    assert len(got) == len(want)
    K.rows_spell(got, reads, groups)
    return c


def in_domain(read_groups, scores):
    """far enough inside the scoring domain that neither side's "outside the band" value is in play"""
    longest = max(len(r) for g in read_groups for r in g)
    return max(abs(int(v)) for v in scores) * (2 * longest + 2) < (1 << 27)


# ---- read sets (bandwidth 100: a pair's band has |length difference| + 201 diagonals) ----
def equal_length_groups(rng):
    out = [K.same_length_group(rng, n, length) for n, length in [(2, 60), (3, 150), (5, 300), (4, 97), (8, 64), (2, 400), (3, 201)]]
    out += [[K.random_read(rng, 130), K.random_read(rng, 130)], ["A" * 90, "C" * 90], ["ACGT" * 30, "ACGT" * 30]]
    return out


def small_difference_groups(rng, diffs=(0, 5, 27, 13, 1)):
    out = [list(K.related_pair(rng, length, d)) for length, d in zip((80, 200, 373, 150, 60), diffs)]
    out += [K.same_length_group(rng, 4, 120), K.same_length_group(rng, 7, 75)]
    a, b = K.related_pair(rng, 250, 20)
    out.append([a, b, a[:len(a) - 7]])
    return out


def three_class_groups(rng):
    """pairs in all three band classes at bandwidth 100: up to 256 diagonals, up to 512, up to 1 024"""
    out = [list(K.related_pair(rng, 700, 10, 0.05, 0.02)), list(K.related_pair(rng, 700, 200, 0.05, 0.02)),
           list(K.related_pair(rng, 600, 800, 0.05, 0.02))]
    out += [list(K.related_pair(rng, 90, 3)), K.same_length_group(rng, 3, 110)]
    return out


def general_groups(rng):
    out = []
    for n, length in [(2, 60), (3, 200), (5, 120), (8, 90), (4, 400), (6, 70)]:
        t = K.random_read(rng, length)
        out.append([K.mutate(t, rng, 0.08, 0.03) for _ in range(n)])
    return out + K.edge_groups(rng, 100)


BUILDERS = {"equal": equal_length_groups, "small": small_difference_groups, "classes": three_class_groups, "general": general_groups,
            "over30": lambda rng: small_difference_groups(rng, (0, 5, 27, 30, 1))}

# (set, reads, expected path).  Paths: "bitvector", "packed_linear", "packed_affine", "int32", "mixed".
# "linear" and "near_bound" charge every edit alike, so their pairs of up to 256 diagonals go to the bit-vector kernel on the
# product route (the packed kernel's spread bound still decides: one cost more and the same pairs go to the 32-bit kernel);
# the packed kernel takes them with the bit-vector kernel switched off, which is how its bound is approached here.
# The last column: (bit-vector, packed, 32-bit) pairs of the call under spec 2 and under spec 1 where the reads hold no empty
# one (spec 2 aligns all pairs of a group, spec 1 every read against the centre), None: only the path is asserted.
TABLE = [
    ("default", "small", "bitvector", ((35, 0, 0), (16, 0, 0))),
    ("linear", "small", "bitvector", ((35, 0, 0), (16, 0, 0))),
    ("linear", "classes", "bitvector_and_packed_linear", ((5, 2, 0), (4, 2, 0))),
    ("near_bound", "equal", "bitvector", ((55, 0, 0), (23, 0, 0))),
    ("near_bound_first_cheaper", "equal", "packed_linear", ((0, 55, 0), (0, 23, 0))),
    ("one_cost_more", "equal", "int32", ((0, 0, 55), (0, 0, 23))),
    ("affine_match5", "small", "packed_affine", ((0, 35, 0), (0, 16, 0))),
    ("affine_match5", "over30", "int32", ((0, 0, 35), (0, 0, 16))),
    ("mixed", "classes", "mixed", ((0, 6, 1), (0, 5, 1))),
    ("mismatch_above_match", "general", "int32", None),
    ("cost_5000", "general", "int32", None),
    ("match_1000", "general", "int32", None),
    ("positive_extension", "general", "int32", None),
]


def assert_path(c, path):
    if path == "bitvector":
        assert c["bitvector"] == c["pairs"]
    elif path == "packed_linear":
        assert c["packed_linear"] == c["packed"] == c["packed_c4"] == c["pairs"]
    elif path == "packed_affine":
        assert c["packed"] == c["packed_c4"] == c["pairs"] and c["packed_linear"] == 0
    elif path == "int32":
        assert c["int32"] == c["pairs"]
    elif path == "bitvector_and_packed_linear":
        assert c["bitvector"] > 0 and c["packed_c8"] > 0 and c["packed_c16"] > 0 and c["packed_linear"] == c["packed"] and c["int32"] == 0
    elif path == "mixed":   # packed up to 512 diagonals, 32-bit in the widest class -- in one call
        assert c["packed_c4"] > 0 and c["packed_c8"] > 0 and c["int32_c16"] > 0
        assert c["int32_c4"] == c["int32_c8"] == c["packed_c16"] == c["bitvector"] == c["packed_linear"] == 0
    else:
        raise AssertionError(path)


@pytest.mark.parametrize("name,readset,path,counts", TABLE, ids=["%s-%s" % (t[0], t[1]) for t in TABLE])
def test_scoring_set_takes_its_kernel_and_matches_the_oracle(oracle, spec, name, readset, path, counts):
    scores = K.SETS[name]
    rng = np.random.default_rng(sum(map(ord, name + readset)))
    read_groups = BUILDERS[readset](rng)
    assert in_domain(read_groups, scores)
    c = check(oracle, spec, read_groups, scores, 100)
    assert_path(c, path)
    if counts:
        assert (c["bitvector"], c["packed"], c["int32"]) == counts[0 if spec == 2 else 1]
    # the inputs where a carry or a wrong clamp would show, under a narrow band (a block of bandwidth - 1 bases deleted)
    edges = K.edge_groups(rng, 12)
    assert in_domain(edges, scores)
    check(oracle, spec, edges, scores, 12)


@pytest.mark.parametrize("scores,readset,path", [
    (K.SETS["linear"], "small", "packed_linear"),
    (K.SETS["near_bound"], "equal", "packed_linear"),       # spread 543 * 20 = 10 860 of 11 000
], ids=["linear", "near_bound"])
def test_packed_linear_kernel_near_its_bound(oracle, spec, scores, readset, path):
    rng = np.random.default_rng(len(readset) + abs(scores[3]))
    read_groups = BUILDERS[readset](rng)
    off = (("msa_bitvector", -1),)
    assert_path(check(oracle, spec, read_groups, scores, 100, off), path)
    check(oracle, spec, K.edge_groups(rng, 12), scores, 12, off)


def test_fractional_scores_are_truncated(oracle, spec):
    frac, whole = K.FRACTIONAL
    rng = np.random.default_rng(19)
    reads, groups = K.flatten(general_groups(rng))
    got, c = run(spec, groups, reads, frac, 100)
    assert got == run(spec, groups, reads, whole, 100)[0]
    assert got == oracle.quick_msa(groups, reads, *frac, 100, spec=spec) == oracle.quick_msa(groups, reads, *whole, 100, spec=spec)
    K.rows_spell(got, reads, groups)


ORDINARY = [(0, -1, -5, -1), (0, -1, -1, -5), (1, -2, -2, -2), (0, -1, -1, -3), (0, -1, -1, -1), (2, -3, -7, -2), (2, -3, -1, -4),
            (1, -2, -3, -2), (5, -4, -6, -8)]   # the sets of tests/test_gpu_msa.py and the fuzzer, and the doubled-cost one


@pytest.mark.parametrize("scores", ORDINARY, ids=str)
def test_msa_int32_option_all_band_classes(oracle, spec, scores):
    """k_msa_pairwise_ad<4 | 8 | 16, spec v1 | v2 outputs> under the ordinary scorings: the product route's rows, and the oracle's.
    On the product route the affine sets with small costs stay packed in all three classes (k_msa_pairwise_pk<16, ., affine>)."""
    rng = np.random.default_rng(3232)
    read_groups = three_class_groups(rng) + K.edge_groups(rng, 100)[:3]
    reads, groups = K.flatten(read_groups)
    want = oracle.quick_msa(groups, reads, *scores, 100, spec=spec)
    plain, p = run(spec, groups, reads, scores, 100)
    got, c = run(spec, groups, reads, scores, 100, (("msa_int32", 1),))
    assert got == want and plain == want
    assert c["int32"] == c["pairs"] and c["packed"] == 0 and c["bitvector"] == 0
    assert c["int32_c4"] > 0 and c["int32_c8"] > 0 and c["int32_c16"] > 0
    if scores in ((0, -1, -1, -5), (0, -1, -1, -3)):
        assert p["packed"] == p["pairs"] and p["packed_c4"] > 0 and p["packed_c8"] > 0 and p["packed_c16"] > 0 and p["packed_linear"] == 0
    K.rows_spell(got, reads, groups)


def test_scoring_domain_is_checked_on_every_route(oracle, spec):
    """max |score| * (2 * longest read + 2) < 2^27: one score beyond it is an error of quick_msa, of the
    fused call and of the resident route, and of the oracle; the largest scores inside it still match the oracle."""
    import torch
    from sarlacc_amd import calls, device
    from sarlacc_amd._lib import SarlaccError
    rng = np.random.default_rng(1500)
    t = K.random_read(rng, 1500)
    reads = [t, K.mutate(t, rng, 0.05, 0.02)[:1490], K.mutate(t, rng, 0.05, 0.02)[:1500], "ACGT"]
    groups = [[1, 2, 3]]
    inside = ((1 << 27) - 1) // (2 * 1500 + 2)
    for scores in [(0, -inside, -inside, -inside), (inside, -inside, -inside, -inside), (0, -3, inside, -inside)]:
        want = oracle.quick_msa(groups, reads, *scores, 30, spec=spec)
        got, c = run(spec, groups, reads, scores, 30)
        assert got == want, scores
        assert c["int32"] == c["pairs"]
        K.rows_spell(got, reads, groups)
    goff, gvals = np.array([0, 3], np.int64), np.array([1, 2, 3], np.int32)
    off = np.zeros(len(reads) + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in reads])
    d_seq = torch.from_numpy(np.frombuffer("".join(reads).encode(), np.uint8).copy()).to("cuda:0")
    for bad in [(0, -inside - 1, -1, -1), (0, -1, -inside - 1, -1), (inside + 1, -1, -1, -1), (0, -100000, -100000, -100000),
                (0, -1, float("nan"), -1), (0, -1, -1, -3e9)]:
        with pytest.raises(oracle.OracleError, match="scoring domain"):
            oracle.quick_msa(groups, reads, *bad, 30, spec=spec)
        with pytest.raises(SarlaccError, match="sarlacc_amd: MSA scores outside the scoring domain"):
            calls.quick_msa(groups, reads, *bad, 30)
        with pytest.raises(SarlaccError, match="sarlacc_amd: MSA scores outside the scoring domain"):
            calls.msa_consensus_flat(goff, gvals, reads, *bad, 30, 0.6)
        with pytest.raises(SarlaccError, match="sarlacc_amd: MSA scores outside the scoring domain"):
            device.dev_msa_consensus(goff, gvals, d_seq, None, off, *bad, 30, 0.6)
    # the longest read of the groups decides: the same scores on the 4-base read alone
    assert calls.quick_msa([[4, 4]], reads, 0, -100000, -100000, -100000, 30) == oracle.quick_msa([[4, 4]], reads, 0, -100000, -100000, -100000, 30, spec=spec)


def test_spec2_weights_beyond_their_fields_go_to_spec_v1(oracle):
    """Spec v2 with real weights.  64 copies of one read make w0 of every record (n - 1) * match exactly: 63 * 1040 = 65 520 is
    the last that fits 16 bits.  Groups beyond the guard's rule (oracle.msa2_weights_fit) are aligned by spec v1 on both sides."""
    from sarlacc_amd import _lib, calls
    rng = np.random.default_rng(64)
    t = K.random_read(rng, 60)
    copies = [t] * 64
    noisy = [K.mutate(t, rng, 0.014, 0.006)[:62] for _ in range(64)]
    g16 = [K.mutate(t, rng, 0.02, 0.0) for _ in range(16)]
    g33 = [K.mutate(t, rng, 0.02, 0.0) for _ in range(33)]
    assert max(map(len, noisy)) <= 64 and len(set(noisy)) > 20
    calls.set_msa_spec(2)
    try:
        for match, expect in [(2, 0), (5, 0), (100, 0), (1040, 0), (1041, 2), (5000, 4)]:
            read_groups = [copies, noisy] + ([g16, g33] if match == 5000 else [])
            reads, groups = K.flatten(read_groups)
            scores = (match, -match, -2 * match, -2 * match)
            want = oracle.quick_msa(groups, reads, *scores, 20, spec=2)
            got = calls.quick_msa(groups, reads, *scores, 20)
            diverted = int(_lib.stage_count("msa_v1_fallback_weights"))
            print("match", match, "msa_v1_fallback_weights", diverted)
            assert got == want, match
            K.rows_spell(got, reads, groups)
            rule = sum(not oracle.msa2_weights_fit(len(g), max(map(len, g)), match, -match) for g in read_groups)
            assert diverted == rule == expect, match
        # the unit-weight scores through the any-weights records: nothing is diverted
        reads, groups = K.flatten([copies, noisy, g16, g33])
        calls.set_option("msa2_general_rows", 1)
        try:
            got = calls.quick_msa(groups, reads, 0, -1, -5, -1, 20)
            assert _lib.stage_count("msa_v1_fallback_weights") == 0 and _lib.stage_count("msa_v1_fallback") == 0
        finally:
            calls.set_option("msa2_general_rows", 0)
        assert got == oracle.quick_msa(groups, reads, 0, -1, -5, -1, 20, spec=2)
        assert got == calls.quick_msa(groups, reads, 0, -1, -5, -1, 20)
        assert _lib.stage_count("msa_v1_fallback_weights") == 0 and _lib.stage_count("msa_v1_fallback") == 0
    finally:
        calls.set_msa_spec(0)


@pytest.mark.parametrize("name,path", [("one_cost_more", "int32"), ("near_bound", "packed_linear")])
def test_fused_msa_consensus_under_other_scorings(spec, name, path):
    """sarlacc_msa_consensus under a 32-bit and a near-bound packed scoring: quick_msa_flat followed by the consensus call."""
    import sarlacc_amd
    from sarlacc_amd import _lib, calls
    from sarlacc_amd.strset import StringSet, csr_from_lists
    scores = K.SETS[name]
    rng = np.random.default_rng(2121)
    reads, groups = K.flatten(equal_length_groups(rng))
    groups.insert(2, [])
    groups.append([3])
    quals = ["".join(chr(int(c)) for c in rng.integers(40, 90, len(r))) for r in reads]
    goff, gvals = csr_from_lists(groups)
    enc = sarlacc_amd.phred_encoding()
    calls.set_option("msa_bitvector", -1)
    try:
        rows, grp_rows, _ = calls.quick_msa_flat(goff, gvals, reads, *scores, 100)
        qsub = StringSet.from_strings(quals).subset(gvals[:int(goff[-1])].astype(np.int64) - 1)
        want = calls.create_consensus_flat(rows, grp_rows, 0.6, quals=qsub, encoding=enc)
        got = calls.msa_consensus_flat(goff, gvals, reads, *scores, 100, 0.6, quals=quals, encoding=enc)
        pairs = _lib.stage_count("msa_pairs")
        key = "msa_pairs_int32" if path == "int32" else "msa_pairs_packed_linear"
        assert _lib.stage_count(key) == pairs > 0
    finally:
        calls.set_option("msa_bitvector", 0)
    assert got[0].to_strings() == want[0].to_strings()
    assert got[1].to_strings() == want[1].to_strings()
    assert len(got[0]) == len(groups) and got[0][2] == ""
