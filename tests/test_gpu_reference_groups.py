"""generics.referenceGroups on the device (csrc/ref_map.hip; sarlacc_dev_sketch_candidates and
sarlacc_dev_candidates_assign), compared exactly, dtype included, with the restatement tests/reference_groups_cases.py
(DESIGN §4.20).  The device batches have buffers exactly as long as their data, so the last reference and the last read
end at their buffer's end."""
import numpy as np
import pytest

from tests import links_verify_cases as V
from tests import reference_groups_cases as R
from tests import sketch_cases as S

pytestmark = pytest.mark.gpu


def _device_reads(seqs):
    """A resident batch whose buffers are exactly as long as the reads."""
    from sarlacc_amd.resident import DevBuffer, DeviceReads
    chars = np.frombuffer(b"".join(seqs), np.uint8)
    off = np.zeros(len(seqs) + 1, np.int64)
    np.cumsum([len(s) for s in seqs], out=off[1:])
    assert chars.size and len(seqs[-1]) > 0
    return DeviceReads(DevBuffer.from_numpy(chars), DevBuffer.from_numpy(chars), DevBuffer.from_numpy(off), off, None)


def _strings(seqs):
    return [s.decode("latin-1") for s in seqs]


def _run(reads, refs, **kwargs):
    """referenceGroups on exact-size device batches of both sides, held to the restatement."""
    from sarlacc_amd import generics
    got = generics.referenceGroups(_device_reads(reads), _device_reads(refs), **kwargs)
    R.same(got, R.expected(reads, refs, **kwargs), str(kwargs))
    return got


def _counters():
    from sarlacc_amd import _lib
    return tuple(int(_lib.stage_count(name)) for name in ("refmap_hits", "refmap_checked", "refmap_second_strand"))


# ---- planted sets ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", S.SEEDS)
@pytest.mark.parametrize("rates, min_shared, identity", R.PLANTED)
def test_planted_sets(seed, rates, min_shared, identity):
    """8 references of 300 bases, every odd one sharing 100 bases with the one before, 48 reads, half of them
    reverse-complemented: every read on its own transcript, the flipped ones on strand 1, at most 2 candidates."""
    from sarlacc_amd import generics
    reads, transcript, refs = R.planted_set(seed, *rates)
    kwargs = dict(min_shared=min_shared, identity=identity)
    got = _run(reads, refs, **kwargs)
    assert np.array_equal(got["reference"], transcript) and got["strand"].sum() == 24 and got["n.candidates"].max() <= 2
    assert np.array_equal(got["strand"], np.arange(48) % 2)
    hits, checked, second = _counters()
    assert hits == int(got["n.hits"]) > 0 and checked == int(got["n.checked"]) >= 48 and second >= 24
    R.same(generics.referenceGroups(generics.Reads(_strings(reads)), _strings(refs), **kwargs), got, "Reads and strings")
    R.same(generics.referenceGroups(_device_reads(reads), generics.Reads(_strings(refs)), **kwargs), got, "second run, references as Reads")


def test_the_distance_overrides_the_rank():
    """10 % + 2 %, seed 2, min_shared 1: the best-ranked candidate of one read is its transcript's neighbour."""
    reads, transcript, refs = R.planted_set(2, 0.10, 0.02)
    plain = _run(reads, refs, min_shared=1, identity=None)
    assert "n.checked" not in plain and (plain["reference"] != transcript).sum() == 1
    assert (plain["dist"] == -1).all() and plain["strand"].sum() == 0
    hits, checked, second = _counters()
    assert hits == int(plain["n.hits"]) and checked == 0 and second == 0
    checked_run = _run(reads, refs, min_shared=1, identity=0.7)
    assert np.array_equal(checked_run["reference"], transcript)
    wrong = int(np.flatnonzero(plain["reference"] != transcript)[0])
    assert plain["reference"][wrong] == (transcript[wrong] ^ 1) and checked_run["n.candidates"][wrong] == 2


@pytest.mark.parametrize("kwargs", [dict(bandwidth=0), dict(bandwidth=16), dict(bandwidth=127), dict(buckets=16), dict(buckets=256),
                                    dict(k=16, buckets=128, min_shared=1, max_candidates=16, identity=1.0),
                                    dict(k=5, min_shared=64, max_candidates=1, identity=0.5)], ids=str)
def test_other_settings_equal_the_restatement(kwargs):
    reads, _, refs = R.planted_set(1, 0.05, 0.01)
    _run(reads, refs, **kwargs)


@pytest.mark.parametrize("seed", S.SEEDS)
def test_one_strand_only(seed):
    """both_strands=False: stranded k-mers and no second orientation, so the flipped reads are unmapped."""
    reads, transcript, refs = R.planted_set(seed, 0.05, 0.01)
    got = _run(reads, refs, min_shared=1, both_strands=False)
    flipped = np.arange(48) % 2 == 1
    assert (got["reference"][flipped] == -1).all() and np.array_equal(got["reference"][~flipped], transcript[~flipped])
    assert got["strand"].sum() == 0 and _counters()[2] == 0


# ---- edge cases ------------------------------------------------------------------------------------------------------------
def test_a_single_reference():
    rng = np.random.default_rng(21)
    ref = S.random_bases(rng, 200)
    reads = [V.noisy(rng, ref, nsub=5), S.random_bases(rng, 200), V.rc(V.noisy(rng, ref, ndel=2, nins=1)), ref]
    got = _run(reads, [ref], min_shared=1)
    assert got["reference"].tolist() == [0, -1, 0, 0] and got["strand"].tolist() == [0, 0, 1, 0] and got["dist"].tolist() == [5, -1, 3, 0]
    assert got["groups"][0].tolist() == [0, 3] and got["groups"][1].tolist() == [1, 3, 4]


def test_sequences_without_kmers():
    """A reference shorter than k is never a candidate; a read without k-mers, and reads of length 0, get -1."""
    rng = np.random.default_rng(22)
    ref = S.random_bases(rng, 150)
    refs = [b"ACGTACGTACGT", ref, b"N" * 40, ref[:75] + S.random_bases(rng, 75)]
    reads = [b"", ref, b"ACGTACGTACGT", b"", b"N" * 40, V.noisy(rng, refs[3], nsub=3), b"", V.rc(ref)]
    got = _run(reads, refs, min_shared=1)
    assert got["ref.n.kmers"].tolist() == [0, 138, 0, 138] and got["n.kmers"].tolist() == [0, 138, 0, 0, 0, 138, 0, 138]
    assert got["reference"].tolist() == [-1, 1, -1, -1, -1, 3, -1, 1] and got["strand"].tolist() == [0, 0, 0, 0, 0, 0, 0, 1]
    assert got["n.candidates"].tolist() == [0, 2, 0, 0, 0, 2, 0, 2] and got["groups"][0].tolist() == [0, 2, 3]
    # the same through a Reads, whose buffer is not of exact size
    from sarlacc_amd import generics
    R.same(generics.referenceGroups(generics.Reads(_strings(reads)), _strings(refs), min_shared=1), got, "Reads")


def test_seventy_identical_references():
    """A run of equal hashes longer than a wavefront, `shared` tied: the lowest references take the slots, and the equal
    distance goes to rank 0."""
    from sarlacc_amd import refmap, sketch
    rng = np.random.default_rng(23)
    ref = S.random_bases(rng, 260)
    refs = [S.random_bases(rng, 260)] * 2 + [ref] * 70 + [S.random_bases(rng, 260)]
    reads = [V.noisy(rng, ref, nsub=8, ndel=1), V.rc(V.noisy(rng, ref, nsub=2)), refs[0], refs[-1]]
    got = _run(reads, refs, max_candidates=4)
    assert got["reference"].tolist() == [2, 2, 0, 72] and got["n.candidates"].tolist() == [4, 4, 2, 1] and got["dist"].tolist() == [9, 2, 0, 0]
    assert int(got["n.hits"]) >= 70 * int(got["shared"][0] + got["shared"][1]) and got["shared"][0] == got["shared"][:1].max() > 2
    # every slot through the two calls: references 2 .. 5 at one distance
    dr, df = _device_reads(reads), _device_reads(refs)
    fsk, _ = sketch.sketch_reads(df.seq, df.off, len(refs), 13, 64)
    rsk, _ = sketch.sketch_reads(dr.seq, dr.off, len(reads), 13, 64)
    cand_ref, cand_shared, ncand, nhits = refmap.sketch_candidates(fsk, len(refs), rsk, len(reads), 64, 2, 4)
    assert nhits == int(got["n.hits"]) and ncand.to_numpy(np.int32, 4).tolist() == [4, 4, 2, 1]
    assert cand_ref.to_numpy(np.int32, 16).reshape(4, 4).tolist() == [[2, 3, 4, 5], [2, 3, 4, 5], [0, 1, -1, -1], [72, -1, -1, -1]]
    (reference, strand, dist, shared), nchecked, (cand_dist, cand_strand) = refmap.candidates_assign(
        df.seq, df.off, len(refs), dr.seq, dr.off, len(reads), cand_ref, cand_shared, 4, 100, V.max_diff_ppm(0.8), True, per_slot=True)
    assert nchecked == 11 == int(got["n.checked"])
    assert cand_dist.to_numpy(np.int32, 16).reshape(4, 4).tolist() == [[9] * 4, [2] * 4, [0, 0, -1, -1], [0, -1, -1, -1]]
    assert cand_strand.to_numpy(np.uint8, 16).reshape(4, 4).tolist() == [[0] * 4, [1] * 4, [0] * 4, [0] * 4]
    assert reference.to_numpy(np.int32, 4).tolist() == [2, 2, 0, 72] and shared.to_numpy(np.int32, 4).tolist() == got["shared"].tolist()


def _candidates(ref_sketch, read_sketch, buckets, min_shared, max_candidates):
    """sarlacc_dev_sketch_candidates on host sketch arrays: (cand_ref, cand_shared as [n, max_candidates], ncand, hits)
    and the device table."""
    from sarlacc_amd import refmap
    from sarlacc_amd.resident import DevBuffer
    nf, n = len(ref_sketch), len(read_sketch)
    table = refmap.sketch_candidates(DevBuffer.from_numpy(ref_sketch), nf, DevBuffer.from_numpy(read_sketch), n, buckets, min_shared, max_candidates)
    cand_ref, cand_shared, ncand, nhits = table
    return (cand_ref.to_numpy(np.int32, n * max_candidates).reshape(n, max_candidates).copy(),
            cand_shared.to_numpy(np.int32, n * max_candidates).reshape(n, max_candidates).copy(), ncand.to_numpy(np.int32, n).copy(), nhits), table


@pytest.mark.parametrize("min_shared, max_candidates", [(1, 2), (2, 2), (1, 1), (3, 16), (4, 1)])
def test_hand_set_sketches_through_the_first_call(min_shared, max_candidates):
    """The two-reference, three-read case of the host test, rule M2 and M3 on the device."""
    fsk, rsk = R.hand_sketch_pair(R.HAND_REFS, R.HAND_READS)
    (cand_ref, cand_shared, ncand, nhits), _ = _candidates(fsk, rsk, 16, min_shared, max_candidates)
    shared, want_hits = R.hits_of(fsk, rsk)
    assert shared == R.HAND_SHARED and nhits == want_hits == R.HAND_HITS and _counters()[0] == R.HAND_HITS
    want = R.candidates_of(shared, 3, min_shared, max_candidates)
    assert np.array_equal(cand_ref, want[0]) and np.array_equal(cand_shared, want[1]) and np.array_equal(ncand, want[2])


def test_max_candidates_one_hides_the_reference_behind_a_decoy():
    """Hand-set sketches: the decoy shares three buckets with the read, its true reference two.  One slot holds the decoy,
    which fails the check; two slots reach the reference."""
    from sarlacc_amd import refmap
    rng = np.random.default_rng(24)
    truth, decoy = S.random_bases(rng, 120), S.random_bases(rng, 120)
    reads, refs = [S.random_bases(rng, 90), V.noisy(rng, truth, nsub=4)], [decoy, truth]
    fsk, rsk = R.hand_sketch_pair([[1, 2, 3, R.E, R.E], [R.E, R.E, R.E, 4, 5]], [[R.E] * 5, [1, 2, 3, 4, 5]])
    dr, df = _device_reads(reads), _device_reads(refs)
    for max_candidates, want_ref, want_dist in ((1, [-1, -1], [-1, -1]), (2, [-1, 1], [-1, 4])):
        (cand_ref, cand_shared, ncand, nhits), table = _candidates(fsk, rsk, 16, 2, max_candidates)
        assert cand_ref[1].tolist() == [0, 1][:max_candidates] and cand_shared[1].tolist() == [3, 2][:max_candidates] and nhits == 5
        assert ncand.tolist() == [0, max_candidates]
        for ppm, ref_now, dist_now in ((V.max_diff_ppm(0.9), want_ref, want_dist), (-1, [-1, 0], [-1, -1])):      # unchecked: the decoy
            (reference, strand, dist, shared), nchecked, (cand_dist, _) = refmap.candidates_assign(
                df.seq, df.off, 2, dr.seq, dr.off, 2, table[0], table[1], max_candidates, 100, ppm, True, per_slot=True)
            assert reference.to_numpy(np.int32, 2).tolist() == ref_now and dist.to_numpy(np.int32, 2).tolist() == dist_now
            assert nchecked == (max_candidates if ppm >= 0 else 0) and _counters()[1] == nchecked
            assert cand_dist.to_numpy(np.int32, 2 * max_candidates).tolist() == [-1] * max_candidates + ([-1, 4][:max_candidates] if ppm >= 0 else [-1] * max_candidates)
            assert shared.to_numpy(np.int32, 2).tolist() == [0, {1: 2, 0: 3, -1: 0}[ref_now[1]]]


def test_min_shared_at_and_above_a_reads_shared():
    rng = np.random.default_rng(25)
    ref = S.random_bases(rng, 300)
    reads = [V.noisy(rng, ref, nsub=20, ndel=3, nins=3), ref]
    shared = int(R.expected(reads, [ref], min_shared=1)["shared"][0])
    assert 1 <= shared < 64
    assert _run(reads, [ref], min_shared=shared)["reference"].tolist() == [0, 0]
    assert _run(reads, [ref], min_shared=shared + 1)["reference"].tolist() == [-1, 0]


@pytest.mark.parametrize("both_strands", [True, False])
def test_the_threshold_is_inclusive(both_strands):
    """dist == t passes and t + 1 fails, on either strand, through the second call with every slot's result."""
    from sarlacc_amd import refmap
    from sarlacc_amd.resident import DevBuffer
    rng = np.random.default_rng(26)
    ref = S.random_bases(rng, 300)
    ppm = V.max_diff_ppm(0.9)
    t = V.threshold(ppm, 300, 300)
    assert t == 30
    found = {}
    for nsub in range(26, 40):
        read = V.noisy(rng, ref, nsub=nsub)
        found.setdefault(V.banded(ref, read, 100), read)
    assert t in found and t + 1 in found                       # substitutions at distinct places: the distance is their number
    reads = [found[t], found[t + 1], V.rc(found[t]), V.rc(found[t + 1])]
    cand = np.zeros((4, 1), np.int32)
    want_dist, want_strand, _ = R.check_slots([ref], reads, cand, ppm, 100, both_strands)
    assert want_dist[:, 0].tolist() == ([t, -1, t, -1] if both_strands else [t, -1, -1, -1])
    dr, df = _device_reads(reads), _device_reads([ref])
    (reference, strand, dist, shared), nchecked, (cand_dist, cand_strand) = refmap.candidates_assign(
        df.seq, df.off, 1, dr.seq, dr.off, 4, DevBuffer.from_numpy(cand), DevBuffer.from_numpy(np.full((4, 1), 7, np.int32)), 1, 100, ppm,
        both_strands, per_slot=True)
    assert np.array_equal(cand_dist.to_numpy(np.int32, 4), want_dist[:, 0]) and np.array_equal(cand_strand.to_numpy(np.uint8, 4), want_strand[:, 0])
    assert np.array_equal(dist.to_numpy(np.int32, 4), want_dist[:, 0]) and np.array_equal(strand.to_numpy(np.uint8, 4), want_strand[:, 0])
    assert reference.to_numpy(np.int32, 4).tolist() == [0 if d >= 0 else -1 for d in want_dist[:, 0]]
    assert shared.to_numpy(np.int32, 4).tolist() == [7 if d >= 0 else 0 for d in want_dist[:, 0]]
    assert nchecked == 4 and _counters()[1:] == (4, 3 if both_strands else 0)


def test_several_workgroups_and_a_partial_last_one():
    """300 reads against 3 references at 16 buckets: 4 800 read entries in 19 workgroups, 300 reads in 2, 1 200 slots in 5."""
    rng = np.random.default_rng(27)
    refs = [S.random_bases(rng, 180) for _ in range(3)]
    reads = [V.noisy(rng, refs[i % 3], nsub=int(rng.integers(0, 12)), ndel=int(rng.integers(0, 3)), nins=int(rng.integers(0, 3))) for i in range(300)]
    reads = [V.rc(s) if i % 5 == 0 else s for i, s in enumerate(reads)]
    got = _run(reads, refs, buckets=16, min_shared=1)
    mapped = got["reference"] >= 0
    assert np.array_equal(got["reference"][mapped], (np.arange(300) % 3)[mapped]) and mapped.sum() > 150
    assert np.array_equal(got["strand"][mapped], (np.arange(300) % 5 == 0)[mapped])
    assert [len(m) for m in np.split(got["groups"][1], got["groups"][0][1:-1])] == [int((got["reference"] == f).sum()) for f in range(3)]


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_by_message_and_a_valid_call_afterwards():
    from sarlacc_amd import _lib, refmap
    from sarlacc_amd.resident import DevBuffer
    rng = np.random.default_rng(28)
    refs = [S.random_bases(rng, 60), S.random_bases(rng, 60)]
    reads = [V.noisy(rng, refs[0], nsub=2), V.noisy(rng, refs[1], nsub=1), refs[0]]
    dr, df = _device_reads(reads), _device_reads(refs)
    cand = DevBuffer.from_numpy(np.array([[0, 1], [1, -1], [0, 1]], np.int32))
    shared = DevBuffer.from_numpy(np.array([[5, 1], [4, 0], [9, 1]], np.int32))
    ppm = V.max_diff_ppm(0.8)

    def assign(ref_off=df.off, read_off=dr.off, cand_ref=cand, max_diff_ppm=ppm):
        out, _ = refmap.candidates_assign(df.seq, ref_off, 2, dr.seq, read_off, 3, cand_ref, shared, 2, 100, max_diff_ppm, True)
        return [b.to_numpy(dt, 3).tolist() for b, dt in zip(out, (np.int32, np.uint8, np.int32, np.int32))]
    good = [[0, 1, 0], [0, 0, 0], [2, 1, 0], [5, 4, 9]]
    assert assign() == good
    # offsets that descend, inside the buffer: only the sound sequences are read
    with pytest.raises(_lib.SarlaccError, match=r"^read 2: its offsets do not ascend inside the sequence buffer, or it has 2\^31 bases or more$"):
        assign(read_off=DevBuffer.from_numpy(np.array([0, 120, 60, 180], np.int64)))
    with pytest.raises(_lib.SarlaccError, match=r"^reference 1: its offsets do not ascend inside the sequence buffer, or it has 2\^31 bases or more$"):
        assign(ref_off=DevBuffer.from_numpy(np.array([60, 0, 120], np.int64)))
    for bad in (2, -2, 2 ** 31 - 1):
        for max_diff_ppm in (ppm, -1):
            with pytest.raises(_lib.SarlaccError, match=r"^read 3: candidate outside 0 \.\. n_refs - 1$"):
                assign(cand_ref=DevBuffer.from_numpy(np.array([[0, 1], [1, -1], [0, bad]], np.int32)), max_diff_ppm=max_diff_ppm)
    assert assign() == good
    assert assign(max_diff_ppm=-1) == [[0, 1, 0], [0, 0, 0], [-1, -1, -1], [5, 4, 9]]
    # a sketch entry outside its bucket
    fsk, rsk = R.hand_sketch_pair([[1, 2]], [[1, 2], [3, 4]])
    moved = rsk.copy()
    moved[1, 1] = 4
    for args, message in (((fsk, moved), r"^read sketch 2, bucket 1: the entry is neither empty nor a hash of that bucket$"),
                          ((moved, rsk), r"^reference sketch 2, bucket 1: ")):
        with pytest.raises(_lib.SarlaccError, match=message):
            _candidates(*args, 16, 1, 2)
    assert _candidates(fsk, rsk, 16, 1, 2)[0][0].tolist() == [[0, -1], [-1, -1]]
    with pytest.raises(_lib.SarlaccError, match="'max_candidates' lies in 1 .. 16"):
        _candidates(fsk, rsk, 16, 1, 17)


# ---- use -------------------------------------------------------------------------------------------------------------------
def test_the_result_feeds_profile_reads_and_umi_group():
    from sarlacc_amd import generics
    from sarlacc_amd.resident import DeviceReads
    from sarlacc_amd.strset import lists_from_csr
    reads, transcript, refs = R.planted_set(3, 0.05, 0.01)
    reads = reads + [S.random_bases(np.random.default_rng(29), 300)]                       # one read of no reference
    host = generics.Reads(_strings(reads), ["I" * len(s) for s in reads])
    dev = DeviceReads.upload(host)
    out = generics.referenceGroups(dev, _strings(refs))
    R.same(out, R.expected(reads, refs), "resident batch with qualities")
    assert np.array_equal(out["reference"][:48], transcript) and out["reference"][48] == -1
    profiles = generics.profileReads(dev, _strings(refs), assignment=out["reference"])
    assert len(profiles) == 8 and all(len(p["score"]) == 6 for p in profiles)
    groups = lists_from_csr(*out["groups"])
    assert [sorted(g.tolist()) for g in groups] == [sorted((np.flatnonzero(transcript == j) + 1).tolist()) for j in range(8)]
    clusters = generics.umiGroup([s[:12] for s in _strings(reads)], threshold1=1, groups=groups)
    assert sorted(i for c in clusters for i in c.tolist()) == list(range(1, 49))
