"""generics.sequenceGroups(identity=, bandwidth=) on the device: the sketch's links checked by the alignment of rule 6a
(csrc/links_verify.hip) before the components are formed, compared exactly with the restatement (tests/sketch_cases.py
for the links, tests/links_verify_cases.py for the check and the groups).

The planted sets hold transcripts that share a third of their bases with a neighbour: the sketch alone chains every
such pair into one group whatever its settings, the sketch and the alignment return one group per transcript."""
import numpy as np
import pytest

from tests import links_verify_cases as V
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


@pytest.mark.parametrize("seed", S.SEEDS)
@pytest.mark.parametrize("rates, min_shared, identity", V.PLANTED)
def test_planted_sets(seed, rates, min_shared, identity):
    from sarlacc_amd import _lib, generics
    seqs, transcript = V.planted_set(seed, *rates)
    dev = _device_reads(seqs)
    kwargs = dict(min_shared=min_shared, identity=identity, bandwidth=100)
    want = V.expected(seqs, **kwargs)
    got = generics.sequenceGroups(dev, **kwargs)
    V.same(got, want, "DeviceReads")
    assert S.one_group_per_transcript(got["group"], transcript) and got["group"].max() + 1 == 8
    assert _lib.stage_count("sketch_verify_pairs") == int(got["n.links"]) > int(got["n.verified"]) > 0
    assert _lib.stage_count("sketch_verify_second_strand") > 0
    V.same(generics.sequenceGroups(generics.Reads([s.decode() for s in seqs]), **kwargs), want, "Reads")
    V.same(generics.sequenceGroups(dev, **kwargs), got, "second run")
    # the sketch alone: every pair of neighbours in one group
    plain = generics.sequenceGroups(dev, min_shared=min_shared)
    S.same(plain, S.expected(seqs, min_shared=min_shared), "without identity")
    assert "n.verified" not in plain and not S.one_group_per_transcript(plain["group"], transcript) and plain["group"].max() + 1 == 4
    assert _lib.stage_count("sketch_verify_pairs") == 0 and _lib.stage_count("sketch_verify_second_strand") == 0


@pytest.mark.parametrize("kwargs", [dict(min_shared=2, identity=0.7), dict(min_shared=1, identity=0.8, bandwidth=16),
                                    dict(min_shared=1, identity=0.9, bandwidth=0), dict(k=16, buckets=128, window=3, min_shared=2, identity=1.0),
                                    dict(min_shared=1, identity=0.5, bandwidth=127)], ids=str)
def test_other_settings_equal_the_restatement(kwargs):
    """Settings for which one group per transcript is not claimed (at 10 % + 2 % and min_shared 2 the restatement itself
    splits a transcript): every key equals the restatement all the same."""
    from sarlacc_amd import generics
    seqs, _ = V.planted_set(1, 0.10, 0.02)
    V.same(generics.sequenceGroups(_device_reads(seqs), **kwargs), V.expected(seqs, **kwargs), str(kwargs))


def test_identity_none_is_what_it_was():
    from sarlacc_amd import _lib, generics
    seqs, transcript = S.mock_set(1)
    dev = _device_reads(seqs)
    generics.sequenceGroups(dev, identity=0.8)                 # a verifying call first: its counts must not stay
    assert _lib.stage_count("sketch_verify_pairs") > 0
    got = generics.sequenceGroups(dev, identity=None)
    S.same(got, S.expected(seqs), "identity=None")
    assert sorted(got) == ["group", "groups", "n.kmers", "n.links", "n.pairs"]
    assert _lib.stage_count("sketch_verify_pairs") == 0 and _lib.stage_count("sketch_verify_second_strand") == 0
    S.same(generics.sequenceGroups(dev), got, "no keyword at all")


@pytest.mark.parametrize("seed", S.SEEDS)
def test_one_strand_only(seed):
    """canonical=False: stranded k-mers in the sketch and both_strands = 0 in the check, so on the flipped set every
    transcript falls into two groups, its reads as they stand and its reverse-complemented ones."""
    from sarlacc_amd import _lib, generics
    seqs, transcript = V.planted_set(seed, 0.05, 0.01)
    kwargs = dict(min_shared=3, identity=0.8, canonical=False)
    want = V.expected(seqs, **kwargs)
    got = generics.sequenceGroups(_device_reads(seqs), **kwargs)
    V.same(got, want, "stranded")
    assert _lib.stage_count("sketch_verify_second_strand") == 0
    # no group holds two transcripts or both strands, so every transcript lies in two groups at least: 16 groups by the
    # restatement on seeds 1 and 3, 18 on seed 2, where two of the halves of three reads fall apart once more
    flipped = np.arange(len(seqs)) % 2
    halves = set(zip(got["group"].tolist(), transcript.tolist(), flipped.tolist()))
    assert got["group"].max() + 1 == len(halves) == {1: 16, 2: 18, 3: 16}[seed]


def test_reads_without_a_link_or_a_kmer():
    from sarlacc_amd import generics
    rng = np.random.default_rng(5)
    base = S.random_bases(rng, 300)
    seqs = [b"ACGT", base, b"N" * 50, base[:150] + S.random_bases(rng, 150), b"", S.random_bases(rng, 300), V.noisy(rng, base, nsub=10)]
    got = generics.sequenceGroups(generics.Reads([s.decode() for s in seqs]), min_shared=1, identity=0.8)
    V.same(got, V.expected(seqs, min_shared=1, identity=0.8), "mixed")
    assert got["group"].tolist() == [-1, 0, -1, 1, -1, 2, 0] and int(got["n.links"]) == 3 and int(got["n.verified"]) == 1
