"""Inputs and expected values shared by the profileReads tests (tests/test_profile_reads_abi.py,
tests/test_gpu_profile_reads.py): seeded reads derived from a homopolymer-rich reference, and the CPU oracle chain
general_align -> find_errors / match_homopolymers / find_homopolymers run through the package's own generics
(errorFinder, homopolymerMatcher) so that it comes out in their format.  Test infrastructure only."""
import contextlib

import numpy as np

from sarlacc_amd.strset import StringSet

SPECIAL_LENGTHS = (0, 1, 63, 64, 65, 127, 128, 129)


def _l(x):
    return x.to_strings() if isinstance(x, StringSet) else list(x)


class OracleCalls:
    """The three profiling routines of sarlacc_amd.calls on the CPU oracle."""

    def __init__(self, oracle):
        self.o = oracle

    def find_homopolymers(self, seqs):
        return self.o.find_homopolymers(_l(seqs))

    def match_homopolymers(self, ref, read):
        return self.o.match_homopolymers(_l(ref), _l(read))

    def find_errors(self, ref, read):
        return self.o.find_errors(_l(ref), _l(read))


@contextlib.contextmanager
def oracle_generics(oracle):
    """generics.errorFinder / homopolymerMatcher computed by the oracle for the duration."""
    from sarlacc_amd import generics
    saved = generics.calls
    generics.calls = OracleCalls(oracle)
    try:
        yield generics
    finally:
        generics.calls = saved


def rich_reference(rng, R):
    ref = rng.choice(list("ACGT"), R)
    for _ in range(R // 12):
        k = int(rng.integers(0, max(R - 6, 1)))
        ref[k:k + int(rng.integers(2, 7))] = ref[k]
    return "".join(ref)


def noisy(rng, ref, p=0.1):
    out = []
    for c in ref:
        u = rng.random()
        if u < p / 3:
            continue                                                  # deletion
        if u < 2 * p / 3:
            out += list(rng.choice(list("ACGT"), int(rng.integers(1, 5))))   # insertion of 1-4 bases
        out.append(c if u > p else "ACGT"[int(rng.integers(0, 4))])  # substitution
    return "".join(out)


def rand_seq(rng, k):
    return "".join(rng.choice(list("ACGT"), k)) if k else ""


def make_reads(rng, ref, n):
    """n reads (A/C/G/T only) with their qualities: noisy copies of `ref`, reads of the special lengths, a long
    insertion (more than 64 bases) inside, in front and behind, the reference itself and an empty read."""
    R = len(ref)
    reads = [ref, ""]
    mid = R // 2
    reads.append(ref[:mid] + rand_seq(rng, 70) + ref[mid:])
    reads.append(ref[:mid] + ref[mid - 1:mid] * 90 + ref[mid:] if R else "A" * 90)
    reads.append(rand_seq(rng, 3) + ref)
    reads.append(ref + rand_seq(rng, 5))
    reads.append(rand_seq(rng, 80) + ref + rand_seq(rng, 66))
    for k in SPECIAL_LENGTHS:
        reads.append(noisy(rng, ref)[:k] if rng.random() < 0.5 else rand_seq(rng, k))
        reads.append((noisy(rng, ref, 0.05) * (k // max(R, 1) + 1))[:k])
    while len(reads) < n:
        reads.append(noisy(rng, ref, float(rng.choice([0.02, 0.1, 0.25]))))
    reads = reads[:n]
    order = rng.permutation(len(reads))
    reads = [reads[i] for i in order]
    quals = ["".join(chr(c) for c in rng.integers(33 + 2, 33 + 41, len(r))) for r in reads]
    return reads, quals


# name -> (reference, number of reads); the references reach k_align's 8- and 16-lane shapes (40, 130 columns),
# k_align_wide_q (1 100), a run across a 64-character step (70 equal bases) and a reference that starts / ends in a run
def cases():
    rng = np.random.default_rng(20240611)
    out = {}
    out["r40"] = (rich_reference(rng, 40), 300)
    out["r130"] = (rich_reference(rng, 130), 300)
    out["r1100"] = (rich_reference(rng, 1100), 48)
    out["run70"] = (rich_reference(rng, 30) + "G" * 70 + rich_reference(rng, 25), 200)
    out["starts_in_run"] = ("TTTT" + rich_reference(rng, 56), 200)
    out["ends_in_run"] = (rich_reference(rng, 57) + "CCC", 200)
    return {k: (ref, *make_reads(np.random.default_rng(len(ref) + n), ref, n)) for k, (ref, n) in out.items()}


def chain_expected(oracle, oenc, ref, reads, quals, go=5, ge=1):
    """The oracle chain: (scores, edits, errorFinder result, homopolymerMatcher result), lists not folded."""
    scores, edits, aref, aqry = oracle.general_align(reads, quals, oenc, go, ge, ref, False)
    with oracle_generics(oracle) as g:
        return scores, edits, g.errorFinder(aref, aqry), g.homopolymerMatcher(aref, aqry)


def plain(x):
    """Nested results as plain Python values, for == between histogram / list forms."""
    if isinstance(x, dict):
        return {k: plain(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [plain(v) for v in x]
    if isinstance(x, np.ndarray):
        return x.tolist()
    if isinstance(x, np.generic):
        return x.item()
    return x
