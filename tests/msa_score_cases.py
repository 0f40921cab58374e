"""Scoring parameter sets and read builders shared by tests/test_oracle_msa_scores.py (CPU: oracle/msa.c against an
independent DP) and tests/test_gpu_msa_scores.py (GPU: the pairwise kernels against the oracle).

A set is (match, mismatch, gap_extension, gap_opening), the .Call order of quick_msa: a gap of length k scores
gap_opening + (k - 1) * gap_extension."""
import numpy as np

NUC = np.frombuffer(b"ACGT", dtype=np.uint8)
MSA_MAXBAND = 1024   # band cap of both specs

# name -> scores.  The comments name the pairwise kernel the set is there for (tests/test_gpu_msa_scores.py asserts it by
# the library's counters; at bandwidth 100 unless said otherwise).
SETS = {
    "default": (0, -1, -5, -1),                 # bit-vector
    "linear": (0, -1, -1, -1),                  # every edit alike: bit-vector up to 256 diagonals, packed with linear gaps beyond
    "near_bound": (0, -20, -20, -20),           # every edit alike: bit-vector; with that kernel off packed, linear, spread 10 860 of 11 000
    "near_bound_first_cheaper": (0, -20, -20, -19),   # not unit-like: packed, linear on the product route, spread 10 859
    "one_cost_more": (0, -21, -21, -21),        # 32-bit: spread 11 403
    "affine_match5": (5, -4, -6, -8),           # packed, affine, costs doubled (18 / 21 / 17): spread 10 927 at 228 diagonals
    "mixed": (0, -4, -6, -8),                   # packed up to 988 diagonals, 32-bit beyond
    "mismatch_above_match": (1, 2, -3, -3),     # outside the cost domain: 32-bit
    "cost_5000": (0, -5000, -5000, -5000),      # doubled cost beyond 4 000: 32-bit
    "match_1000": (1000, -1000, -3000, -2000),  # 32-bit
    "positive_extension": (0, -3, 1, -5),       # a positive gap score: 32-bit
}
FRACTIONAL = ((1.9, -2.9, -2.5, -2.5), (1, -2, -2, -2))   # truncated toward zero on both sides


def pair_bandwidth(bandwidth, lr, lc):
    """The band cap (oracle/msa.c orc_msa_pairwise, msa_common.hpp msa_pair_bandwidth): the pair's own bandwidth, -1 for
    the diagonal alignment of reads differing by 1 024 bases or more."""
    dl = abs(lc - lr)
    if dl + 2 * bandwidth + 1 <= MSA_MAXBAND:
        return bandwidth
    return (MSA_MAXBAND - 1 - dl) // 2 if MSA_MAXBAND - 1 - dl >= 0 else -1


def dna5(s):
    return "".join(c if c in "ACGT" else "N" for c in s.upper())


def random_read(rng, n):
    return NUC[rng.integers(0, 4, n)].tobytes().decode()


def mutate(read, rng, sub, indel):
    """Substitutions at rate `sub`, insertions and deletions at rate `indel` / 2 each."""
    out = []
    for ch in read:
        u = rng.random()
        if u < indel / 2:
            continue
        if u < indel:
            out.append("ACGT"[int(rng.integers(0, 4))])
        out.append("ACGT"[int(rng.integers(0, 4))] if rng.random() < sub else ch)
    return "".join(out)


def related_pair(rng, length, diff, sub=0.08, indel=0.03):
    """Two reads of one template at `sub` substitutions and `indel` indels, the second exactly `diff` bases longer."""
    t = random_read(rng, length + diff + 40)
    a = mutate(t[:length], rng, sub, indel)
    b = mutate(t, rng, sub, indel)[:len(a) + diff]
    assert len(b) == len(a) + diff
    return a, b


def same_length_group(rng, n, length, sub=0.08):
    """n reads of one template, all `length` bases: substitutions, and one insertion paired with one deletion each."""
    t = random_read(rng, length)
    reads = []
    for _ in range(n):
        r = list(mutate(t, rng, sub, 0.0))
        i, j = sorted(int(x) for x in rng.integers(1, length - 1, 2))
        del r[i]
        r.insert(j, "ACGT"[int(rng.integers(0, 4))])
        reads.append("".join(r))
    return reads


def edge_groups(rng, bandwidth, length=90):
    """Groups where a carry between packed halves or a wrong clamp would show: unrelated reads, poly-A against poly-C, a read
    against itself with bandwidth - 1 bases deleted, homopolymer runs (ties), N and lower case, an empty read."""
    r = random_read(rng, length + bandwidth)
    cut = length // 3
    runs = "".join(c * int(k) for c, k in zip("ACGTTGCAAC" * 2, rng.integers(3, 9, 20)))
    runs2 = "".join(c * int(k) for c, k in zip("ACGTTGCAAC" * 2, rng.integers(3, 9, 20)))
    mixed = mutate(r[:length], rng, 0.05, 0.02)
    noisy = mixed[:10] + "N" + mixed[11:30].lower() + "NN" + mixed[32:50] + "r" + mixed[51:]
    return [
        [random_read(rng, length), random_read(rng, length - 3)],
        ["A" * length, "C" * length],
        ["A" * length, "A" * (length - 7), "C" * 5 + "A" * (length - 20)],
        [r, r[:cut] + r[cut + max(bandwidth - 1, 0):]],
        [runs, runs2, mutate(runs, rng, 0.05, 0.05)],
        [mixed, noisy, mixed.lower()],
        ["", r[:40]],
        [r[:25], "", ""],
    ]


def flatten(read_groups):
    """lists of reads -> (reads, 1-based group lists) as quick_msa takes them"""
    reads, groups = [], []
    for g in read_groups:
        groups.append(list(range(len(reads) + 1, len(reads) + len(g) + 1)))
        reads.extend(g)
    return reads, groups


def rows_spell(rows_per_group, reads, groups):
    for rows, g in zip(rows_per_group, groups):
        assert len(rows) == len(g) and len({len(r) for r in rows}) <= 1
        for row, i in zip(rows, g):
            if len(g) == 1:
                assert row == reads[i - 1]          # singleton groups verbatim
            else:
                assert row.replace("-", "") == dna5(reads[i - 1])
