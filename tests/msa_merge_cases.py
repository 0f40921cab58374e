"""Inputs that steer the merge of MSA spec v2 (sarlacc_amd/csrc/msa2.hip k_m2_group) onto
the paths that random clusters of one or a few molecules do not reach, shared by tests/test_oracle_msa2_merge.py (CPU: what the
CPU statement, oracle/msa2.c, does on them) and tests/test_gpu_msa_merge.py (GPU: the kernels against it, with the library's
counters showing which path ran).

A group is a list of reads; `flatten` turns groups into what quick_msa takes.  Every builder is deterministic."""
import numpy as np

from tests.msa_score_cases import flatten, random_read, rows_spell   # noqa: F401  (re-exported for the two test files)

DEFAULT = (0, -1, -5, -1, 100)        # the reference's default call as the aligner sees it, bandwidth 100
GAPS_ONLY = (1, -50, -1, -1, 250)     # gaps beat mismatches: unrelated bases never pair; weights stay 1 (match, mismatch <= 1)

RING_REACH = 510                      # the chain kernel's ring: M2_QW - 2 columns behind the front (oracle/msa2.c MSA2_RING_REACH)

SWEEP_SIZES = (2, 3, 11, 12, 13, 23, 24, 25, 31, 32, 33, 63, 64)
SWEEP_LENGTHS = (1, 5, 63, 64, 65, 129)
# sizes on the two sides of a class boundary of the merge go into one call: 12 | 13 reads (choice of the extension kernel),
# 24 | 25 (one wavefront per group | eight), 32 | 33 (32-bit | 64-bit member sets, eight | four wavefronts)
SWEEP_CALLS = ((2,), (3,), (11,), (12, 13), (23,), (24, 25), (31,), (32, 33), (63,), (64,))


def split(S, extra=0, prefix=0, seed=600):
    """[V, U, U + V] (+ `extra` further copies of U + V) with U, V independent random reads of S bases, for DEFAULT.
    The guide tree joins V with U first; in the join of that profile with U + V, column i holds V_i, whose partner is column
    S + i of the second child, and U_i, whose partner is column i: every row has one match S columns behind the front of the
    chain -- from the first row on.
    With `prefix` > 0 all reads start with the same random P of that many bases: [P + V, P + U, P + U + V].  The rows of P have
    one match each, on the diagonal (the library of a base of P names the same position directly and through the third read), so
    the chain is `prefix` rows into the join, with predecessors written and columns entered, when the first row of the split
    comes."""
    rng = np.random.default_rng(seed + S)
    U, V = random_read(rng, S), random_read(rng, S)
    P = random_read(rng, prefix)
    return [P + V, P + U, P + U + V] + [P + U + V] * extra


def homopolymers(L, extra=()):
    """["A" * L, "C" * L, "G" * L, "T" * L] + extra, for GAPS_ONLY: no two bases of different reads pair, every join of the
    four has an empty match list and the alignment is exactly 4 L columns wide -- against a first-pass profile capacity of
    min(4 L, 3 L + 64) columns: L = 64 fits at equality, L = 65 exceeds it by one column in the last join."""
    return ["A" * L, "C" * L, "G" * L, "T" * L] + list(extra)


def six_read_overflow():
    """homopolymers(100) with "AC" * 50 and "GT" * 50: joins of 50 and 100 matches, and a profile that outgrows the first-pass
    capacity (3 * 100 + 64 columns) before the last join."""
    return homopolymers(100, extra=("AC" * 50, "GT" * 50))


def ordinary(seed, n=6, length=150, sub=0.05, indel=0.01):
    """n reads of one random molecule: the clusters the merge is built for"""
    from sarlacc_amd.mock import NUC, mutate
    rng = np.random.default_rng(seed)
    t = NUC[rng.integers(0, 4, length)]
    return [mutate(t, rng, sub, indel).tobytes().decode() for _ in range(n)]


def sweep(size):
    """The groups of `size` reads of the boundary sweep, for DEFAULT: per molecule length of SWEEP_LENGTHS a group of one
    molecule and a group of two molecules with members alternating; 5 % substitutions, 2 % indel events (molecules of 1 and 5
    bases leave a few reads empty, which is wanted).  Returns [(length, molecules, group)]."""
    from sarlacc_amd.mock import NUC, mutate
    rng = np.random.default_rng(7000 + size)
    out = []
    for length in SWEEP_LENGTHS:
        for nmol in (1, 2):
            truths = [NUC[rng.integers(0, 4, length)] for _ in range(nmol)]
            out.append((length, nmol, [mutate(truths[k % nmol], rng, 0.05, 0.02).tobytes().decode() for k in range(size)]))
    return out


_REFERENCE = {}


def reference(oracle, key, read_groups, params, max_columns=65535):
    """(rows per group, oracle.msa2_stats() of exactly this call) of the CPU statement under spec v2, computed once per `key`
    and shared by the tests of a session.  Callers must not modify what they get."""
    if key not in _REFERENCE:
        reads, groups = flatten(read_groups)
        oracle.msa2_stats()
        rows = oracle.quick_msa(groups, reads, *params, spec=2, max_columns=max_columns)
        _REFERENCE[key] = (rows, oracle.msa2_stats())
    return _REFERENCE[key]
