"""profileReads exists at every layer that needs no device -- declared in include/sarlacc_amd.h, bound in
sarlacc_amd._lib.PROTOTYPES, reachable from the package -- and its host helpers (lists <-> histograms) are inverse to
each other on the CPU oracle chain's output and on the literal cases of the reference's profiling tests."""
import ctypes as C

import numpy as np

from sarlacc_amd import _lib, calls, generics
from sarlacc_amd.resident import DeviceReads
from tests.abi_text import _header_decls
from tests.profile_cases import ERROR_CASES, MATCH_CASES
from tests.profile_reads_cases import cases, chain_expected, oracle_generics, plain

NAMES = ("sarlacc_dev_profile_reads", "sarlacc_profile_fetch", "sarlacc_profile_reads")


def test_declared_and_bound():
    decls = _header_decls()
    for name in NAMES:
        assert name in decls, name + " is not declared in the header"
        assert name in _lib.PROTOTYPES, name + " is not in the prototype table"
        assert decls[name][0] == "int" and _lib.PROTOTYPES[name][0] is C.c_int
    dev = decls["sarlacc_dev_profile_reads"][1]
    assert dev[3:5] == [("int64_t", "n"), ("int32_t", "max_len")] and dev[-1] == ("void*", "stream")
    assert dev[-6:-1] == [("double*", "d_scores"), ("int32_t*", "d_edits"), ("int64_t*", "n_ins"), ("int64_t*", "n_hp_runs"), ("int64_t*", "n_hp_obs")]
    fetch = decls["sarlacc_profile_fetch"][1]
    assert [p for p in fetch if p[1].startswith("cap_")] == [("int64_t", "cap_ins"), ("int64_t", "cap_runs"), ("int64_t", "cap_obs")]
    assert fetch[0] == ("int32_t*", "counts") and ("int64_t*", "ins_mult") in fetch and ("int64_t*", "obs_mult") in fetch
    host = decls["sarlacc_profile_reads"][1]
    assert [p[1] for p in host[:5]] == ["seq", "seq_off", "qual", "qual_off", "n"] and [p[1] for p in host[-3:]] == ["n_ins", "n_hp_runs", "n_hp_obs"]


def test_python_entry_points():
    assert callable(calls.profile_reads) and callable(DeviceReads.profile) and callable(generics.profileReads)
    for f in (generics.foldLengths, generics.expandLengths, generics.foldProfile, generics.expandProfile):
        assert callable(f)


def test_lengths_round_trip():
    lengths, mult = generics.foldLengths([0, 0, 3, 1, 3, 3, 70])
    assert lengths.tolist() == [0, 1, 3, 70] and mult.tolist() == [2, 1, 3, 1] and lengths.dtype == np.int32 and mult.dtype == np.int64
    assert generics.expandLengths((lengths, mult)) == [0, 0, 1, 3, 3, 3, 70]
    assert generics.expandLengths(generics.foldLengths([])) == []


def check_round_trip(errors, homopolymers, n):
    fe, fh = generics.foldProfile(errors, homopolymers)
    assert plain(generics.expandProfile(fe, fh)) == plain((errors, homopolymers))
    for lengths, mult in fe["full"]["insertion"]:
        assert int(mult.sum()) == n and (np.diff(lengths) > 0).all()
        # the multiplicity of length 0 is n minus the others'
        zero = int(mult[lengths == 0].sum())
        assert zero == n - int(mult[lengths != 0].sum())
    for h in fh:
        assert int(h["observed"][1].sum()) == n


def test_round_trip_on_the_oracle_chain(oracle, oenc):
    ref, reads, quals = cases()["r40"]
    _, _, errors, homopolymers = chain_expected(oracle, oenc, ref, reads[:60], quals[:60])
    assert any(any(v) for v in errors["full"]["insertion"]) and homopolymers
    check_round_trip(errors, homopolymers, 60)


def test_round_trip_on_the_literal_cases(oracle):
    with oracle_generics(oracle) as g:
        for reads, refs in ERROR_CASES:
            for rd, rf in zip(reads, refs):   # (the literal references differ from pair to pair)
                check_round_trip(g.errorFinder([rf], [rd]), g.homopolymerMatcher([rf], [rd]), 1)
        for reads, refs in MATCH_CASES:
            if len({r.replace("-", "") for r in refs}) == 1 and all(set(r) <= set("ACGT-") for r in reads):
                check_round_trip(g.errorFinder(refs, reads), g.homopolymerMatcher(refs, reads), len(refs))
