"""profileReads on the GPU (sarlacc_profile_reads / sarlacc_dev_profile_reads / sarlacc_profile_fetch,
profile_reads.hip) against the CPU oracle chain general_align -> find_errors + match_homopolymers and against the
existing GPU chain qualityAlign -> errorFinder + homopolymerMatcher.  Integers and score bit patterns: exact."""
import ctypes as C

import numpy as np
import pytest

from tests.encodings import BY_NAME, draw_quals
from tests.profile_reads_cases import DENSE, EDGE, TILE, cases, chain_expected, long_cases, noisy, phred_quals, plain, stride_case

pytestmark = pytest.mark.gpu

CASES = cases()


@pytest.fixture(scope="module")
def expected(oracle, oenc):
    """Per case the oracle chain's (scores, edits, errors, homopolymers), computed once and only read."""
    return {name: chain_expected(oracle, oenc, ref, reads, quals) for name, (ref, reads, quals) in CASES.items()}


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.int64).tolist()


def same_profile(got, scores, edits, errors, homopolymers, generics, folded=True):
    if folded:
        errors, homopolymers = generics.foldProfile(errors, homopolymers)
    assert plain(got["errors"]) == plain(errors)
    assert plain(got["homopolymers"]) == plain(homopolymers)
    assert bits(got["score"]) == bits(scores) and np.asarray(got["edit"]).tolist() == np.asarray(edits).tolist()


@pytest.mark.parametrize("name", sorted(CASES))
def test_against_the_oracle_chain_and_the_gpu_chain(name, expected, enc):
    from sarlacc_amd import calls, generics
    from sarlacc_amd.resident import DeviceReads
    ref, reads, quals = CASES[name]
    scores, edits, errors, homopolymers = expected[name]
    rd = generics.Reads(reads, quals)
    host = generics.profileReads(rd, ref)
    same_profile(host, scores, edits, errors, homopolymers, generics)
    ga = calls.general_align(reads, quals, enc, 5, 1, ref, True)
    assert bits(host["score"]) == bits(ga[0]) and host["edit"].tolist() == ga[1].tolist()
    dev = DeviceReads.upload(rd)
    same_profile(generics.profileReads(dev, ref), scores, edits, errors, homopolymers, generics)
    # expand=True: value for value what the two generics give for qualityAlign's strings
    qa = generics.qualityAlign(rd, ref)
    expanded = generics.profileReads(dev, ref, expand=True)
    same_profile(expanded, qa["score"], qa["edit"], generics.errorFinder(qa["reference"], qa["query"]),
                 generics.homopolymerMatcher(qa["reference"], qa["query"]), generics, folded=False)
    # the reads cover what they are meant to
    n = len(reads)
    ins = host["errors"]["full"]["insertion"]
    assert max(int(l.max()) for l, _ in ins) > 64 and ins[0][0].max() > 0 and ins[len(ref)][0].max() > 0
    assert "" in reads and ref in reads and all(int(m.sum()) == n for _, m in ins)
    if name == "run70":
        assert any(h["end"] - h["start"] + 1 >= 70 and int(h["observed"][0].max()) >= 64 for h in host["homopolymers"])


def test_chunks(expected):
    import sarlacc_amd
    from sarlacc_amd import calls, generics
    from sarlacc_amd.resident import DeviceReads
    ref, reads, quals = CASES["r130"]
    n = len(reads)
    dev = DeviceReads.upload(generics.Reads(reads, quals))
    try:
        for chunk, want in ((1, n), (7, (n + 6) // 7), (n, 1)):
            calls.set_option("profile_chunk_reads", chunk)
            same_profile(generics.profileReads(dev, ref), *expected["r130"], generics)
            assert sarlacc_amd.stage_count("profile_chunks") == want
            assert sarlacc_amd.stage_ms("profile_align") >= 0 and sarlacc_amd.stage_ms("profile_reduce") >= 0
    finally:
        calls.set_option("profile_chunk_reads", 0)
    same_profile(generics.profileReads(dev, ref), *expected["r130"], generics)
    assert sarlacc_amd.stage_count("profile_chunks") == 1


def test_another_encoding(oracle):
    from sarlacc_amd import calls, generics
    t = BY_NAME["n60_high"]   # 60 names from byte 160: a negative offset, characters past the last entry clamp
    ref, reads, _ = CASES["r40"]
    quals = draw_quals(t, [len(r) for r in reads], seed=3)
    got = generics.profileReads(generics.Reads(reads, quals, encoding=t.enc), ref)
    ga = calls.general_align(reads, quals, t.enc, 5, 1, ref, True)
    assert bits(got["score"]) == bits(ga[0]) and got["edit"].tolist() == ga[1].tolist()
    same_profile(got, *chain_expected(oracle, t.oenc, ref, reads, quals), generics)


def test_no_reads_and_no_reference(oracle):
    from sarlacc_amd import generics
    ref = CASES["r40"][0]
    got = generics.profileReads(generics.Reads([], []), ref)
    full = got["errors"]["full"]
    assert all(full[k] == [0] * len(ref) + [None] for k in ("A", "C", "G", "T", "deletion")) and full["base"] == list(ref) + [None]
    assert len(full["insertion"]) == len(ref) + 1 and all(l.size == 0 and m.size == 0 for l, m in full["insertion"])
    runs = oracle.find_homopolymers([ref])
    assert [(h["start"], h["end"], h["base"]) for h in got["homopolymers"]] == \
        [(int(p), int(p + w - 1), b) for p, w, b in zip(runs[1], runs[2], runs[3])]
    assert all(h["observed"][0].size == 0 for h in got["homopolymers"]) and got["score"].size == 0 and not got["errors"]["transition"].any()
    # an empty reference: no counts, every (non-empty) read one insertion at position 0
    reads = ["ACGT", "", "GG", "ACGT" * 20, "TT"]
    got = generics.profileReads(generics.Reads(reads, ["5" * len(r) for r in reads]), "")
    assert got["errors"]["full"]["A"] == [None] and got["homopolymers"] == []
    assert plain(got["errors"]["full"]["insertion"]) == [[[0, 2, 4, 80], [1, 2, 1, 1]]]
    assert got["edit"].tolist() == [4, 0, 2, 80, 2]


def test_errors_are_the_chains(enc):
    from sarlacc_amd import SarlaccError, calls, generics
    ref, reads, quals = CASES["r40"]
    reads, quals = list(reads[:40]), list(quals[:40])
    k = next(i for i, r in enumerate(reads) if r == ref)
    bad = list(reads)
    bad[k] = ref[:7] + "N" + ref[8:]
    with pytest.raises(SarlaccError, match="unknown character 'N'") as chain:
        qa = generics.qualityAlign(generics.Reads(bad, quals), ref)
        generics.errorFinder(qa["reference"], qa["query"])
    with pytest.raises(SarlaccError, match="unknown character 'N'") as fused:
        generics.profileReads(generics.Reads(bad, quals), ref)
    assert str(fused.value) == str(chain.value)
    # what general_align raises comes first, with its message
    for rf, rd, q in ((ref[:5] + "!" + ref[6:], bad, quals), (ref, bad, [x.replace(x[:1], " ", 1) if x else x for x in quals])):
        with pytest.raises(SarlaccError) as chain:
            calls.general_align(rd, q, enc, 5, 1, rf, False)
        with pytest.raises(SarlaccError) as fused:
            calls.profile_reads(rd, q, enc, 5, 1, rf)
        assert str(fused.value) == str(chain.value)
    assert "reference" in str(chain.value) or "quality" in str(chain.value)


def test_fetch_with_a_short_capacity(enc):
    from sarlacc_amd import SarlaccError, _lib, calls
    ref, reads, quals = CASES["r40"]
    raw = calls.profile_reads(reads, quals, enc, 5, 1, ref)
    ni, nr, no = raw["ins_pos"].size, len(raw["run_base"]), raw["obs_run"].size
    assert ni > 1 and nr > 0 and no > 1
    arrays = [np.full((5, len(ref)), -7, np.int32)] + [np.full(ni, -7, t) for t in (np.int32, np.int32, np.int64)] + \
        [np.full(nr, -7, np.int32), np.full(nr, -7, np.int32), np.full(nr, 249, np.uint8)] + [np.full(no, -7, t) for t in (np.int32, np.int32, np.int64)]
    a = arrays
    for caps in ((ni - 1, nr, no), (ni, nr - 1, no), (ni, nr, no - 1)):
        with pytest.raises(SarlaccError, match="too small"):
            _lib.check(_lib.lib().sarlacc_profile_fetch(a[0], a[1], a[2], a[3], caps[0], a[4], a[5], a[6], caps[1], a[7], a[8], a[9], caps[2]))
        assert all((x == (249 if x.dtype == np.uint8 else -7)).all() for x in arrays)
    _lib.check(_lib.lib().sarlacc_profile_fetch(a[0], a[1], a[2], a[3], ni, a[4], a[5], a[6], nr, a[7], a[8], a[9], no))
    assert a[0].tolist() == raw["counts"].tolist() and a[3].tolist() == raw["ins_mult"].tolist() and a[9].tolist() == raw["obs_mult"].tolist()


def test_several_references():
    from sarlacc_amd import generics
    from sarlacc_amd.resident import DeviceReads
    names = ("r40", "starts_in_run", "ends_in_run")
    refs = [CASES[k][0] for k in names]
    reads, quals, assignment = [], [], []
    for j, k in enumerate(names):
        reads += CASES[k][1][:50]; quals += CASES[k][2][:50]; assignment += [j] * 50
    rng = np.random.default_rng(11)
    assignment = np.array(assignment)
    assignment[rng.choice(assignment.size, 20, replace=False)] = -1
    order = rng.permutation(assignment.size)
    reads, quals, assignment = [reads[i] for i in order], [quals[i] for i in order], assignment[order]
    rd = generics.Reads(reads, quals)
    parts = generics.profileReads(DeviceReads.upload(rd), refs, assignment=assignment)
    assert len(parts) == 3
    for j, part in enumerate(parts):
        alone = generics.profileReads(rd.subset(np.flatnonzero(assignment == j)), refs[j])
        assert plain(part) == plain(alone)
    assert plain(generics.profileReads(rd, refs, assignment=assignment)) == plain(parts)


# ---- beyond one tile of reference positions (2 048), beyond one sweep of the persistent grid, and where the dense
# ---- table of event lengths ends and the list begins (64)
LONG = long_cases()


@pytest.fixture(scope="module")
def long_expected(oracle, oenc):
    return {name: chain_expected(oracle, oenc, ref, reads, quals) for name, (ref, reads, quals) in LONG.items()}


def edge_rows(rows, lengths):
    """the rows that hold the lengths 63, 64 and 65"""
    rows, lengths = np.asarray(rows), np.asarray(lengths)
    return sorted(int(r) for r in np.unique(rows) if set(EDGE) <= set(lengths[rows == r].tolist()))


@pytest.mark.parametrize("name", sorted(LONG, key=lambda k: int(k[1:])))
def test_tile_edge(name, long_expected):
    from sarlacc_amd import generics
    from sarlacc_amd.resident import DeviceReads
    ref, reads, quals = LONG[name]
    R = len(ref)
    scores, edits, errors, homopolymers = long_expected[name]
    # what the comparison is about, on the expected side: insertions of 63, 64 and 65 bases at the start, beyond the tile
    # edge and behind the last base; a run beyond the edge observed with 63, 64 and 65 bases; a run across the edge
    ins = errors["full"]["insertion"]
    assert len(ins) == R + 1 and sum(errors["full"]["deletion"][2000:min(2100, R)]) >= min(2100, R) - 2000
    at = [p for p in range(R + 1) if set(EDGE) <= set(ins[p])]
    assert min(at) <= 1 and max(at) == R and (R <= TILE or any(TILE <= p < R for p in at)), at
    seen = [h["start"] for h in homopolymers if set(EDGE) <= set(h["observed"])]
    assert len(seen) >= 3 and (R < 4100 or any(s - 1 > TILE for s in seen)), seen
    if R > TILE:
        assert R == int(name[1:]) and any(h["start"] - 1 <= TILE - 4 and h["end"] > TILE and h["base"] == "G" for h in homopolymers)
    rd = generics.Reads(reads, quals)
    same_profile(generics.profileReads(rd, ref), scores, edits, errors, homopolymers, generics)
    dev = DeviceReads.upload(rd)
    same_profile(generics.profileReads(dev, ref), scores, edits, errors, homopolymers, generics)
    qa = generics.qualityAlign(rd, ref)
    same_profile(generics.profileReads(dev, ref, expand=True), qa["score"], qa["edit"], generics.errorFinder(qa["reference"], qa["query"]),
                 generics.homopolymerMatcher(qa["reference"], qa["query"]), generics, folded=False)


def test_dense_table_and_list_on_one_row(enc, long_expected):
    """lengths 63 (dense table), 64 and 65 (list) of one position / one run come out side by side, in ascending order"""
    from sarlacc_amd import calls, generics
    ref, reads, quals = LONG["r4100"]
    errors, homopolymers = generics.foldProfile(*long_expected["r4100"][2:])
    raw = calls.profile_reads(reads, quals, enc, 5, 1, ref)
    for rows, lengths, mult, want in ((raw["ins_pos"], raw["ins_len"], raw["ins_mult"], [(p, v) for p, v in enumerate(errors["full"]["insertion"])]),
                                      (raw["obs_run"], raw["obs_len"], raw["obs_mult"], [(k, h["observed"]) for k, h in enumerate(homopolymers)])):
        found = edge_rows(rows, lengths)
        assert found and found[-1] > 0
        for r in found:
            mine = np.flatnonzero(rows == r)
            assert (np.diff(mine) == 1).all() and (np.diff(lengths[mine]) > 0).all()
            l, m = dict(want)[r]
            keep = np.asarray(l) > 0 if rows is raw["ins_pos"] else np.ones(len(l), bool)   # (no insertion: no event)
            assert lengths[mine].tolist() == np.asarray(l)[keep].tolist() and mult[mine].tolist() == np.asarray(m)[keep].tolist()
        assert (np.diff(rows) >= 0).all() and (mult > 0).all()


def test_tile_edge_in_chunks(long_expected):
    import sarlacc_amd
    from sarlacc_amd import calls, generics
    from sarlacc_amd.resident import DeviceReads
    name = "r%d" % (TILE + 1)
    ref, reads, quals = LONG[name]
    n = len(reads)
    dev = DeviceReads.upload(generics.Reads(reads, quals))
    try:
        for chunk, want in ((1, n), (7, (n + 6) // 7)):
            calls.set_option("profile_chunk_reads", chunk)
            same_profile(generics.profileReads(dev, ref), *long_expected[name], generics)
            assert sarlacc_amd.stage_count("profile_chunks") == want
    finally:
        calls.set_option("profile_chunk_reads", 0)


def test_grid_stride(oracle, oenc):
    """more alignments than one sweep of the persistent grid (4 x CUs workgroups of 8): every wavefront walks a second
    alignment into the same counters, and a list event comes with a multiplicity"""
    import torch
    from sarlacc_amd import calls, generics
    from sarlacc_amd.resident import DeviceReads
    n = 32 * torch.cuda.get_device_properties(0).multi_processor_count + 300
    ref, reads, quals, inserted = stride_case(n)
    scores, edits, errors, homopolymers = chain_expected(oracle, oenc, ref, reads, quals)
    shared = reads.count(inserted)
    events = [(p, l, v.count(l)) for p, v in enumerate(errors["full"]["insertion"]) for l in sorted(set(v)) if l >= DENSE]
    assert shared > 1 and len(events) == 1 and events[0][1] >= 70 - 2 and events[0][2] == shared, events
    rd = generics.Reads(reads, quals)
    same_profile(generics.profileReads(rd, ref), scores, edits, errors, homopolymers, generics)
    same_profile(generics.profileReads(DeviceReads.upload(rd), ref), scores, edits, errors, homopolymers, generics)
    raw = calls.profile_reads(reads, quals, rd.encoding, 5, 1, ref)
    k = np.flatnonzero(raw["ins_len"] >= DENSE)
    assert [(int(raw["ins_pos"][j]), int(raw["ins_len"][j]), int(raw["ins_mult"][j])) for j in k] == events
    assert int(raw["counts"].sum()) == len(ref) * n


def outcome(f):
    from sarlacc_amd import SarlaccError
    try:
        return ("value", f())
    except SarlaccError as e:
        return ("error", str(e))


def test_error_order_across_tiles():
    """the unknown character the chain meets first: by alignment, then by position from the front -- while the walk goes from
    the back and each tile sees its own positions only"""
    from sarlacc_amd import generics
    ref = LONG["r4100"][0]
    rng = np.random.default_rng(4100)
    reads = [noisy(rng, ref, 0.02) for _ in range(6)] + [""]
    quals = phred_quals(rng, reads)

    def put(s, k, c):
        return s[:k] + c + s[k + 1:]

    def chain(rd):
        qa = generics.qualityAlign(rd, ref)
        return plain([generics.errorFinder(qa["reference"], qa["query"]), generics.homopolymerMatcher(qa["reference"], qa["query"])])

    def fused(rd):
        got = generics.profileReads(rd, ref, expand=True)
        return plain([got["errors"], got["homopolymers"]])
    mid = reads[2][:2500] + "ACGTANACGT" + reads[2][2500:]   # (ten bases the reference does not hold there: an insertion)
    for bad, letter in (([put(r, 3000, "R") if i == 3 else put(r, 10, "N") if i == 5 else r for i, r in enumerate(reads)], "R"),
                        ([put(put(r, 3000, "N"), 100, "R") if i == 4 else r for i, r in enumerate(reads)], "R"),
                        ([put(r, len(r) - 5, "N") if i == 1 else put(r, 2, "R") if i == 2 else r for i, r in enumerate(reads)], "N"),
                        ([mid if i == 2 else r for i, r in enumerate(reads)], None)):
        q = [x if len(x) == len(r) else x[:2500] + "5" * 10 + x[2500:] for x, r in zip(quals, bad)]
        rd = generics.Reads(bad, q)
        want, got = outcome(lambda: chain(rd)), outcome(lambda: fused(rd))
        assert got == want
        if letter:
            assert want == ("error", "unknown character '%s' in alignment string" % letter)


def test_several_references_with_different_tile_counts():
    from sarlacc_amd import generics
    from sarlacc_amd.resident import DeviceReads
    names = ("r40", "r%d" % (TILE + 1), "r4100")
    sets = [CASES["r40"]] + [LONG[k] for k in names[1:]]
    refs = [s[0] for s in sets]
    assert [(len(r) + TILE - 1) // TILE for r in refs] == [1, 2, 3]
    reads, quals, assignment = [], [], []
    for j, (_, rds, qs) in enumerate(sets):
        reads += rds[:20]; quals += qs[:20]; assignment += [j] * 20
    order = np.random.default_rng(12).permutation(len(reads))
    reads, quals, assignment = [reads[i] for i in order], [quals[i] for i in order], np.array(assignment)[order]
    rd = generics.Reads(reads, quals)
    parts = generics.profileReads(DeviceReads.upload(rd), refs, assignment=assignment)
    assert len(parts) == 3
    for j, part in enumerate(parts):
        assert plain(part) == plain(generics.profileReads(rd.subset(np.flatnonzero(assignment == j)), refs[j]))
