"""CPU tests of the host-side logic (no GPU): string-set plumbing, the R-generic
counterparts' pure logic, the mock generator, the C-ABI surface, and the
fail-loudly-without-a-GPU contract."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_exports_every_declared_symbol():
    hdr = open(os.path.join(ROOT, "include", "sarlacc_amd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    names = set(re.findall(r"\b(sarlacc_[a-z0-9_]+)\s*\(", hdr))
    assert len(names) >= 19
    so = os.path.join(ROOT, "sarlacc_amd", "libsarlacc_amd.so")
    if not os.path.exists(so):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(so)
    missing = [n for n in sorted(names) if not hasattr(lib, n)]
    assert not missing, missing


def test_product_fails_loudly_without_gpu():
    import sarlacc_amd
    from sarlacc_amd import calls
    if sarlacc_amd.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(sarlacc_amd.SarlaccError, match="no HIP device"):
        calls.adaptor_align(["ACGT"], ["IIII"], sarlacc_amd.phred_encoding(), 5, 1, "ACG", [], [])
    with pytest.raises(sarlacc_amd.SarlaccError, match="no HIP device"):
        calls.umi_group(["ACGT", "ACGA"], 1, None, 1, [[1, 2]])
    with pytest.raises(sarlacc_amd.SarlaccError, match="no HIP device"):
        calls.create_consensus_basic(["ACGT"], 0.6, 1)
    with pytest.raises(sarlacc_amd.SarlaccError, match="no HIP device"):
        calls.quick_msa([[1, 2]], ["ACGT", "ACGA"], 0, -1, -5, -1, 100)


def test_product_never_imports_the_oracle():
    """The shipped package may mention the oracle in comments, but must not import, include,
    link or call it."""
    pkg = os.path.join(ROOT, "sarlacc_amd")
    for base, _, files in os.walk(pkg):
        for f in files:
            path = os.path.join(base, f)
            if f.endswith(".py"):
                txt = open(path).read()
                assert not re.search(r"^\s*(from|import)\s+oracle", txt, flags=re.M), f
                assert "liboracle" not in txt, f
            elif f.endswith((".hip", ".cpp", ".hpp", ".h")):
                txt = open(path).read()
                assert not re.search(r"#include\s+[<\"][^>\"]*oracle", txt), f
                assert not re.search(r"\borc_[a-z0-9_]+\s*\(", txt), f
    mk = open(os.path.join(pkg, "csrc", "Makefile")).read()
    assert "oracle" not in mk


def test_stringset_roundtrip_and_subset():
    from sarlacc_amd.strset import StringSet, csr_from_lists, lists_from_csr
    strs = ["ACGT", "", "A", "GGGTTT"]
    ss = StringSet.from_strings(strs)
    assert ss.to_strings() == strs and len(ss) == 4 and ss.total == 11
    assert ss.subset([3, 0, 1]).to_strings() == ["GGGTTT", "ACGT", ""]
    assert StringSet.from_strings([]).to_strings() == []
    off, vals = csr_from_lists([[1, 2], [], [3]])
    assert [x.tolist() for x in lists_from_csr(off, vals)] == [[1, 2], [], [3]]


def test_setup_subseqs_known_values():
    # tests/testthat/test-adaptor-align.R:124-128
    from sarlacc_amd.generics import _setup_subseqs
    for ad, (s, e) in {"AAAAGGNNNNCCTTTT": (7, 10), "AAAAGGYYYYCCTTTT": (7, 10), "AAAAGGCCTTTTRRRR": (13, 16)}.items():
        out = _setup_subseqs(ad)
        assert out["starts"].tolist() == [s] and out["ends"].tolist() == [e]
    out = _setup_subseqs("ACGT")
    assert out["starts"].size == 0 and out["ends"].size == 0
    out = _setup_subseqs("NNACGNNNT")
    assert out["starts"].tolist() == [1, 6] and out["ends"].tolist() == [2, 8]


def test_front_and_back():
    # tests/testthat/test-adaptor-align.R:130-139
    from sarlacc_amd.generics import Reads, _get_front_and_back
    from sarlacc_amd.mock import revcomp
    seqs = ["AAAAGGGGCCCCTTTT", "ACGTACGTACGTAAAAGGGGCCCCTTTT", "GGGGCCCC", ""]
    quals = ["".join(chr(40 + (i % 50)) for i in range(len(s))) for s in seqs]
    rd = Reads(seqs, quals)
    front, back = _get_front_and_back(rd, 10)
    assert front.seq.to_strings() == [s[:10] for s in seqs]
    assert [revcomp(b) for b in back.seq.to_strings()] == [s[max(0, len(s) - 10):] for s in seqs]
    assert back.qual.to_strings() == [q[max(0, len(q) - 10):][::-1] for q in quals]
    front, back = _get_front_and_back(rd, 10000)
    assert front.seq.to_strings() == seqs and [revcomp(b) for b in back.seq.to_strings()] == seqs


def test_resolve_strand():
    from sarlacc_amd.generics import _resolve_strand
    rev, sc = _resolve_strand(np.array([5.0, -3.0, 2.0]), np.array([1.0, -1.0, 2.0]),
                              np.array([2.0, 4.0, 2.0]), np.array([3.0, -9.0, 2.0]))
    assert rev.tolist() == [False, True, False] and sc.tolist() == [6.0, 4.0, 4.0]


def test_mock_reads_shape():
    from sarlacc_amd.mock import mock_reads, revcomp
    a1 = "ACGATCAGC" + "N" * 12 + "GTCAGTCAG"
    sim = mock_reads(a1, "CACACTGAGCAGCGACTAGACA", nmolecules=5, nreads=4, seqlen=300, seed=1)
    assert len(sim["reads"]) == 20 and len(sim["quals"]) == 20
    assert (sim["reads"].widths() == sim["quals"].widths()).all()
    assert all(len(u) == 12 for u in sim["umi"])
    assert abs(np.mean(sim["reads"].widths()) - 352) < 15
    assert revcomp("ACGTN") == "NACGT"


def test_encoding_vector():
    import sarlacc_amd
    enc = sarlacc_amd.phred_encoding()
    assert len(enc) == 94 and enc.names[:2] == b"!\"" and enc.errors[0] == 1.0 and abs(enc.errors[20] - 0.01) < 1e-15
    assert enc.to_error(b"!5~").tolist() == [1.0, 10 ** -2.0, 10 ** -9.3]


def test_generic_pipeline_runs_on_the_oracle(monkeypatch):
    """BASELINE config 1 (plumbing, no GPU): mockReads 1k x 1kb-shaped data through
    adaptorAlign -> umiGroup -> multiReadAlign -> consensusReadSeq with the oracle standing
    in for the HIP library.  Checks the host logic and the biology end to end."""
    from sarlacc_amd import generics
    from sarlacc_amd.mock import mock_reads
    from tests import oracle_calls
    from tests.test_oracle_umi import lev2
    monkeypatch.setattr(generics, "calls", oracle_calls)
    a1 = "ACGATCAGC" + "N" * 12 + "GTCAGTCAG"
    a2 = "CACACTGAGCAGCGACTAGACA"
    sim = mock_reads(a1, a2, nmolecules=12, nreads=8, seqlen=400, seed=1000)
    rd = generics.Reads(sim["reads"], sim["quals"], ["R%d" % i for i in range(len(sim["reads"]))])
    aln = generics.adaptorAlign(a1, a2, rd)
    assert (aln["reversed"] == sim["flipped"]).mean() > 0.95
    good = (aln["adaptor1"]["score"] > 10) & (aln["adaptor2"]["score"] > 5)
    assert good.mean() > 0.8
    # orient reads, take UMIs from the adaptor-1 section
    umis = aln["adaptor1"]["subseq"]["Sub1"]
    keep = np.flatnonzero(good)
    groups = generics.umiGroup([umis[i] for i in keep], threshold1=2)
    assert sorted(x for g in groups for x in g.tolist()) == list(range(1, len(keep) + 1))
    # clusters are (almost) pure with respect to the molecule of origin
    mol = sim["molecule"][keep]
    big = [g for g in groups if len(g) >= 4]
    assert len(big) >= 8
    assert np.mean([len(set(mol[g - 1])) == 1 for g in big]) > 0.9
    # orient and trim, then MSA + consensus per cluster
    from sarlacc_amd.mock import revcomp
    seqs, quals = sim["reads"].to_strings(), sim["quals"].to_strings()
    orient_s = [revcomp(seqs[i]) if aln["reversed"][i] else seqs[i] for i in keep]
    orient_q = [quals[i][::-1] if aln["reversed"][i] else quals[i] for i in keep]
    msa = generics.multiReadAlign(generics.Reads(orient_s, orient_q), big)
    cons = generics.consensusReadSeq(msa)
    assert len(cons) == len(big)
    for c, g in zip(cons.seq.to_strings(), big):
        truth = sim["reference"][mol[g[0] - 1]]
        assert lev2(c, truth) / 2 <= 0.05 * len(truth)
    basic = generics.consensusReadSeq({"alignments": msa["alignments"]})
    assert len(basic) == len(big)


def test_tied_overlap_known_values():
    # tests/testthat/test-tuning.R:53-59
    from sarlacc_amd.generics import _tied_overlap
    r = np.arange(1, 11, dtype=float)
    assert _tied_overlap(r, r - 10) == 1
    assert _tied_overlap(r, r) == 0.5
    assert abs(_tied_overlap(r, r - 0.5) - 0.55) < 1e-12
    assert abs(_tied_overlap(r, r + 0.5) - 0.45) < 1e-12
    assert _tied_overlap(r, r + 10) == 0


def test_compute_threshold():
    # .compute_threshold (R/getAdaptorThresholds.R:94-103): smallest real score whose estimated FDR <= error
    from sarlacc_amd.generics import _compute_threshold
    real = np.array([1.0, 2, 3, 10, 11, 12, 13, 14, 15, 16])
    scr = np.array([0.5, 1.5, 2.5, 2.7, 2.9])
    assert _compute_threshold(real, scr, 0.01) == 3.0
    assert _compute_threshold(real, scr, 0.4) == 2.0
    assert _compute_threshold(real, scr, 0.5) == 1.0


def test_oracle_scramble_is_a_permutation(oracle):
    from sarlacc_amd.mock import random_reads
    seqs, quals = random_reads(30, 0, 80, seed=2)
    a, b = oracle.scramble(seqs, quals, 7)
    for s, q, x, y in zip(seqs, quals, a, b):
        assert sorted(zip(s, q)) == sorted(zip(x, y))
    assert oracle.scramble(seqs, quals, 7) == (a, b) and oracle.scramble(seqs, quals, 8) != (a, b)


def _fake_aligned(n, rng):
    width = rng.integers(200, 400, n).astype(np.int32)
    def side(lo):
        start = rng.integers(1, 20, n).astype(np.int32) + lo
        return {"score": rng.normal(8, 4, n), "start": start, "end": start + rng.integers(15, 30, n).astype(np.int32),
                "subseq": {"Sub1": ["ACGT"[i % 4] * 3 for i in range(n)]}, "metadata": {"sequence": "X"}}
    a1 = side(0)
    a2 = side(0)
    a2["start"], a2["end"] = width - a2["start"] + 1, width - a2["end"] + 1    # reported in read coordinates
    return {"read.width": width, "adaptor1": a1, "adaptor2": a2, "reversed": rng.random(n) < 0.5,
            "names": ["r%d" % i for i in range(n)], "metadata": {"filepath": None}}


def test_filter_reads_matches_the_r_logic():
    """filterReads (R/filterReads.R:2-43) on a synthetic alignment table, against a line-by-line
    restatement with plain loops; covers essential / non-essential adaptors."""
    from sarlacc_amd.generics import filterReads
    rng = np.random.default_rng(3)
    aln = _fake_aligned(200, rng)
    for ess1, ess2 in ((True, True), (True, False), (False, True), (False, False)):
        got = filterReads(aln, 6, 9, ess1, ess2)
        names, ts, te = [], [], []
        for i in range(200):
            s1, s2 = aln["adaptor1"]["score"][i], aln["adaptor2"]["score"][i]
            if (ess1 and not s1 >= 6) or (ess2 and not s2 >= 9):
                continue
            start = aln["adaptor1"]["end"][i] + 1 if s1 >= 6 else 1
            end = aln["adaptor2"]["end"][i] - 1 if s2 >= 9 else aln["read.width"][i]
            if start < end:
                names.append(aln["names"][i]); ts.append(start); te.append(end)
        assert got["names"] == names
        assert got["trim.start"].tolist() == ts and got["trim.end"].tolist() == te
        assert len(got["adaptor1"]["subseq"]["Sub1"]) == len(names) == len(got["reversed"])
    assert len(filterReads(aln, 1e9, 1e9)["names"]) == 0


def test_barcode_thresholds_and_flat_helpers():
    from sarlacc_amd import calls
    from sarlacc_amd.generics import getBarcodeThresholds
    from sarlacc_amd.strset import StringSet
    x = np.array([1.0, 2.0, 3.0, 4.0, 100.0])
    thr = getBarcodeThresholds({"score": x, "gap": x / 2}, nmads=3)
    # R: median 3, mad = 1.4826 * median(|x - 3|) = 1.4826
    assert abs(thr["score"] - (3 - 3 * 1.4826)) < 1e-12 and abs(thr["gap"] - (1.5 - 3 * 1.4826 * 0.5)) < 1e-12
    off = np.array([0, 2, 2, 5, 6], np.int64)
    vals = np.array([7, 8, 1, 2, 3, 9], np.int32)
    noff, nvals = calls.csr_select(off, vals, np.diff(off) >= 2)
    assert noff.tolist() == [0, 2, 5] and nvals.tolist() == [7, 8, 1, 2, 3]
    ss = StringSet.from_strings(["AC", "", "GGT", "T", "CCCC"])
    assert ss.slice(1, 4).to_strings() == ["", "GGT", "T"] and ss.slice(0, 5).to_strings() == ss.to_strings()
    assert ss.slice(2, 2).to_strings() == []


def test_assign_groups_snake_is_balanced_and_deterministic():
    from sarlacc_amd.shard import assign_groups_snake
    rng = np.random.default_rng(4)
    cost = rng.integers(15000, 25000, 10001).astype(float)
    for world in (1, 2, 3, 8):
        owner = assign_groups_snake(cost, world)
        assert np.array_equal(owner, assign_groups_snake(cost.copy(), world))
        assert owner.min() == 0 and owner.max() == world - 1
        load = np.bincount(owner, weights=cost, minlength=world)
        assert load.max() - load.min() <= cost.max()          # within one group of each other
        counts = np.bincount(owner, minlength=world)
        assert counts.max() - counts.min() <= 1
    assert assign_groups_snake(np.zeros(0), 4).size == 0


def test_strlist_behaves_like_a_list_of_strings():
    from sarlacc_amd.strset import StrList
    words = ["ACGT", "", "GG", "TTTTT", "A"]
    sl = StrList(words)
    assert len(sl) == 5 and list(sl) == words and sl == words and words == sl and sl == StrList(words)
    assert sl != words[:-1] and not (sl == ["ACGT", "", "GG", "TTTTT", "C"])
    assert sl[3] == "TTTTT" and sl[-1] == "A" and sl[1:4] == words[1:4]
    mask = np.array([True, False, True, False, True])
    assert sl.select(mask) == ["ACGT", "GG", "A"] and sl[mask] == ["ACGT", "GG", "A"]
    assert sl[np.array([4, 0])] == ["A", "ACGT"]
    other = StrList(["x1", "x2", "x3", "x4", "x5"])
    assert StrList.where(mask, other, sl) == ["x1", "", "x3", "TTTTT", "x5"]
    assert StrList([]) == [] and len(StrList([]).select(np.zeros(0, bool))) == 0
    with pytest.raises(IndexError):
        sl[5]


def test_quality_class_encodings():
    """.qual2class + .create_encoding_vector for the three classes of adaptorAlign's qual.type
    (R/adaptorAlign.R:8,:97-99; R/qualityMask.R:19-28): offsets, ranges and the score -> error maps."""
    from sarlacc_amd.encoding import encoding_for_qual_type
    name, ph = encoding_for_qual_type(("phred", "solexa", "illumina"))   # the default: first choice
    assert name == "phred" and ph.names[0] == 33 and ph.errors[0] == 1.0 and abs(ph.errors[20] - 0.01) < 1e-15
    name, il = encoding_for_qual_type("illumina")
    assert name == "illumina" and il.names[0] == 64 and il.names[-1] == 126 and abs(il.errors[30] - 1e-3) < 1e-18
    name, so = encoding_for_qual_type("s")                                # unique prefix, as match.arg
    assert name == "solexa" and so.names[0] == 59 and so.names[5] == 64
    assert abs(so.errors[5] - 0.5) < 1e-15                                # Solexa score 0: p/(1-p) = 1
    q = 10.0
    assert abs(so.errors[15] - (10 ** (-q / 10)) / (1 + 10 ** (-q / 10))) < 1e-15
    assert (np.diff(so.errors) < 0).all() and (np.diff(il.errors) < 0).all()
    for bad in ("", "sanger", "x", None, 3):
        with pytest.raises(ValueError, match="should be one of"):
            encoding_for_qual_type(bad)


def test_bench_refuses_fewer_than_one_timed_step():
    """bench.py --steps sets the number of timed steps: none at all is an argument error, before any device is asked for."""
    import subprocess
    import sys
    for bad in (["--steps", "0"], ["--warmup", "-1"]):
        res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + bad, capture_output=True, text=True, timeout=120)
        assert res.returncode != 0 and "--steps must be at least 1" in res.stderr
        assert not [x for x in res.stdout.splitlines() if x.startswith("{")]


def test_bench_giant_rehearsal_needs_full():
    """bench.py --giant-virtual-ranks rehearses a leg that only --full runs measure: without --full it is an argument error,
    before any device is asked for, rather than a run that silently leaves the leg out."""
    import subprocess
    import sys
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--giant-virtual-ranks", "8"], capture_output=True, text=True,
                         timeout=120)
    assert res.returncode != 0 and "add --full" in res.stderr
    assert not [x for x in res.stdout.splitlines() if x.startswith("{")]


def test_bench_output_dump_sampling_and_budget(tmp_path, monkeypatch):
    """bench.py --dump-outputs: float32 / float64 files only, whole outputs while they fit, beyond that the same seeded
    sample on every call, within the byte budget."""
    import bench
    from sarlacc_amd.strset import StringSet
    rng = np.random.default_rng(5)
    n = 3000
    outs = {"scores": rng.random(n), "starts": rng.integers(1, 500, n, dtype=np.int32), "ends": rng.integers(1, 500, n, dtype=np.int32),
            "section_starts": rng.integers(1, 500, n, dtype=np.int32), "section_widths": rng.integers(0, 20, n, dtype=np.int32)}

    def load(d):
        return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}

    whole = tmp_path / "whole"
    whole.mkdir()
    bench.dump_align(str(whole), outs)
    got = load(whole)
    assert sorted(got) == sorted("align_" + k for k in outs)
    for k, v in outs.items():
        assert got["align_" + k].dtype == np.float64 and np.array_equal(got["align_" + k], v)

    monkeypatch.setattr(bench, "DUMP_ALIGN_BYTES", 8000)
    sampled = []
    for rep in range(2):
        d = tmp_path / ("sampled%d" % rep)
        d.mkdir()
        written = bench.dump_align(str(d), outs)
        assert written <= 8000 + 6 * bench.DUMP_HEADER_BYTES
        sampled.append(load(d))
    idx = sampled[0]["align_read_index"].astype(np.int64)
    assert idx.size == 8000 // 48 and (np.diff(idx) > 0).all()
    for k, v in outs.items():
        assert np.array_equal(sampled[0]["align_" + k], v[idx]) and np.array_equal(sampled[1]["align_" + k], sampled[0]["align_" + k])

    # consensus reads of a pipeline pass: groups of 2..6 reads, consensus of 50..150 characters
    ng = 2500
    sizes = rng.integers(2, 7, ng)
    goff = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    gflat = rng.permutation(int(goff[-1])).astype(np.int32) + 1
    widths = rng.integers(50, 151, ng)
    coff = np.concatenate([[0], np.cumsum(widths)]).astype(np.int64)
    cons = StringSet(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(coff[-1]))], coff)
    phred = StringSet(rng.integers(33, 75, int(coff[-1])).astype(np.uint8), coff.copy())
    r = {"cons": cons, "phred": phred, "goff": goff, "gflat": gflat}
    for budget in (10**8, 300_000):
        dumps = []
        for rep in range(2):
            d = tmp_path / ("cons%d_%d" % (budget, rep))
            d.mkdir()
            written = bench.dump_consensus(str(d), r, budget)
            assert written <= budget + 6 * bench.DUMP_HEADER_BYTES
            dumps.append(load(d))
        got = dumps[0]
        for k in got:
            assert got[k].dtype in (np.float32, np.float64) and np.array_equal(got[k], dumps[1][k]), k
        pick = got["pipeline_consensus_index"].astype(np.int64)
        assert 0 < pick.size <= bench.DUMP_CONSENSUS and (np.diff(pick) > 0).all()
        assert pick.size == bench.DUMP_CONSENSUS or budget < 10**8
        co, go = got["pipeline_consensus_offsets"].astype(np.int64), got["pipeline_group_offsets"].astype(np.int64)
        for i, j in enumerate(pick):
            assert got["pipeline_consensus_bases"][co[i]:co[i + 1]].astype(np.uint8).tobytes() == cons[j].encode()
            assert got["pipeline_consensus_quals"][co[i]:co[i + 1]].astype(np.uint8).tobytes() == phred[j].encode()
            assert np.array_equal(got["pipeline_group_members"][go[i]:go[i + 1]], gflat[goff[j]:goff[j + 1]])
