"""readGroups without a device: the plain-Python restatement of its rules (tests/read_groups_cases.py) is pinned on
hand-written cases whose expected arrays are typed out, the argument checks raise before the library is touched, and
no reads or no rows return the empty result without one."""
import numpy as np
import pytest

from sarlacc_amd import generics, groups
from sarlacc_amd.strset import StrList, lists_from_csr
from tests import read_groups_cases as G


@pytest.fixture
def no_library(monkeypatch):
    """Any touch of the native library fails the test."""
    from sarlacc_amd import _lib

    def refuse():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", refuse)


@pytest.mark.parametrize("case", G.LITERAL, ids=[c[0] for c in G.LITERAL])
def test_restatement_on_literal_cases(case):
    what, rows, names, kwargs, want = case
    G.same(G.expected(G.make_ranges(rows), names, **kwargs), G.literal_expected(want), what)


def test_restatement_nested_range_needs_the_running_maximum():
    """The wrong rule -- compare with the previous end -- splits the group of the nested case; the restatement does not."""
    what, rows, names, kwargs, want = G.LITERAL[1]
    order = sorted(range(4), key=lambda r: rows[r][2])
    wrong, label, prev_end = [], -1, None
    for r in order:
        if prev_end is None or rows[r][2] > prev_end:
            label += 1
        prev_end = rows[r][2] + rows[r][3] - 1
        wrong.append(label)
    assert wrong == [0, 0, 1, 2] and want["group"] == [0, 0, 0, 1]


def test_key_and_duplicates():
    assert [G.key_of(s) for s in ("a b", "a\tb c", "ab", " x", "a ", "")] == ["a", "a", "ab", "", "a", ""]
    ranges = G.make_ranges([("a", 0, 1, 1, "+")])
    with pytest.raises(G.DuplicateKey, match="read names 2 and 4 are the same up to their first space or tab"):
        G.expected(ranges, ["x", "a 1", "b", "a\t2", "a", "x"])
    with pytest.raises(G.DuplicateKey, match="read names 1 and 3 are"):
        G.expected(ranges, ["q", "r", "q", "r"])


def test_split_labels():
    off, members = G.split_labels([3, -1, 0, 3, 7, 0])
    assert off.tolist() == [0, 2, 4, 5] and members.tolist() == [3, 6, 1, 4, 5]
    assert [m.tolist() for m in lists_from_csr(off, members)] == [[3, 6], [1, 4], [5]]
    off, members = G.split_labels([-1, -1])
    assert off.tolist() == [0] and members.size == 0


def test_generated_cases_hold_what_they_promise():
    rows, names = G.name_case(5000)
    keys = [G.key_of(s) for s in names]
    assert len(set(keys)) == 5000 and set(G.KEY_LENGTHS) <= set(len(k) for k in keys)
    assert len(names[-1]) == max(len(s) for s in names) and len(rows[-1][0]) == max(len(r[0]) for r in rows)
    assert any("\t" in s for s in names) and any(s.endswith(" ") for s in names)
    want = G.expected(G.make_ranges(rows, 7), names)
    assert want["n.records"].max() == 6 and (want["n.records"] == 0).any() and want["unmatched.records"] > 1000
    for n in (1, 2, 63):
        rows, names = G.name_case(n)
        assert len(names) == n
    rows, names = G.locus_case()
    want = G.expected(G.make_ranges(rows, 7), names, by="locus", maxgap=0, ignore_strand=True)
    on3 = [i for i in range(len(names)) if want["reference"][i] == 3]
    assert len(set(want["group"][on3].tolist())) > 20      # the reach of reference 2 does not merge reference 3


# ---- rule 5 ----------------------------------------------------------------------------------------------------------------
RANGES = G.make_ranges([("a", 0, 1, 5, "+"), ("b", 1, 3, 5, "-")])


def _with(**cols):
    return dict(RANGES, **cols)


@pytest.mark.parametrize("ranges, names, kwargs, message", [
    (RANGES, ["a"], dict(by="transcript"), "'by' should be one of"),
    (RANGES, ["a"], dict(by=None), "'by' should be one of"),
    (RANGES, ["a"], dict(by="locus", maxgap=-1), "'maxgap' should be an integer"),
    (RANGES, ["a"], dict(by="locus", maxgap=2 ** 31), "'maxgap' should be an integer"),
    (RANGES, ["a"], dict(by="locus", maxgap=1.5), "'maxgap' should be an integer"),
    (RANGES, ["a"], dict(maxgap=True), "'maxgap' should be an integer"),
    (_with(width=np.array([5], np.int32)), ["a"], {}, "columns of 'ranges' differ in length"),
    (_with(names=StrList(["a", "b", "c"])), ["a"], {}, "columns of 'ranges' differ in length"),
    (_with(strand=np.array(["+"], "<U1")), ["a"], {}, "columns of 'ranges' differ in length"),
    (_with(seqnames=np.array([0, 2], np.int32)), ["a"], {}, "row 2 of 'ranges': seqname code 2 outside the seqinfo"),
    (_with(seqnames=np.array([-1, 0], np.int32)), ["a"], {}, "row 1 of 'ranges': seqname code -1 outside the seqinfo"),
    ({k: v for k, v in RANGES.items() if k != "strand"}, ["a"], {}, "'ranges' lacks strand"),
])
def test_argument_checks_raise_before_the_library(no_library, ranges, names, kwargs, message):
    with pytest.raises(ValueError, match=message):
        generics.readGroups(ranges, names, **kwargs)


def test_reads_without_names_are_refused(no_library):
    reads = generics.Reads(["ACGT"], ["IIII"])
    with pytest.raises(ValueError, match="reads have no names"):
        generics.readGroups(RANGES, reads)


def test_read_names_of_every_kind():
    reads = generics.Reads(["ACGT", "AC"], ["IIII", "II"], names=["a x", "b"])
    for r in (reads, ["a x", "b"], StrList(["a x", "b"])):
        assert groups.read_names(r).to_strings() == ["a x", "b"]
    ss = StrList(["a x", "b"]).ss
    assert groups.read_names(StrList(ss)) is ss          # handed over undecoded


@pytest.mark.parametrize("by", ["reference", "locus"])
def test_empty_inputs_need_no_device(no_library, by):
    empty = G.make_ranges([], 3)
    got = generics.readGroups(empty, ["a", "b c"], by=by)
    G.same(got, G.expected(empty, ["a", "b c"], by=by), "no rows")
    assert got["record"].tolist() == [-1, -1] and got["n.records"].tolist() == [0, 0] and got["groups"][0].tolist() == [0]
    got = generics.readGroups(RANGES, [], by=by)
    G.same(got, G.expected(RANGES, [], by=by), "no reads")
    assert got["record"].size == 0 and got["groups"][1].size == 0
    assert lists_from_csr(*got["groups"]) == []
