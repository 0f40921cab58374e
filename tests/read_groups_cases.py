"""Plain-Python restatement of generics.readGroups (sarlacc_amd/groups.py, csrc/read_groups.hip) and the cases its tests
share: a dict join, `max` with the tie rule, and a sort plus a running maximum.  Everything is integers; nothing here
touches the library.  tests/test_read_groups_host.py pins the restatement on the literal cases below, whose expected
arrays are typed out; tests/test_gpu_read_groups.py holds the device to it."""
import numpy as np

from sarlacc_amd.strset import StrList

INT_MAX = 2 ** 31 - 1


class DuplicateKey(Exception):
    def __init__(self, j, k):
        super().__init__("read names %d and %d are the same up to their first space or tab" % (j, k))
        self.j, self.k = j, k


def key_of(name):
    """The name up to, and not including, its first space or tab."""
    cut = [p for p in (name.find(" "), name.find("\t")) if p >= 0]
    return name[:min(cut)] if cut else name


def make_ranges(rows, nref=None):
    """rows: (qname, seqname code, start, width, strand) -> the dict sam2ranges returns (the used columns)."""
    ref = np.array([r[1] for r in rows], np.int32)
    start = np.array([r[2] for r in rows], np.int64)
    width = np.array([r[3] for r in rows], np.int64)
    nref = (int(ref.max()) + 1 if ref.size else 1) if nref is None else nref
    return {"seqnames": ref, "start": start.astype(np.int32), "width": width.astype(np.int32),
            "end": (start + width - 1).astype(np.int32),      # (wraps where the end leaves int32: nobody reads it)
            "strand": np.array([r[4] for r in rows], "<U1"), "names": StrList([r[0] for r in rows]),
            "seqinfo": {"seqnames": ["ref%d" % k for k in range(nref)], "seqlengths": np.zeros(nref, np.int64)}}


def split_labels(labels):
    """split(seq_along(x), labels) without empty levels and the negative labels, as the CSR pair."""
    labels = np.asarray(labels)
    levels = sorted(set(int(v) for v in labels if v >= 0))
    lists = [[i + 1 for i, v in enumerate(labels) if v == lev] for lev in levels]
    off = np.zeros(len(lists) + 1, np.int64)
    if lists:
        np.cumsum([len(x) for x in lists], out=off[1:])
    return off, np.array([i for x in lists for i in x], np.int32)


def expected(ranges, names, by="reference", maxgap=0, ignore_strand=True):
    """What readGroups returns, by the rules of DESIGN §4 as they are written."""
    names = list(names)
    n = len(names)
    first = {}
    for i, name in enumerate(names):                       # rule 1
        k = key_of(name)
        if k in first:
            raise DuplicateKey(first[k] + 1, i + 1)
        first[k] = i
    ref, start, width, strand = (ranges[c] for c in ("seqnames", "start", "width", "strand"))
    rows_of, unmatched = {}, 0
    for r, q in enumerate(ranges["names"]):
        if q in first:
            rows_of.setdefault(first[q], []).append(r)
        else:
            unmatched += 1
    record = np.full(n, -1, np.int32)
    count = np.zeros(n, np.int32)
    for i, rows in rows_of.items():                        # rule 2: greatest width, the lowest row among equals
        record[i] = max(rows, key=lambda r: (int(width[r]), -r))
        count[i] = len(rows)
    reference = np.array([int(ref[r]) if r >= 0 else -1 for r in record], np.int32)
    if by == "reference":
        group = reference.copy()
    else:                                                  # rule 4
        group = np.full(n, -1, np.int32)
        items = sorted((int(ref[r]), 0 if ignore_strand or strand[r] != "-" else 1, int(start[r]), i)
                       for i, r in enumerate(record) if r >= 0)
        label, previous, running = -1, None, None
        for rf, sb, st, i in items:
            end = st + int(width[record[i]]) - 1
            if previous != (rf, sb) or st > running + maxgap:
                label += 1
                running = end
            running = max(running, end)
            previous = (rf, sb)
            group[i] = label
    return {"record": record, "n.records": count, "reference": reference, "group": group, "groups": split_labels(group),
            "unmatched.records": np.int64(unmatched)}


def same(got, want, what=""):
    """Every entry of two readGroups results, exactly, dtype included."""
    for k in ("record", "n.records", "reference", "group"):
        assert got[k].dtype == np.int32 and np.array_equal(got[k], want[k]), (what, k, got[k][:20], want[k][:20])
    assert got["groups"][0].dtype == np.int64 and got["groups"][1].dtype == np.int32, what
    assert np.array_equal(got["groups"][0], want["groups"][0]) and np.array_equal(got["groups"][1], want["groups"][1]), (what, "groups")
    assert int(got["unmatched.records"]) == int(want["unmatched.records"]), (what, "unmatched.records")


# ---- literal cases: (what, rows, read names, arguments, expected columns typed out) ----------------------------------------
# Every read of a locus case has one row unless said otherwise; "group" is the label per read.
TOP = INT_MAX
LITERAL = [
    ("tie rule: the first of the widest rows",
     [("a", 0, 10, 5, "+"), ("a", 1, 20, 9, "+"), ("a", 2, 30, 9, "-"), ("a", 0, 40, 3, "+"), ("b", 2, 5, 0, "+"), ("zz", 0, 1, 1, "+")],
     ["b comment", "a", "c"], dict(by="reference"),
     dict(record=[4, 1, -1], count=[1, 4, 0], reference=[2, 1, -1], group=[2, 1, -1], off=[0, 1, 2], members=[2, 1], unmatched=1)),
    ("a nested long range, then a range that overlaps only the long one",
     [("r1", 0, 1, 100, "+"), ("r2", 0, 10, 11, "+"), ("r3", 0, 50, 11, "+"), ("r4", 0, 101, 5, "+")],
     ["r1", "r2", "r3", "r4"], dict(by="locus", maxgap=0),
     dict(record=[0, 1, 2, 3], count=[1, 1, 1, 1], reference=[0, 0, 0, 0], group=[0, 0, 0, 1], off=[0, 3, 4], members=[1, 2, 3, 4], unmatched=0)),
    ("adjacent ranges, maxgap 0",
     [("r1", 0, 1, 10, "+"), ("r2", 0, 11, 10, "+")], ["r1", "r2"], dict(by="locus", maxgap=0),
     dict(record=[0, 1], count=[1, 1], reference=[0, 0], group=[0, 1], off=[0, 1, 2], members=[1, 2], unmatched=0)),
    ("adjacent ranges, maxgap 1",
     [("r1", 0, 1, 10, "+"), ("r2", 0, 11, 10, "+")], ["r1", "r2"], dict(by="locus", maxgap=1),
     dict(record=[0, 1], count=[1, 1], reference=[0, 0], group=[0, 0], off=[0, 2], members=[1, 2], unmatched=0)),
    ("identical coordinates on two references",
     [("r1", 1, 7, 30, "+"), ("r2", 0, 7, 30, "+"), ("r3", 1, 7, 30, "+")], ["r1", "r2", "r3"], dict(by="locus", maxgap=50),
     dict(record=[0, 1, 2], count=[1, 1, 1], reference=[1, 0, 1], group=[1, 0, 1], off=[0, 1, 3], members=[2, 1, 3], unmatched=0)),
    ("strands ignored",
     [("r1", 0, 1, 10, "+"), ("r2", 0, 5, 11, "-"), ("r3", 0, 8, 5, "+")], ["r1", "r2", "r3"], dict(by="locus", ignore_strand=True),
     dict(record=[0, 1, 2], count=[1, 1, 1], reference=[0, 0, 0], group=[0, 0, 0], off=[0, 3], members=[1, 2, 3], unmatched=0)),
    ("strands kept: '+' before '-'",
     [("r1", 0, 1, 10, "-"), ("r2", 0, 5, 11, "+"), ("r3", 0, 8, 5, "-")], ["r1", "r2", "r3"], dict(by="locus", ignore_strand=False),
     dict(record=[0, 1, 2], count=[1, 1, 1], reference=[0, 0, 0], group=[1, 0, 1], off=[0, 1, 3], members=[2, 1, 3], unmatched=0)),
    ("zero-width ranges, maxgap 0: an empty range ends in front of its start",
     [("r1", 0, 5, 0, "+"), ("r2", 0, 5, 0, "+"), ("r3", 0, 4, 1, "+")], ["r1", "r2", "r3"], dict(by="locus", maxgap=0),
     dict(record=[0, 1, 2], count=[1, 1, 1], reference=[0, 0, 0], group=[1, 2, 0], off=[0, 1, 2, 3], members=[3, 1, 2], unmatched=0)),
    ("zero-width ranges, maxgap 1",
     [("r1", 0, 5, 0, "+"), ("r2", 0, 5, 0, "+"), ("r3", 0, 4, 1, "+")], ["r1", "r2", "r3"], dict(by="locus", maxgap=1),
     dict(record=[0, 1, 2], count=[1, 1, 1], reference=[0, 0, 0], group=[0, 0, 0], off=[0, 3], members=[1, 2, 3], unmatched=0)),
    ("an end at 2^31 - 1 and one beyond it, maxgap 0: ends in 64 bits",
     [("r1", 0, TOP, 1, "+"), ("r2", 0, 1, 1, "+"), ("r3", 0, 3, TOP, "+")], ["r1", "r2", "r3"], dict(by="locus", maxgap=0),
     dict(record=[0, 1, 2], count=[1, 1, 1], reference=[0, 0, 0], group=[1, 0, 1], off=[0, 1, 3], members=[2, 1, 3], unmatched=0)),
    ("an end at 2^31 - 1, maxgap 2^31 - 1: the sum in 64 bits",
     [("r1", 0, TOP, 1, "+"), ("r2", 0, 1, 1, "+"), ("r3", 1, 1, TOP, "+")], ["r1", "r2", "r3"], dict(by="locus", maxgap=TOP),
     dict(record=[0, 1, 2], count=[1, 1, 1], reference=[0, 0, 1], group=[0, 0, 1], off=[0, 2, 3], members=[1, 2, 3], unmatched=0)),
]


def literal_expected(e):
    return {"record": np.array(e["record"], np.int32), "n.records": np.array(e["count"], np.int32),
            "reference": np.array(e["reference"], np.int32), "group": np.array(e["group"], np.int32),
            "groups": (np.array(e["off"], np.int64), np.array(e["members"], np.int32)), "unmatched.records": np.int64(e["unmatched"])}


# ---- generated cases ---------------------------------------------------------------------------------------------------------
KEY_LENGTHS = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 254, 300)
_ALPHABET = "".join(chr(c) for c in range(33, 127))


def _random_key(rng, length):
    return "".join(_ALPHABET[k] for k in rng.integers(0, len(_ALPHABET), length))


def name_case(n, seed=0):
    """(rows, read names) of n reads whose keys have the lengths above (the wavefront takes 64 bytes a step), among them
    keys that differ only in their last byte, only behind byte 64, and proper prefixes of other keys; comments behind a
    space, behind a tab, and an empty one; per read 0 to 6 rows with small widths, so that ties are common; rows that
    name no read, among them a read's whole name with its comment and a key followed by a space; rows in shuffled
    order.  The longest read name stands last in its buffer, and so does the longest record name."""
    rng = np.random.default_rng(seed)
    keys = []
    if n >= 12:
        stem = _random_key(rng, 299)
        keys += [stem[:15] + "a", stem[:15] + "b",          # the last byte of one 16-byte piece
                 stem[:64] + "a", stem[:64] + "b",          # only behind byte 64
                 stem[:128] + "x", stem[:128] + "y", stem[:128],
                 stem[:10], stem[:63], stem[:253] + "q", stem + "1", stem + "2"]
    taken = set(keys)
    while len(keys) < n:
        length = KEY_LENGTHS[len(keys) % len(KEY_LENGTHS)]
        if length == 1 and len(keys) >= 60:
            length = 20 + len(keys) % 9
        k = _random_key(rng, length)
        if k not in taken:
            taken.add(k)
            keys.append(k)
    keys = keys[:n]
    keys.sort(key=lambda k: (len(k) >= 300, rng.random()))      # shuffled, one of the longest last
    comments = ("", " runid=0a1b ch=12", "\tstart_time=2020", " ")
    names = [k + comments[i % 4] for i, k in enumerate(keys)]
    names[-1] = keys[-1] + " the longest name of the buffer stands last"
    rows = []
    for i, k in enumerate(keys):
        for _ in range((0, 1, 1, 2, 1, 3, 6, 1, 4)[i % 9]):
            rows.append((k, int(rng.integers(0, 7)), int(rng.integers(1, 400)), int(rng.integers(0, 4) * 25), "+-"[int(rng.integers(0, 2))]))
    for i in range(0, n, 7):
        rows.append((names[i] if " " in names[i] or "\t" in names[i] else keys[i] + " ", 0, 1, 500, "+"))   # the whole name: no match
        rows.append((keys[i] + " ", 1, 1, 500, "+"))
        rows.append((keys[i][:-1] if len(keys[i]) > 1 and keys[i][:-1] not in taken else "nobody", 2, 1, 500, "-"))
        rows.append(("", 3, 1, 500, "+"))
    order = rng.permutation(len(rows))
    rows = [rows[j] for j in order]
    rows.append((keys[-1] + "_and_then_some_more_bytes_that_no_read_has", 0, 1, 500, "+"))
    return rows, names


def locus_case(n=3000, nref=7, seed=1):
    """n reads with one row each on nref references: starts from a small range, widths from 0 to a few long ones, so
    that chains of overlaps and nested ranges are common; both strands.  Reference 2 holds one range that reaches past
    every start of reference 3: a running maximum that is not reset at the boundary merges all of reference 3."""
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(n):
        ref = int(rng.integers(0, nref))
        width = int(rng.integers(0, 12)) if rng.random() < 0.9 else int(rng.integers(50, 300))
        rows.append(("read%d" % i, ref, int(rng.integers(1, 6000)), width, "+-"[int(rng.integers(0, 2))]))
    rows[0] = ("read0", 2, 5990, 100000, "+")
    names = ["read%d" % i for i in range(n)]
    order = rng.permutation(n)
    return [rows[j] for j in order], names
