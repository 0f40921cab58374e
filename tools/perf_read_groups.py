"""readGroups on the device against the route a user writes today, and its kernels beside a copy of the name bytes.

Workload: --reads reads (default 10^6) with basecaller-like names, a 36-byte UUID and a comment ("<uuid> runid=... ch=...");
5 % of them unmapped (no record), 15 % with 2 to 4 records, the rest with one: about 1.2 records per read, in shuffled
order, on --refs references (default 20 000 transcripts), starts uniform over 2 000 bases, widths 200 to 1 500.

  k lines  the stage timers of the four C calls (HIP events on the stream, best of five): names_keys, names_build,
           names_check, names_probe, records_pick, locus_labels, labels_csr, beside sarlacc_dev_copy of the name bytes of
           both sets (wall, best of five).
  w lines  generics.readGroups end to end (uploads and downloads included) in both modes against the host route: the names
           decoded to Python strings, a dict over the keys, a lookup per record name, numpy lexsort for the pick and for
           the loci, np.unique for the split.  The two routes alternate in one process, five repeats each, after a check
           that they return identical arrays.

    python tools/perf_read_groups.py [--reads 1000000] [--refs 20000] [--out profiles/read_groups.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
STAGES = ("names_keys", "names_build", "names_check", "names_probe", "records_pick", "locus_labels", "labels_csr")


def say(out, line):
    print(line, flush=True)
    with open(out, "a") as fh:
        fh.write(line + "\n")


def workload(n, nref, seed=1000):
    """(ranges as sam2ranges returns them, read names as a StrList)."""
    from sarlacc_amd.strset import StringSet, StrList
    rng = np.random.default_rng(seed)
    hexd = np.frombuffer(b"0123456789abcdef", np.uint8)
    uuid = hexd[rng.integers(0, 16, (n, 36))]
    uuid[:, [8, 13, 18, 23]] = ord("-")
    uuid[:, :8] = hexd[(np.arange(n)[:, None] >> (4 * np.arange(7, -1, -1))) & 15]      # distinct whatever the draw
    comment = np.frombuffer(b" runid=", np.uint8)[None, :].repeat(n, 0)
    tail = np.concatenate([comment, hexd[rng.integers(0, 16, (n, 8))], np.frombuffer(b" ch=", np.uint8)[None, :].repeat(n, 0),
                           hexd[rng.integers(0, 10, (n, 3))]], axis=1)
    names = StrList(StringSet.from_matrix(np.concatenate([uuid, tail], axis=1)))
    u = rng.random(n)
    per_read = np.where(u < 0.05, 0, np.where(u < 0.20, rng.integers(2, 5, n), 1))
    read = np.repeat(np.arange(n), per_read)
    read = read[rng.permutation(read.size)]
    m = read.size
    start = rng.integers(1, 2000, m).astype(np.int32)
    width = rng.integers(200, 1500, m).astype(np.int32)
    ranges = {"seqnames": rng.integers(0, nref, m).astype(np.int32), "start": start, "width": width, "end": start + width - 1,
              "strand": np.array(["+", "-"])[rng.integers(0, 2, m)], "names": StrList(StringSet.from_matrix(uuid[read])),
              "seqinfo": {"seqnames": ["T%d" % k for k in range(nref)] + ["*"], "seqlengths": np.zeros(nref + 1, np.int64)}}
    return ranges, names


def host_route(ranges, names, by, maxgap=0, ignore_strand=True):
    """What a user writes today, with numpy wherever numpy has the operation."""
    import re
    cut = re.compile("[ \t]")
    keys = [cut.split(s, 1)[0] for s in names.tolist()]
    n = len(keys)
    index = {k: i for i, k in enumerate(keys)}
    if len(index) != n:
        raise ValueError("duplicate keys")
    qn = ranges["names"].tolist()
    ror = np.fromiter((index.get(q, -1) for q in qn), np.int64, len(qn))
    ref, start, width, strand = (ranges[c] for c in ("seqnames", "start", "width", "strand"))
    rows = np.flatnonzero(ror >= 0)
    order = rows[np.lexsort((rows, -width[rows].astype(np.int64), ror[rows]))]
    owner = ror[order]
    head = np.r_[True, owner[1:] != owner[:-1]] if order.size else np.zeros(0, bool)
    record = np.full(n, -1, np.int32)
    record[owner[head]] = order[head]
    count = np.bincount(ror[rows], minlength=n).astype(np.int32)
    mapped = np.flatnonzero(record >= 0)
    reference = np.full(n, -1, np.int32)
    reference[mapped] = ref[record[mapped]]
    if by == "reference":
        group = reference
    else:
        rec = record[mapped]
        sbit = np.zeros(rec.size, np.int64) if ignore_strand else (strand[rec] == "-").astype(np.int64)
        o = np.lexsort((mapped, start[rec], sbit, ref[rec]))
        seg = ref[rec][o].astype(np.int64) * 2 + sbit[o]
        st = start[rec][o].astype(np.int64)
        end = st + width[rec][o] - 1
        running = np.maximum.accumulate(seg * (1 << 34) + end + (1 << 33)) - seg * (1 << 34) - (1 << 33)    # a maximum per segment
        new = np.r_[True, (seg[1:] != seg[:-1]) | (st[1:] > running[:-1] + maxgap)] if o.size else np.zeros(0, bool)
        group = np.full(n, -1, np.int32)
        group[mapped[o]] = np.cumsum(new) - 1
    labelled = np.flatnonzero(group >= 0)
    by_label = labelled[np.argsort(group[labelled], kind="stable")]
    _, first = np.unique(group[by_label], return_index=True)
    off = np.r_[first, by_label.size].astype(np.int64)
    return {"record": record, "n.records": count, "reference": reference, "group": group,
            "groups": (off, (by_label + 1).astype(np.int32)), "unmatched.records": np.int64((ror < 0).sum())}


def identical(a, b):
    return (all(np.array_equal(a[k], b[k]) for k in ("record", "n.records", "reference", "group"))
            and np.array_equal(a["groups"][0], b["groups"][0]) and np.array_equal(a["groups"][1], b["groups"][1])
            and int(a["unmatched.records"]) == int(b["unmatched.records"]))


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10 ** 6)
    ap.add_argument("--refs", type=int, default=20000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "read_groups.txt"))
    args = ap.parse_args()
    from sarlacc_amd import _lib, generics
    from sarlacc_amd._lib import check
    from sarlacc_amd.resident import DevBuffer
    out = args.out
    open(out, "w").close()
    say(out, "tools/perf_read_groups.py --reads %d --refs %d --repeats %d" % (args.reads, args.refs, args.repeats))
    ranges, names = workload(args.reads, args.refs)
    n, m = len(names), len(ranges["names"])
    nbytes = names.ss.total + ranges["names"].ss.total
    say(out, "%d reads (%.1f MB of names), %d records (%.1f MB of names), %d references" % (n, names.ss.total / 1e6, m, ranges["names"].ss.total / 1e6, args.refs))
    modes = (("reference", {}), ("locus", {"maxgap": 0, "ignore_strand": False}))
    for by, kw in modes:      # the check, and the warm-up of both routes
        dev, host = generics.readGroups(ranges, names, by=by, **kw), host_route(ranges, names, by, **kw)
        if not identical(dev, host):
            sys.exit("by = %s: the two routes differ" % by)
        say(out, "c by = %s: identical arrays, %d groups, %d reads without a record, %d reads with several" % (by, dev["groups"][0].size - 1, int((dev["record"] < 0).sum()), int((dev["n.records"] > 1).sum())))

    stage = {s: [] for s in STAGES}
    for _ in range(args.repeats):
        for by, kw in modes:
            generics.readGroups(ranges, names, by=by, **kw)
            for s in STAGES:
                if s != "locus_labels" or by == "locus":
                    stage[s].append(_lib.stage_ms(s))
    a, b = DevBuffer(nbytes), DevBuffer(nbytes)
    copy = min(timed(lambda: check(_lib.lib().sarlacc_dev_copy(a, b, nbytes, None)))[0] for _ in range(args.repeats))
    say(out, "k sarlacc_dev_copy of the %.1f MB of names: %.3f ms (wall)" % (nbytes / 1e6, copy))
    for s in STAGES:
        say(out, "k %-13s %8.3f ms (best of %d; %s)" % (s, min(stage[s]), len(stage[s]), " ".join("%.3f" % v for v in stage[s])))
    say(out, "k the four name stages together %.3f ms = %.1f x the copy" % (sum(min(stage[s]) for s in STAGES[:4]), sum(min(stage[s]) for s in STAGES[:4]) / copy))

    for by, kw in modes:
        d, h = [], []
        for _ in range(args.repeats):      # the routes alternate
            d.append(timed(lambda: generics.readGroups(ranges, names, by=by, **kw))[0])
            h.append(timed(lambda: host_route(ranges, names, by, **kw))[0])
        say(out, "w by = %s: readGroups %s ms (best %.1f) | host route %s ms (best %.1f) | host / device %.1f"
            % (by, " ".join("%.1f" % v for v in d), min(d), " ".join("%.1f" % v for v in h), min(h), min(h) / min(d)))


if __name__ == "__main__":
    main()
