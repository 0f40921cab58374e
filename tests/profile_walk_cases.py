"""Gapped alignment strings built around what the profiling walks carry from one 64-character step to the next
(profile_walk.hpp, profile.hip, profile_reads.hip): one feature -- a gap run, a homopolymer, a run split by gaps, a run
with gaps in front of or behind it -- of a length around 1, 64, 128 and 192 behind a pad that puts it at every phase of
a step, with the reads that make the matcher and the error walk look across it; a heavy-tailed random generator; and a
count, read off the strings alone, of the step situations a list of strings holds.  Seeded, no GPU, no kernel code:
test infrastructure shared by the oracle tests and the GPU parity tests."""
import functools
import itertools

import numpy as np

STEP = 64
PADS = (0, 1, 2, 62, 63, 64, 65, 127, 128)
FEATURES = (1, 2, 3, 62, 63, 64, 65, 66, 127, 128, 129, 192, 193)
TAILS = (0, 1, 2, 63, 64)
DEGENERATE = (1, 63, 64, 65, 128, 129)
EDGE_LENGTHS = (63, 64, 65, 127, 128, 129)
RANDOM_TOTALS = (0, 1, 63, 64, 65, 128, 200, 300, 400)
BASE = "G"          # the feature's base
_CYCLE = "ACGT"


def _pad(n):
    """n bases, no two equal neighbours, the last one a T"""
    return "".join(_CYCLE[(k - n) % 4] for k in range(n))


def _tail(n):
    """n bases, no two equal neighbours, the first one an A"""
    return "".join(_CYCLE[k % 4] for k in range(n))


def _fill(ref, f):
    """the reference with every gap run replaced by f(base before it or "", base after it or "", its length)"""
    out, i, last = [], 0, ""
    while i < len(ref):
        if ref[i] != "-":
            out.append(ref[i]); last = ref[i]; i += 1
            continue
        j = i
        while j < len(ref) and ref[j] == "-":
            j += 1
        out.append(f(last, ref[j] if j < len(ref) else "", j - i))
        i = j
    return "".join(out)


def _other(a, b, k):
    return next(c for c in _CYCLE if c != a and c != b) * k


def _reads_for(kind, pad, F, tail, ref):
    """(variant, read) for one reference string: equal length, never a gap opposite a gap"""
    out = [("i", _fill(ref, lambda a_, b_, k: BASE * k)),          # same-base insertion: a read run across the gaps
           ("ii", _fill(ref, _other))]                             # an insertion that touches neither neighbour
    if kind == "b":
        out.append(("iii", pad + "-" * F + tail))                  # the homopolymer deleted
    if kind == "d":   # ref: pad, F gaps, GG, tail
        out.append(("iv", pad + BASE * F + "--" + tail))           # the read's run lies in the extension only: 0
        out.append(("v", pad + BASE * F + BASE + "-" + tail))      # one base of the run proper kept: F + 1
    if kind == "f":   # ref: pad, GG, F gaps, tail
        out.append(("iv", pad + "--" + BASE * F + tail))
        out.append(("v", pad + "-" + BASE + BASE * F + tail))
    if "-" in ref:
        out.append(("vi", _fill(ref, lambda a_, b_, k: "N" * k)))  # N opposite reference gaps only: no error
    return out


def _feature(kind, F, a, b):
    if kind == "a":
        return "-" * F
    if kind == "b":
        return BASE * F
    if kind == "c":
        return BASE * a + "-" * F + BASE * b
    if kind == "d":
        return "-" * F + BASE * 2
    if kind == "f":
        return BASE * 2 + "-" * F
    raise ValueError(kind)


# cases found failing on the device, kept by name: (name, reference string, read string)
REGRESSIONS = []


@functools.lru_cache(maxsize=None)
def family():
    """((name, reference string, read string), ...): every kind x pad x feature length x tail, the degenerate strings and
    the named regression cases.  Names read kind:pad:F:tail[:a.b]:variant.  Kinds (F the feature length): a = F gaps,
    b = F times G, c = one run of G split by F gaps (a bases in front, b behind), d = F gaps in front of GG, f = F gaps
    behind GG, e = degenerate strings.  Variants: see _reads_for."""
    out, seen = [], set()

    def add(name, ref, read):
        assert len(ref) == len(read) and not any(x == "-" and y == "-" for x, y in zip(ref, read)), name
        if (ref, read) not in seen:
            seen.add((ref, read))
            out.append((name, ref, read))

    for kind in "abcdf":
        for (ip, p), F, (it, t) in itertools.product(enumerate(PADS), FEATURES, enumerate(TAILS)):
            a, b = ((1, 1), (1, 2), (2, 1), (2, 2))[(ip + it) % 4] if kind == "c" else (0, 0)
            pad, tail = _pad(p), _tail(t)
            ref = pad + _feature(kind, F, a, b) + tail
            tag = "%s:%d:%d:%d" % (kind, p, F, t) + (":%d.%d" % (a, b) if kind == "c" else "")
            for variant, read in _reads_for(kind, pad, F, tail, ref):
                add(tag + ":" + variant, ref, read)
    add("e:empty", "", "")
    for k in DEGENERATE:
        for fill in ("G", "A", "N"):
            add("e:gaps:%d:%s" % (k, fill), "-" * k, fill * k)
        add("e:run:%d:same" % k, BASE * k, BASE * k)
        add("e:run:%d:deleted" % k, BASE * k, "-" * k)
        add("e:run:%d:other" % k, BASE * k, "A" * k)
        for fill in ("G", "A", "N"):
            add("e:base+gaps:%d:%s" % (k, fill), BASE + "-" * k, BASE + fill * k)
            add("e:base+gaps:%d:%s:deleted" % (k, fill), BASE + "-" * k, "-" + fill * k)
    for name, ref, read in REGRESSIONS:
        add("regression:" + name, ref, read)
    return tuple(out)


def _segment_length(rng):
    u = rng.random()
    if u < 0.5:
        return int(rng.integers(1, 5))
    if u < 0.75:
        return int(rng.choice((62, 63, 64, 65, 66, 126, 127, 128, 129, 130, 191, 192, 193)))
    return int(rng.integers(1, 141))


def random_reference(rng, total, p_gap=0.4):
    """a gapped string of `total` characters in segments of heavy-tailed length: gap runs and homopolymers"""
    out = []
    while sum(map(len, out)) < total:
        k = _segment_length(rng)
        out.append("-" * k if rng.random() < p_gap else _CYCLE[int(rng.integers(0, 4))] * k)
    return "".join(out)[:total]


def random_read(rng, ref):
    """a read string for `ref`: opposite a gap run either one base throughout (half of the time that of a neighbour) or
    random bases; opposite a base mostly that base, else another one or a deletion -- at times over a whole stretch"""
    def ins(a, b, k):
        u = rng.random()
        if u < 0.25 and a:
            return a * k
        if u < 0.5 and b:
            return b * k
        if u < 0.6:
            return _CYCLE[int(rng.integers(0, 4))] * k
        return "".join(rng.choice(list(_CYCLE), k))
    read = list(_fill(ref, ins))
    i = 0
    while i < len(ref):
        if ref[i] != "-":
            u = rng.random()
            if u < 0.04:   # a deletion of a heavy-tailed length, over bases only
                for j in range(i, min(len(ref), i + _segment_length(rng))):
                    if ref[j] != "-":
                        read[j] = "-"
            elif u < 0.12:
                read[i] = _CYCLE[int(rng.integers(0, 4))]
        i += 1
    return "".join(read)


@functools.lru_cache(maxsize=None)
def random_pairs(seed=20250117, per_total=11, reads_per_ref=3):
    """((reference string, read string), ...): about 300 pairs, `reads_per_ref` reads against each reference string"""
    rng = np.random.default_rng(seed)
    out = []
    for total in RANDOM_TOTALS:
        for _ in range(per_total):
            ref = random_reference(rng, total)
            for _ in range(reads_per_ref):
                out.append((ref, random_read(rng, ref)))
    return tuple(out)


def by_reference(pairs):
    """{ungapped reference: ([reference strings], [read strings])} in the order given: find_errors takes alignments of
    one reference sequence only"""
    groups = {}
    for ref, read in pairs:
        g = groups.setdefault(ref.replace("-", ""), ([], []))
        g[0].append(ref); g[1].append(read)
    return groups


def coverage(strings):
    """What a list of gapped strings holds of the situations a 64-character walk treats apart, read off the strings:
    full steps that are all gaps, full steps that hold bases and no run start (a run start: a base that differs from the
    base before it, gaps skipped), the longest gap run and the longest run (in bases), the run starts on a step's first
    character, the run ends (a run's last base) on a step's last character, and the sets of gap-run and run lengths."""
    c = {"all_gap_steps": 0, "no_start_steps": 0, "longest_gap_run": 0, "longest_run": 0, "starts_at_lane_0": 0,
         "ends_at_lane_63": 0, "gap_run_lengths": set(), "run_lengths": set()}
    for s in strings:
        starts, ends, runs = [], [], []     # indices of run starts and of runs' last bases; bases per run
        prev, last = "", -1
        for i, ch in enumerate(s):
            if ch == "-":
                continue
            if ch != prev:
                if last >= 0:
                    ends.append(last)
                starts.append(i); runs.append(0)
            runs[-1] += 1
            prev, last = ch, i
        if last >= 0:
            ends.append(last)
        c["run_lengths"].update(runs)
        c["starts_at_lane_0"] += sum(1 for i in starts if i % STEP == 0)
        c["ends_at_lane_63"] += sum(1 for i in ends if i % STEP == STEP - 1)
        g = 0
        for ch in s + "A":
            if ch == "-":
                g += 1
            elif g:
                c["gap_run_lengths"].add(g); g = 0
        is_start = set(starts)
        for x0 in range(0, len(s) - STEP + 1, STEP):
            step = s[x0:x0 + STEP]
            if step == "-" * STEP:
                c["all_gap_steps"] += 1
            elif not any(x in is_start for x in range(x0, x0 + STEP)):
                c["no_start_steps"] += 1
    c["longest_gap_run"] = max(c["gap_run_lengths"], default=0)
    c["longest_run"] = max(c["run_lengths"], default=0)
    return c
