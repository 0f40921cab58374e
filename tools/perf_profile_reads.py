"""The profiling workflow (align every read to its reference, then the error and homopolymer profiles) on resident
reads: seeded reads of 2 kb (1 % deletions, 1 % insertions, 5 % substitutions, Phred+33) against their 2-kb
homopolymer-rich reference.  Two routes in one process, alternating, each timed as wall time around a call that ends
with its results on the host:
  (chain) generics.qualityAlign -> errorFinder + homopolymerMatcher: the strings through the host,
  (fused) generics.profileReads on the DeviceReads (sarlacc_dev_profile_reads + sarlacc_profile_fetch).
At every size at which both run, profileReads(expand=True) must equal the chain before any time is printed.  The chain
starts at `first` reads and goes up by factors of 4 until one pass exceeds `chain_limit` seconds; the fused call goes on
alone up to `last`.  For the fused call the stage timers give the DP launches (profile_align), k_profile_pairs
(profile_kernel) and the merge of the events (profile_reduce).

usage: perf_profile_reads.py [first=10000] [last=1000000] [chain_limit=60] [repeats=3]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import sarlacc_amd
from sarlacc_amd import generics
from sarlacc_amd.resident import DeviceReads
from sarlacc_amd.strset import StringSet

R = 2000


def reference(rng):
    ref = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, R)].copy()
    for _ in range(R // 12):
        k = int(rng.integers(0, R - 6))
        ref[k:k + int(rng.integers(2, 7))] = ref[k]
    return ref


def reads(n, ref, rng, block=20000):
    """n reads of R bases: a walk along the reference that skips a base (deletion) or stalls on a random one (insertion)."""
    seq = np.empty((n, R), np.uint8)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    for lo in range(0, n, block):
        m = min(block, n - lo)
        u = rng.random((m, R), dtype=np.float32)
        step = np.ones((m, R), np.int8)
        step[u < 0.01] = 2
        step[(u >= 0.01) & (u < 0.02)] = 0
        idx = np.cumsum(step, axis=1, dtype=np.int32) - 1
        np.clip(idx, 0, R - 1, out=idx)
        part = ref[idx]
        rnd = (step == 0) | (u > 0.95)
        part[rnd] = acgt[rng.integers(0, 4, int(rnd.sum()))]
        seq[lo:lo + m] = part
    off = np.arange(n + 1, dtype=np.int64) * R
    qual = rng.integers(33 + 5, 33 + 41, n * R, dtype=np.uint8)
    return generics.Reads(StringSet(seq.reshape(-1), off), StringSet(qual, off.copy()))


def chain(rd, ref):
    qa = generics.qualityAlign(rd, ref)
    return qa, generics.errorFinder(qa["reference"], qa["query"]), generics.homopolymerMatcher(qa["reference"], qa["query"])


def fused(dev, ref, expand=False):
    out = generics.profileReads(dev, ref, expand=expand)
    return out, {k: sarlacc_amd.stage_ms(k) for k in ("profile_align", "profile_kernel", "profile_reduce")}, sarlacc_amd.stage_count("profile_chunks")


def plain(x):
    if isinstance(x, dict):
        return {k: plain(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [plain(v) for v in x]
    return x.tolist() if isinstance(x, (np.ndarray, np.generic)) else x


def main():
    args = sys.argv[1:]
    first = int(args[0]) if args else 10000
    last = int(args[1]) if len(args) > 1 else 1000000
    chain_limit = float(args[2]) if len(args) > 2 else 60.0
    repeats = int(args[3]) if len(args) > 3 else 3
    if sarlacc_amd.device_count() < 1:
        raise SystemExit("perf_profile_reads needs a HIP device")
    rng = np.random.default_rng(20241)
    refa = reference(rng)
    ref = refa.tobytes().decode()
    print("reads of %d bases against a reference of %d columns, gap opening 5, extension 1; %d timed repeats per route, min-max" % (R, R, repeats))
    n, with_chain = first, True
    while n <= last:
        rd = reads(n, refa, rng)
        dev = DeviceReads.upload(rd)
        cells = float(n) * R * R
        fused(dev, ref)   # warm-up at the timed size
        if with_chain:
            t0 = time.perf_counter(); qa, ef, hm = chain(rd, ref); first_pass = time.perf_counter() - t0
            ex, _, _ = fused(dev, ref, expand=True)
            same = plain(ex["errors"]) == plain(ef) and plain(ex["homopolymers"]) == plain(hm) and \
                np.array_equal(ex["score"].view(np.int64), qa["score"].view(np.int64)) and np.array_equal(ex["edit"], qa["edit"])
            if not same:
                raise SystemExit("the fused call and the chain disagree at %d reads" % n)
        wall = {"chain": [], "fused": []}
        stages = []
        for _ in range(repeats):
            if with_chain:
                t0 = time.perf_counter(); chain(rd, ref); wall["chain"].append(time.perf_counter() - t0)
            t0 = time.perf_counter(); _, st, chunks = fused(dev, ref); wall["fused"].append(time.perf_counter() - t0)
            stages.append(st)
        ms = {k: (min(s[k] for s in stages), max(s[k] for s in stages)) for k in stages[0]}
        line = "n = %8d: fused wall s %.3f-%.3f in %d chunk(s)" % (n, min(wall["fused"]), max(wall["fused"]), chunks)
        if with_chain:
            line += "; chain wall s %.2f-%.2f (identical results); chain/fused %.0f-%.0f x" % (
                min(wall["chain"]), max(wall["chain"]), min(wall["chain"]) / max(wall["fused"]), max(wall["chain"]) / min(wall["fused"]))
        print(line)
        print("      profile_align %.1f-%.1f ms (%.0f GCUPS), profile_kernel %.2f-%.2f ms = %.2f %% of the DP, profile_reduce %.2f-%.2f ms"
              % (*ms["profile_align"], cells / (ms["profile_align"][0] / 1e3) / 1e9, *ms["profile_kernel"],
                 100 * ms["profile_kernel"][0] / ms["profile_align"][0], *ms["profile_reduce"]), flush=True)
        if with_chain and max(wall["chain"] + [first_pass]) > chain_limit:
            with_chain = False
            print("      (a chain pass exceeded %.0f s: the fused call goes on alone)" % chain_limit)
        n *= 4
        if n > last and n < 4 * last and n // 4 != last:
            n = last


if __name__ == "__main__":
    main()
