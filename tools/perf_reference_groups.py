"""referenceGroups on resident reads: its stages beside a copy of the read bytes and beside sequenceGroups(identity=0.8)
on the same reads, the whole call, and what it makes of reads with the mock error process.

Workload: --molecules transcripts (default 100 000) of --length random bases (default 2 000), each observed --copies
times (default 10: 10^6 reads) through devsynth.make_molecule_reads (substitutions by a uniform base, indel events),
generated in HBM, in transcript order, all on one strand; the transcripts themselves are the references.

  k lines  the stage timers of the C calls (HIP events on the stream, best of --repeats): sketch_reads of the references
           and of the reads (k_sketch), refmap_entries_sort, refmap_probe (directory, count, scan, fill),
           refmap_hits_sort, refmap_select, refmap_candidates (the four together, host waits included), refmap_assign,
           labels_csr, beside a device-to-device copy of the read bytes (HIP events).
  w lines  generics.referenceGroups end to end on the resident batch, downloads included (host clock, best of
           --repeats), and generics.sequenceGroups(identity=0.8) on the same reads.
  q lines  at the mock error rates (5 % substitutions + 1 % indel events) and at twice that, with identity 0.8 and with
           identity=None: the share of reads on their own transcript, the share unmapped, hits, candidates checked,
           second strands.

    python tools/perf_reference_groups.py [--molecules 100000] [--copies 10] [--length 2000] [--out profiles/reference_groups.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
CANDIDATE_STAGES = ("refmap_entries_sort", "refmap_probe", "refmap_hits_sort", "refmap_select", "refmap_candidates")


def say(out, line):
    print(line, flush=True)
    with open(out, "a") as fh:
        fh.write(line + "\n")


def resident(seq, qual, off):
    """Device tensors as a DeviceReads that borrows them."""
    from sarlacc_amd.resident import DevBuffer, DeviceReads
    return DeviceReads(DevBuffer.borrow(seq.data_ptr(), seq.numel()), DevBuffer.borrow(qual.data_ptr(), qual.numel()),
                       DevBuffer.borrow(off.data_ptr(), 8 * off.numel()), off.cpu().numpy(), None)


def stage_lines(dev, refs, repeats, out):
    """The k lines: the calls of refmap.reference_groups one by one, each stage timer read after its call."""
    from sarlacc_amd import _lib, groups, refmap, sketch
    n, nf = len(dev), len(refs)
    ms = {}

    def note(name, value=None):
        ms.setdefault(name, []).append(_lib.stage_ms(name) if value is None else value)
    for _ in range(repeats):
        fsk, _ = sketch.sketch_reads(refs.seq, refs.off, nf, 13, 64, True)
        note("sketch_reads (references)", _lib.stage_ms("sketch_reads"))
        rsk, _ = sketch.sketch_reads(dev.seq, dev.off, n, 13, 64, True)
        note("sketch_reads (reads)", _lib.stage_ms("sketch_reads"))
        cand_ref, cand_shared, _, _ = refmap.sketch_candidates(fsk, nf, rsk, n, 64, 2, 4)
        for s in CANDIDATE_STAGES:
            note(s)
        (reference, _, _, _), _ = refmap.candidates_assign(refs.seq, refs.off, nf, dev.seq, dev.off, n, cand_ref, cand_shared, 4, 100, 200000, True)
        note("refmap_assign")
        groups.labels_csr(reference, n)
        note("labels_csr")
    for name, values in ms.items():
        say(out, "k %-26s %9.3f ms (best of %d; %s)" % (name, min(values), len(values), " ".join("%.3f" % v for v in values)))
    return {name: min(values) for name, values in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--molecules", type=int, default=100000)
    ap.add_argument("--copies", type=int, default=10)
    ap.add_argument("--length", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "reference_groups.txt"))
    args = ap.parse_args()
    import torch

    from sarlacc_amd import _lib, devsynth, generics
    out = args.out
    open(out, "w").close()
    say(out, "tools/perf_reference_groups.py --molecules %d --copies %d --length %d --repeats %d" % (args.molecules, args.copies, args.length, args.repeats))
    device = torch.device("cuda:0")
    for scale in (1, 2):
        sub, indel = 0.05 * scale, 0.01 * scale
        sim = devsynth.make_molecule_reads(args.molecules, args.copies, args.length, 1000 + scale, device, sub_rate=sub, indel_rate=indel, keep_truth=True)
        dev = resident(sim["seq"], sim["qual"], sim["off"])
        truth = sim["truth"].reshape(-1)
        refs = resident(truth, truth, torch.arange(args.molecules + 1, dtype=torch.int64, device=device) * args.length)
        n, nbytes = len(dev), dev.total
        own = np.arange(n) // args.copies
        say(out, "%d reads of %d transcripts, %.1f MB of bases, %.0f %% substitutions + %.0f %% indel events; the transcripts are the references"
            % (n, args.molecules, nbytes / 1e6, 100 * sub, 100 * indel))
        for identity in (0.8, None):
            t0 = time.perf_counter()
            res = generics.referenceGroups(dev, refs, identity=identity)
            wall = (time.perf_counter() - t0) * 1e3
            say(out, "q identity %s: reads on their own transcript %.6f, unmapped %.6f, on another %d; %d hits, %d candidates kept, %d checked, %d second strands (%.0f ms)"
                % (identity, float((res["reference"] == own).mean()), float((res["reference"] < 0).mean()),
                   int(((res["reference"] >= 0) & (res["reference"] != own)).sum()), int(res["n.hits"]), int(res["n.candidates"].sum()),
                   int(res.get("n.checked", 0)), int(_lib.stage_count("refmap_second_strand")), wall))
        if scale == 2:
            break
        best = stage_lines(dev, refs, args.repeats, out)
        copy, target = [], torch.empty_like(sim["seq"])
        for _ in range(args.repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            target.copy_(sim["seq"])
            b.record()
            torch.cuda.synchronize()
            copy.append(a.elapsed_time(b))
        del target
        say(out, "k device copy of the %.1f MB of bases: %.3f ms (HIP events, best of %d)" % (nbytes / 1e6, min(copy), args.repeats))
        stages = sum(v for name, v in best.items() if name not in CANDIDATE_STAGES[:4])
        say(out, "k all stages together %.3f ms = %.1f x the copy; refmap_assign alone %.1f x the copy" % (stages, stages / min(copy), best["refmap_assign"] / min(copy)))
        walls = {"referenceGroups": [], "sequenceGroups(identity=0.8)": []}
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            generics.referenceGroups(dev, refs)
            walls["referenceGroups"].append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            generics.sequenceGroups(dev, identity=0.8)
            walls["sequenceGroups(identity=0.8)"].append((time.perf_counter() - t0) * 1e3)
        for name, values in walls.items():
            say(out, "w %s end to end %s ms (best %.1f)" % (name, " ".join("%.1f" % v for v in values), min(values)))
        del dev, refs, sim, truth
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
