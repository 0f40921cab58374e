"""sequenceGroups on resident reads: its kernels beside a copy of the read bytes, the whole call, and what the default
parameters make of reads with the mock error process.

Workload: --molecules transcripts (default 100 000) of --length random bases (default 2 000), each observed --copies
times (default 10: 10^6 reads) through devsynth.make_molecule_reads (substitutions by a uniform base, indel events),
generated in HBM, in transcript order, all on one strand.

  k lines  the stage timers of the C calls (HIP events on the stream, best of --repeats): sketch_reads (k_sketch),
           sketch_entries_sort, sketch_pairs, sketch_pairs_sort, sketch_select, components, labels_csr, beside a
           device-to-device copy of the read bytes (HIP events): the floor for k_sketch, which reads every base once.
  w lines  generics.sequenceGroups end to end on the resident batch, downloads of the labels and groups included.
  q lines  at the mock error rates (5 % substitutions + 1 % indel events) and at twice that, for k = 13 (the default)
           with min_shared 3 (the default), 2 and 4, and for k = 16 and 21: groups, the share of transcripts whose
           reads lie in several groups, the share of groups that hold reads of several transcripts, reads without a
           group, candidate pairs, links, rounds of the component kernels.

    python tools/perf_sequence_groups.py [--molecules 100000] [--copies 10] [--length 2000] [--out profiles/sequence_groups.txt]

With --verify the alignment check of the links (identity=, DESIGN §4.19 rule 6a) is measured instead, into
profiles/sequence_groups_verify.txt, on the same reads at both error rates:

  v lines  for min_shared 3, 2 and 1 with identity 0.8 and 0.7 (k = 13, bandwidth 100): n.links, n.verified, the pairs
           whose second strand was computed, the stage timer sketch_verify (HIP events, best of --repeats), links per
           second, band cells per second -- the (2 w + 1) x |b| cells of the links that PASS alone, a lower bound of the
           work: a failing link stops early and is not counted --, the whole call, and the two quality shares of the q
           lines.  A setting whose first call takes more than --slow seconds is not repeated.
  p lines  identity=None, whole call and stage timers, of the package under --root DIR (default: this tree), appended to
           --out: how a parent commit is held beside this one, like for like:

    python tools/perf_sequence_groups.py --verify
    python tools/perf_sequence_groups.py --verify --root . --label "this tree"
    python tools/perf_sequence_groups.py --verify --root ../parent --label "parent commit"
"""
import argparse
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAGES = ("sketch_reads", "sketch_entries_sort", "sketch_pairs", "sketch_pairs_sort", "sketch_select", "components", "labels_csr")


def say(out, line):
    print(line, flush=True)
    with open(out, "a") as fh:
        fh.write(line + "\n")


def resident(sim):
    """The tensors of devsynth.make_molecule_reads as a DeviceReads that borrows them."""
    from sarlacc_amd.resident import DevBuffer, DeviceReads
    seq, qual, off = sim["seq"], sim["qual"], sim["off"]
    return DeviceReads(DevBuffer.borrow(seq.data_ptr(), seq.numel()), DevBuffer.borrow(qual.data_ptr(), qual.numel()),
                       DevBuffer.borrow(off.data_ptr(), 8 * off.numel()), off.cpu().numpy(), None)


def quality(group, copies):
    """(groups, share of transcripts in several groups, share of groups with several transcripts, reads without a group)."""
    transcript = np.arange(group.size) // copies
    kept = group >= 0
    pairs = np.unique(np.stack([transcript[kept], group[kept]], axis=1), axis=0)
    per_transcript = np.bincount(pairs[:, 0], minlength=group.size // copies)
    per_group = np.bincount(pairs[:, 1])
    return per_group.size, float((per_transcript > 1).mean()), float((per_group > 1).mean()), int((~kept).sum())


def verify_lines(args, out):
    """The v lines."""
    import torch

    from sarlacc_amd import _lib, devsynth, generics, sketch
    bandwidth = 100
    say(out, "tools/perf_sequence_groups.py --verify --molecules %d --copies %d --length %d --repeats %d" % (args.molecules, args.copies, args.length, args.repeats))
    for scale in (1, 2):
        sub, indel = 0.05 * scale, 0.01 * scale
        sim = devsynth.make_molecule_reads(args.molecules, args.copies, args.length, 1000 + scale, torch.device("cuda:0"), sub_rate=sub, indel_rate=indel)
        dev = resident(sim)
        lengths = np.diff(dev.off_host)
        say(out, "%d reads of %d transcripts, %.1f MB of bases, %.0f %% substitutions + %.0f %% indel events" % (len(dev), args.molecules, dev.total / 1e6, 100 * sub, 100 * indel))
        for min_shared in (3, 2, 1):
            for identity in (0.8, 0.7):
                walls, stage = [], []
                for _ in range(args.repeats):
                    t0 = time.perf_counter()
                    res = generics.sequenceGroups(dev, min_shared=min_shared, identity=identity, bandwidth=bandwidth)
                    walls.append((time.perf_counter() - t0) * 1e3)
                    stage.append(_lib.stage_ms("sketch_verify"))
                    if walls[0] > 1e3 * args.slow:
                        break
                second = int(_lib.stage_count("sketch_verify_second_strand"))
                assert int(_lib.stage_count("sketch_verify_pairs")) == int(res["n.links"])
                # the passing links once more, for the cells they stand for
                d_sketch, _ = sketch.sketch_reads(dev.seq, dev.off, len(dev), 13, 64, True)
                d_links, _, nlinks = sketch.sketch_links(d_sketch, len(dev), 64, 8, min_shared)
                d_kept, nkept, _, _ = sketch.verify_links(dev.seq, dev.off, len(dev), d_links, nlinks, identity, bandwidth)
                assert nkept == int(res["n.verified"]) and nlinks == int(res["n.links"])
                second_reads = (d_kept.to_numpy(np.uint64, nkept) & np.uint64(0xffffffff)).astype(np.int64)
                cells = float(lengths[second_reads].sum()) * (2 * bandwidth + 1)
                del d_sketch, d_links, d_kept, second_reads
                groups, split, mixed, none = quality(res["group"], args.copies)
                ms = min(stage)
                say(out, "v min_shared %d, identity %.1f: %d links, %d verified, %d second strands, sketch_verify %.3f ms (best of %d; %s), %.1f M links/s, "
                    "%.2f T band cells/s, whole call %.1f ms (best of %d), %d groups, transcripts in several groups %.4f, groups with several transcripts %.4f"
                    % (min_shared, identity, nlinks, nkept, second, ms, len(stage), " ".join("%.3f" % v for v in stage), nlinks / ms / 1e3,
                       cells / ms / 1e9, min(walls), len(walls), groups, split, mixed))
        del dev, sim
        torch.cuda.empty_cache()


def parent_lines(args, out):
    """The p lines: identity=None of the package under --root."""
    import torch

    from sarlacc_amd import _lib, devsynth, generics
    label = args.label or os.path.basename(os.path.abspath(args.root))
    sim = devsynth.make_molecule_reads(args.molecules, args.copies, args.length, 1001, torch.device("cuda:0"), sub_rate=0.05, indel_rate=0.01)
    dev = resident(sim)
    stage, walls = {s: [] for s in STAGES}, []
    generics.sequenceGroups(dev)
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        res = generics.sequenceGroups(dev)
        walls.append((time.perf_counter() - t0) * 1e3)
        for s in STAGES:
            stage[s].append(_lib.stage_ms(s))
    say(out, "p [%s] identity=None on %d reads: whole call %s ms (best %.1f); %s; all stages %.3f ms; %d links, keys %s, sketch_verify_pairs %d"
        % (label, len(dev), " ".join("%.1f" % v for v in walls), min(walls), ", ".join("%s %.3f" % (s, min(stage[s])) for s in STAGES),
           sum(min(stage[s]) for s in STAGES), int(res["n.links"]), " ".join(sorted(res)), int(_lib.stage_count("sketch_verify_pairs"))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--molecules", type=int, default=100000)
    ap.add_argument("--copies", type=int, default=10)
    ap.add_argument("--length", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out")
    ap.add_argument("--verify", action="store_true", help="measure the alignment check of the links (v lines)")
    ap.add_argument("--slow", type=float, default=20.0, help="--verify: seconds above which a setting is run once only")
    ap.add_argument("--root", help="--verify: the p lines of the package of this checkout, appended to --out")
    ap.add_argument("--label", help="what the p lines call that checkout (default: its directory's name)")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root) if args.root else HERE)
    if args.out is None:
        args.out = os.path.join(HERE, "profiles", "sequence_groups_verify.txt" if args.verify else "sequence_groups.txt")
    if args.verify:
        if args.root:
            return parent_lines(args, args.out)
        open(args.out, "w").close()
        return verify_lines(args, args.out)
    import torch

    from sarlacc_amd import _lib, devsynth, generics
    out = args.out
    open(out, "w").close()
    say(out, "tools/perf_sequence_groups.py --molecules %d --copies %d --length %d --repeats %d" % (args.molecules, args.copies, args.length, args.repeats))
    device = torch.device("cuda:0")
    for scale in (1, 2):
        sub, indel = 0.05 * scale, 0.01 * scale
        sim = devsynth.make_molecule_reads(args.molecules, args.copies, args.length, 1000 + scale, device, sub_rate=sub, indel_rate=indel)
        dev = resident(sim)
        n, nbytes = len(dev), dev.total
        say(out, "%d reads of %d transcripts, %.1f MB of bases, %.0f %% substitutions + %.0f %% indel events" % (n, args.molecules, nbytes / 1e6, 100 * sub, 100 * indel))
        for k, min_shared in ((13, 3), (13, 2), (13, 4), (16, 3), (21, 3), (21, 2)):
            t0 = time.perf_counter()
            res = generics.sequenceGroups(dev, k=k, min_shared=min_shared)
            wall = (time.perf_counter() - t0) * 1e3
            groups, split, mixed, none = quality(res["group"], args.copies)
            say(out, "q k %d, min_shared %d: %d groups, transcripts in several groups %.4f, groups with several transcripts %.4f, reads without a group %d, "
                "%d candidate pairs, %d links, %d component rounds (%.0f ms)"
                % (k, min_shared, groups, split, mixed, none, int(res["n.pairs"]), int(res["n.links"]), int(_lib.stage_count("components_rounds")), wall))
        if scale == 2:
            break
        stage, walls = {s: [] for s in STAGES}, []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            generics.sequenceGroups(dev)
            walls.append((time.perf_counter() - t0) * 1e3)
            for s in STAGES:
                stage[s].append(_lib.stage_ms(s))
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
        for s in STAGES:
            say(out, "k %-20s %8.3f ms (best of %d; %s)" % (s, min(stage[s]), len(stage[s]), " ".join("%.3f" % v for v in stage[s])))
        say(out, "k sketch_reads = %.2f x the copy, %.1f GB/s of bases; all stages together %.3f ms"
            % (min(stage["sketch_reads"]) / min(copy), nbytes / min(stage["sketch_reads"]) / 1e6, sum(min(stage[s]) for s in STAGES)))
        say(out, "w sequenceGroups end to end %s ms (best %.1f)" % (" ".join("%.1f" % v for v in walls), min(walls)))
        del dev, sim
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
