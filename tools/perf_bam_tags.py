"""BAM tags on the device against their floors: the aux extract, the find pass and one splice (replace RX) beside
sarlacc_dev_copy of the bytes each moves and beside k_bgzf_inflate of the same file; k_bamw_format with and without tags
beside the copy of its output; the deflate ratio with 3 n cuts, 2 n cuts and one table per block; from_bam and to_bam
wall time with and without tags.

Reads of 200, 2 000 and 100 000 uniform ACGT bases (qualities from error probabilities ~ U(0, 0.06)), about --mb MB
(default 192: 0.2 GB) of records per length, with a basecaller-like tag set: a dozen short i / f / Z tags, RG:Z,
mv:B:c of one entry per 6 bases, MM:Z and ML:B:C of one call per 25 bases, and RX:Z; and the 2 000-base reads once more
with RX:Z and BC:Z alone ("umi").  --distinct reads are drawn per case and repeated.  One child process per case, each under its own time limit;
HIP events (the library's stage timers) where a kernel is timed, best of three.

    python tools/perf_bam_tags.py [--mb 192] [--limit 240] [--out profiles/bam_tags.txt]

With --root DIR the package of the checkout DIR (built there) is measured instead, and only the tag-free to_bam and
from_bam walls, which every version has ("p" lines, appended to --out, in a process that does nothing else).  That is
how a parent commit is held beside this one, like for like:

    python tools/perf_bam_tags.py --root . --label "this tree"
    python tools/perf_bam_tags.py --root ../parent --label "parent commit"
"""
import argparse
import os
import struct
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHM = "/dev/shm"
LABEL = [""]
CASES = (("200", 200, "full"), ("2000", 2000, "full"), ("100000", 100000, "full"), ("umi", 2000, "umi"))


def say(out, line):
    print(line, flush=True)
    with open(out, "a") as fh:
        fh.write(line + "\n")


def z(tag, value):
    return tag + b"Z" + value + b"\0"


def aux_of(rng, L, k, kind):
    """The aux bytes of read k."""
    umi = z(b"RX", bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 12)))
    if kind == "umi":
        return umi + z(b"BC", b"barcode%02d" % (k % 96))
    f32 = lambda v: struct.pack("<f", v)      # noqa: E731
    nmod = L // 25
    mv = rng.integers(0, 2, L // 6).astype(np.uint8).tobytes()
    mm = b"C+m?" + b"".join(b",%d" % v for v in rng.integers(0, 30, nmod)) + b";"
    return b"".join([b"qsf" + f32(rng.uniform(5, 30)), b"duf" + f32(rng.uniform(0.1, 20)), b"nsi" + struct.pack("<i", 6 * L),
                     b"tsS" + struct.pack("<H", int(rng.integers(0, 500))), b"mxC\x01", b"chS" + struct.pack("<H", k % 512),
                     z(b"st", b"2026-01-01T00:00:%02d.000+00:00" % (k % 60)), b"rni" + struct.pack("<i", k), z(b"fn", b"file_%d.pod5" % (k % 7)),
                     b"smf" + f32(rng.normal(90, 5)), b"sdf" + f32(rng.normal(20, 2)), z(b"sv", b"pa"), z(b"RG", b"run1_model_v5"), umi,
                     b"mvBc" + struct.pack("<I", 1 + len(mv)) + b"\x06" + mv, z(b"MM", mm),
                     b"MLBC" + struct.pack("<I", nmod) + rng.integers(0, 256, nmod).astype(np.uint8).tobytes()])


def make_batch(args, L, kind):
    """(resident batch with names, its tags) of about args.mb MB of records."""
    from sarlacc_amd.generics import Reads
    from sarlacc_amd.resident import DeviceReads
    from sarlacc_amd.strset import StringSet, StrList
    rng = np.random.default_rng(1000)
    distinct = max(min(args.distinct, (args.mb << 20) // (2 * L)), 1)
    areas = [aux_of(rng, L, k, kind) for k in range(distinct)]
    per_read = 36 + 13 + (L + 1) // 2 + L + sum(map(len, areas)) // distinct
    repeat = max((args.mb << 20) // (per_read * distinct), 1)
    n = distinct * repeat
    seq = np.tile(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (distinct, L))], (repeat, 1))
    err = np.maximum(rng.random((distinct, L)) * 0.06, 1e-9)
    qual = np.tile((33 + np.clip(np.rint(-10 * np.log10(err)), 0, 60)).astype(np.uint8), (repeat, 1))
    reads = DeviceReads.upload(Reads(StringSet.from_matrix(seq), StringSet.from_matrix(qual)))
    reads.names = StrList(StringSet.from_matrix(np.frombuffer(b"".join(b"read_%07d" % (k % 10 ** 7) for k in range(n)), np.uint8).reshape(n, 12)))
    return reads, areas * repeat


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def copy_ms(lib, check, nbytes):
    from sarlacc_amd.resident import DevBuffer
    a, b = DevBuffer(max(nbytes, 1)), DevBuffer(max(nbytes, 1))
    return min(timed(lambda: check(lib.sarlacc_dev_copy(a, b, nbytes, None)))[0] for _ in range(3))


def walls(out, label, reads, path, keep_tags_ok):
    """to_bam and from_bam wall times, best of three, tag-free and (where the package has them) with tags."""
    from sarlacc_amd.resident import DeviceReads
    rows = []
    for tags in ((False, True) if keep_tags_ok and getattr(reads, "tags", None) is not None else (False,)):
        held = getattr(reads, "tags", None)
        if not tags and keep_tags_ok:
            reads.tags = None
        w = [timed(lambda: reads.to_bam(path)) for _ in range(3)]
        kw = {"keep_tags": True} if tags else {}
        r = [timed(lambda: DeviceReads.from_bam(path, **kw))[0] for _ in range(3)]
        if keep_tags_ok:
            reads.tags = held
        rows.append((tags, w, r))
        say(out, "%s %s, %s: to_bam %s ms (best %.1f, %.3f GB written) | from_bam %s ms (best %.1f)"
            % ("w" if keep_tags_ok else "p [%s]" % LABEL[0], label, "with tags" if tags else "tag-free", " ".join("%.1f" % t for t, _ in w), min(t for t, _ in w),
               w[0][1] / 1e9, " ".join("%.1f" % t for t in r), min(r)))
    return rows


def one_case(args, label, L, kind):
    sys.path.insert(0, args.root or HERE)
    import sarlacc_amd
    from sarlacc_amd import _lib, bgzf, sam
    from sarlacc_amd._lib import check
    from sarlacc_amd.resident import DevBuffer
    assert os.path.dirname(os.path.dirname(os.path.abspath(sarlacc_amd.__file__))) == os.path.abspath(args.root or HERE)
    lib, out = _lib.lib(), args.out
    reads, areas = make_batch(args, L, kind)
    n = len(reads)
    tag = "%s-base reads, %s tags" % (L, kind)
    path = os.path.join(SHM, "perf_bam_tags.%d" % os.getpid())
    try:
        if args.root:      # a named checkout: what every version has
            LABEL[0] = args.label or os.path.basename(os.path.abspath(args.root))
            walls(out, tag, reads, path, False)
            return
        import ctypes as C
        from sarlacc_amd.tags import DeviceTags
        reads.tags = DeviceTags.upload(areas)
        tags, aux_bytes = reads.tags, reads.tags.total
        say(out, "%s: %d reads, %.3f GB of bases and qualities, %.3f GB of tags (%.0f bytes per read)" % (tag, n, 2 * reads.total / 1e9, aux_bytes / 1e9, aux_bytes / n))

        # t: find and splice (replace RX) on the resident tags
        find_ms, splice_ms = [], []
        umis = np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(7).integers(0, 4, (n, 12))]
        from sarlacc_amd.strset import StringSet
        from sarlacc_amd.tags import tag_column
        column = tag_column(StringSet.from_matrix(umis), n)
        for _ in range(3):
            hit = tags.find(b"RX")
            find_ms.append(_lib.stage_ms("bam_tags_find"))
            new = tags.splice(cut=(hit.tag_off, hit.tag_len.to_numpy(np.int64, n).copy()), name=b"RX", column=column)
            splice_ms.append(_lib.stage_ms("bam_tags_splice"))
        assert hit.n_present == n and new.total == aux_bytes
        c1, c2 = copy_ms(lib, check, aux_bytes), copy_ms(lib, check, aux_bytes)
        say(out, "t %s: k_tags_find %.3f ms = %.1f GB/s of tags read | k_tags_splice (replace RX) %.3f ms = %.1f GB/s read + written | "
            "sarlacc_dev_copy of the tag bytes %.3f ms (wall) | find / copy %.2f | splice / copy %.2f"
            % (tag, min(find_ms), aux_bytes / min(find_ms) / 1e6, min(splice_ms), 2 * aux_bytes / min(splice_ms) / 1e6, min(c1, c2),
               min(find_ms) / min(c1, c2), min(splice_ms) / min(c1, c2)))
        del new, hit

        # f: the writer's kernels with and without tags
        for with_tags in (False, True):
            reads.tags = tags if with_tags else None
            size_ms, format_ms = [], []
            plan = reads._write_plan(None, bam=True)
            total = int(plan.ro[-1])
            d_rec = DevBuffer(total)
            aux = (tags.aux, tags.off) if with_tags else ()
            for _ in range(3):
                reads._write_plan(None, bam=True)
                size_ms.append(_lib.stage_ms("bam_format_size"))
                check(plan.format(reads.seq, reads.qual, reads.off, plan.names, plan.noff, 1, *aux, plan.rec_off, 0, n, d_rec, None))
                format_ms.append(_lib.stage_ms("bam_format"))
            c = copy_ms(lib, check, total)
            say(out, "f %s, %s: k_bamw_size + scan + cuts %.3f ms | k_bamw_format %.3f ms for %.3f GB of records = %.1f GB/s written | "
                "sarlacc_dev_copy of the output %.3f ms (wall) | format / copy %.2f"
                % (tag, "with tags" if with_tags else "tag-free", min(size_ms), min(format_ms), total / 1e9, total / min(format_ms) / 1e6, c, min(format_ms) / c))
            if with_tags:      # k: the deflate of the records with tags under three piece rules
                cuts3 = plan.cuts.to_numpy(np.int64, 3 * n)
                cuts2 = DevBuffer.from_numpy(np.ascontiguousarray(cuts3.reshape(n, 3)[:, :2]).reshape(-1))
                d_comp = None
                for what, kw in (("3 n cuts", {"cuts": (plan.cuts, 3 * n)}), ("2 n cuts", {"cuts": (cuts2, 2 * n)}), ("one table per block", {"mode": 1})):
                    d_comp, nbytes = bgzf.deflate_device(d_rec, total, out=d_comp, **kw)
                    say(out, "k %s, %s: %.3f GB -> %.3f GB, ratio %.4f | k_bgzf_deflate %.2f ms"
                        % (tag, what, total / 1e9, nbytes / 1e9, nbytes / total, sarlacc_amd.last_kernel_ms()))
                del d_comp
            del d_rec
        reads.tags = tags

        # w: whole files, with and without tags
        walls(out, tag, reads, path, True)
        reads.to_bam(path)      # (the file with tags, for the extract)

        # x: the aux extract beside the inflate of the same file and the copy of its bytes
        with open(path, "rb") as fh:
            origin = sam.read_bam_header(fh)[2]
            fh.seek(origin[0])
            d_bam, nbytes, _ = bgzf.DeviceTextStream(fh, None, first_block=origin[1], skip=origin[2]).next(None)
        inflate_ms = sarlacc_amd.last_kernel_ms()
        nrec, used, nreads, ab = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)
        extract_ms = []
        for _ in range(3):
            check(lib.sarlacc_dev_bam_reads_index(d_bam, nbytes, 1, 1, 0x900, C.byref(nrec), C.byref(used), C.byref(nreads), None))
            check(lib.sarlacc_dev_bam_reads_aux_range(0, nreads.value, C.byref(ab)))
            aux, aoff = DevBuffer(max(ab.value, 1)), DevBuffer(8 * (nreads.value + 1))
            check(lib.sarlacc_dev_bam_reads_aux_extract(d_bam, 0, nreads.value, aux, aoff, None))
            extract_ms.append(_lib.stage_ms("bam_reads_aux"))
        assert nreads.value == n and ab.value == aux_bytes
        c = copy_ms(lib, check, aux_bytes)
        say(out, "x %s: k_bamr_aux (+ offsets) %.3f ms = %.1f GB/s of tags read + written | sarlacc_dev_copy of the tag bytes %.3f ms (wall) | "
            "extract / copy %.2f | k_bgzf_inflate of the file (%.3f GB inflated) %.2f ms | extract / inflate %.3f"
            % (tag, min(extract_ms), 2 * aux_bytes / min(extract_ms) / 1e6, c, min(extract_ms) / c, nbytes / 1e9, inflate_ms, min(extract_ms) / inflate_ms))
    finally:
        if os.path.exists(path):
            os.remove(path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=192, help="MB of records per case")
    ap.add_argument("--distinct", type=int, default=2048, help="distinct reads per case, repeated to --mb")
    ap.add_argument("--limit", type=int, default=240, help="seconds per case")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "bam_tags.txt"))
    ap.add_argument("--root", help="measure the package of this checkout instead (tag-free walls only)")
    ap.add_argument("--label", help="what the p lines call that checkout (default: its directory's name)")
    ap.add_argument("--case", help="run one case in this process")
    args = ap.parse_args()
    if args.case is None:
        if not args.root:
            open(args.out, "w").close()
        say(args.out, "tools/perf_bam_tags.py --mb %d --distinct %d%s" % (args.mb, args.distinct, " --root: the tag-free walls of [%s]" % (args.label or os.path.basename(os.path.abspath(args.root))) if args.root else ""))
        for label, _, _ in CASES:     # a fresh process per case, each under its own limit; nothing runs after a failure
            cmd = [sys.executable, os.path.abspath(__file__), "--mb", str(args.mb), "--distinct", str(args.distinct), "--out", args.out, "--case", label]
            rc = subprocess.run(cmd + (["--root", args.root, "--label", args.label or ""] if args.root else []), timeout=args.limit).returncode
            if rc:
                sys.exit("case %s failed with status %d" % (label, rc))
        return
    label, L, kind = next(c for c in CASES if c[0] == args.case)
    one_case(args, label, L, kind)


if __name__ == "__main__":
    main()
