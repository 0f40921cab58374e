"""Output of unaligned BAM from resident reads: the device route (records packed by k_bamw_*, deflated by k_bgzf_deflate
with the SEQ and QUAL starts as piece boundaries) against its floors and against the host route.

The generator's reads (tools/perf_bgzf_ingest.py: uniform ACGT bases, qualities from error probabilities ~ U(0, 0.06)
as Phred+33, a 36-byte name line of which BAM keeps 12 bytes) at 200, 2 000 and 100 000 bases, about --mb MB of FASTQ
text repeated --repeat times.  One child process per read length, each under its own time limit:

  f  k_bamw_size (+ scan and cuts) and k_bamw_format by HIP events, beside sarlacc_dev_copy of the same output bytes
     (the floor tools/perf_bam_reads.py also uses)
  k  k_bgzf_deflate on the records by HIP events: mode 0 with the cuts, mode 0 without (= mode 1); compressed sizes with
     cuts, without, and of zlib level 6 and Z_HUFFMAN_ONLY on the same 65 280-byte blocks (the first --mb MB)
  w  DeviceReads.to_bam against DeviceReads.to_fastq(compress=True), both to /dev/shm
  h  the host route a user has today: download(), a numpy pack of the records, zlib level 6 on 16 threads into BGZF blocks

    python tools/perf_bam_write.py [--mb 32] [--repeat 8] [--limit 240] [--out profiles/bam_write.txt]
"""
import argparse
import gzip
import os
import subprocess
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from tools.perf_bgzf_ingest import BLOCK, THREADS, synth

SHM = "/dev/shm"
LENGTHS = (200, 2000, 100000)


def say(out, line):
    print(line, flush=True)
    with open(out, "a") as fh:
        fh.write(line + "\n")


def zlib_block(level, strategy=zlib.Z_DEFAULT_STRATEGY):
    def work(data):
        c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
        return len(c.compress(data)) + len(c.flush()) + 26
    return work


def host_records(seq, qual, n, L, period):
    """The records of n reads of L bases named read_0000000 ... (the numbers start again every `period` reads), packed with
    numpy: what a user would write today."""
    name = b"read_0000000\0"
    size = 36 + len(name) + (L + 1) // 2 + L
    rec = np.zeros((n, size), np.uint8)
    fixed = np.array([size - 4, -1, -1, len(name) | (4680 << 16), 4 << 16, L, -1, -1, 0], np.int64).astype(np.uint32)
    rec[:, :36] = fixed.view(np.uint8)
    rec[:, 36:36 + len(name)] = np.frombuffer(name, np.uint8)
    idx = np.arange(n) % period
    for d in range(7):
        rec[:, 36 + 11 - d] = 48 + (idx // 10 ** d) % 10
    lut = np.zeros(256, np.uint8)
    for code, letter in enumerate(b"=ACMGRSVTWYHKDBN"):
        lut[letter] = code
    codes = np.zeros((n, L + (L & 1)), np.uint8)
    codes[:, :L] = lut[seq.reshape(n, L)]
    o = 36 + len(name)
    rec[:, o:o + (L + 1) // 2] = (codes[:, 0::2] << 4) | codes[:, 1::2]
    rec[:, o + (L + 1) // 2:] = qual.reshape(n, L) - 33
    return rec.reshape(-1)


def one_length(args, L):
    import sarlacc_amd
    from sarlacc_amd import _lib, bgzf
    from sarlacc_amd._lib import check
    from sarlacc_amd.resident import DevBuffer, DeviceReads
    lib, out = _lib.lib(), args.out
    text, nrec = synth(args.mb << 20, L, np.random.default_rng(1000))
    d_text = DevBuffer.from_numpy(np.tile(text, args.repeat))
    reads = DeviceReads._from_device_text(d_text, text.size * args.repeat, None)
    n = len(reads)
    assert n == nrec * args.repeat
    del d_text
    tag = "%d-base reads" % L

    # f: the size pass, the format pass, the copy of the same bytes
    plan = reads._write_plan(None, bam=True)
    names, noff, rec_off, cuts, total = plan.names, plan.noff, plan.rec_off, plan.cuts, int(plan.ro[-1])
    say(out, "%s: %d reads, %.3f GB of bases and qualities -> %.3f GB of records" % (tag, n, 2 * reads.total / 1e9, total / 1e9))
    d_rec, d_copy = DevBuffer(total), DevBuffer(total)
    size_ms, format_ms, copy_ms = [], [], []
    for _ in range(3):
        reads._write_plan(None, bam=True)
        size_ms.append(_lib.stage_ms("bam_format_size"))
        check(lib.sarlacc_dev_bam_format(reads.seq, reads.qual, reads.off, names, noff, 1, rec_off, 0, n, d_rec, None))
        format_ms.append(_lib.stage_ms("bam_format"))
        t0 = time.perf_counter()
        check(lib.sarlacc_dev_copy(d_copy, d_rec, total, None))
        copy_ms.append((time.perf_counter() - t0) * 1e3)
    moved = 2 * reads.total + total       # bases and qualities read once, records written once
    say(out, "f %s: k_bamw_size + scan + cuts %.2f ms | k_bamw_format %.2f ms = %.1f GB/s algorithmic (%.3f GB read and "
        "written) | sarlacc_dev_copy of the output bytes %.2f ms (wall) | format / copy %.2f"
        % (tag, min(size_ms), min(format_ms), moved / min(format_ms) / 1e6, moved / 1e9, min(copy_ms), min(format_ms) / min(copy_ms)))
    head = d_rec.to_numpy(np.uint8, min(total, args.mb << 20)).tobytes()
    seq, qual = reads.download()
    want = host_records(seq.chars[:reads.total], qual.chars[:reads.total], n, L, nrec)
    assert head == want[:len(head)].tobytes(), "the records are not what the numpy pack gives"

    # k: the deflate kernel with and without the cuts
    d_comp = None
    for label, kw in (("with cuts", {"cuts": (cuts, 2 * n)}), ("without cuts", {"cuts": (None, 0)}), ("mode 1", {"mode": 1})):
        best, nbytes = [], 0
        for _ in range(2):
            d_comp, nbytes = bgzf.deflate_device(d_rec, total, out=d_comp, **kw)
            best.append(sarlacc_amd.last_kernel_ms())
        if label == "with cuts":
            part = d_comp.to_numpy(np.uint8, nbytes)[:8 << 20].tobytes()
            used = bgzf.scan(part)[1]
            assert gzip.decompress(part[:used]) == head[:len(gzip.decompress(part[:used]))], "the blocks do not decode to the records"
        say(out, "k %s, %s: k_bgzf_deflate %.2f ms by HIP events | %.2f GB/s of records | %.3f GB -> %.3f GB, ratio %.4f"
            % (tag, label, min(best), total / min(best) / 1e6, total / 1e9, nbytes / 1e9, nbytes / total))
    blocks = [head[i:i + BLOCK] for i in range(0, len(head), BLOCK)]
    with ThreadPoolExecutor(THREADS) as pool:
        for label, work in (("level 6", zlib_block(6)), ("Z_HUFFMAN_ONLY", zlib_block(6, zlib.Z_HUFFMAN_ONLY))):
            say(out, "k %s, zlib %s on the same blocks (the first %.0f MB): ratio %.4f"
                % (tag, label, len(head) / 1e6, sum(pool.map(work, blocks)) / len(head)))
    del d_comp, d_copy, d_rec

    # w: whole files
    path = os.path.join(SHM, "perf_bam_write.%d" % os.getpid())
    try:
        for _ in range(2):
            t0 = time.perf_counter()
            written = reads.to_bam(path)
            dt = time.perf_counter() - t0
            say(out, "w %s, to_bam: %.1f ms | %.3f GB of records -> %.3f GB written | %.2f GB/s of records"
                % (tag, dt * 1e3, total / 1e9, written / 1e9, total / dt / 1e9))
            t0 = time.perf_counter()
            written = reads.to_fastq(path, compress=True)
            dt = time.perf_counter() - t0
            say(out, "w %s, to_fastq(compress=True): %.1f ms | %.3f GB written" % (tag, dt * 1e3, written / 1e9))
    finally:
        if os.path.exists(path):
            os.remove(path)

    # h: the host route
    t0 = time.perf_counter()
    seq, qual = reads.download()
    t1 = time.perf_counter()
    rec = host_records(seq.chars[:reads.total], qual.chars[:reads.total], n, L, nrec)
    t2 = time.perf_counter()
    view = memoryview(rec)
    spans = [(i, min(i + BLOCK, rec.size)) for i in range(0, rec.size, BLOCK)]
    work = zlib_block(6)
    with ThreadPoolExecutor(THREADS) as pool:
        size = sum(pool.map(lambda s: work(view[s[0]:s[1]]), spans, chunksize=64))
    t3 = time.perf_counter()
    say(out, "h %s: download %.1f ms | numpy pack %.1f ms | zlib level 6 on %d threads %.1f ms (ratio %.4f) | together %.1f ms"
        % (tag, (t1 - t0) * 1e3, (t2 - t1) * 1e3, THREADS, (t3 - t2) * 1e3, size / rec.size, (t3 - t0) * 1e3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=32)
    ap.add_argument("--repeat", type=int, default=8)
    ap.add_argument("--limit", type=int, default=240, help="seconds per read length")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bam_write.txt"))
    ap.add_argument("--length", type=int, help="run one read length in this process")
    args = ap.parse_args()
    if args.length is None:
        open(args.out, "w").close()
        say(args.out, "tools/perf_bam_write.py --mb %d --repeat %d: %d-byte blocks, %d host threads" % (args.mb, args.repeat, BLOCK, THREADS))
        for L in LENGTHS:     # a fresh process per read length, each under its own limit; nothing runs after a failure
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--mb", str(args.mb), "--repeat", str(args.repeat),
                                 "--out", args.out, "--length", str(L)], timeout=args.limit).returncode
            if rc:
                sys.exit("read length %d failed with status %d" % (L, rc))
        return
    one_length(args, args.length)


if __name__ == "__main__":
    main()
