"""Reads from a BAM file: the size and unpack passes of bam_reads.hip by HIP events next to the locator and the inflate,
a device-to-device copy of the same output bytes as the floor, and the whole DeviceReads.from_bam call against
DeviceReads.from_fastq on a BGZF FASTQ file of the same reads.

The workload is that of tools/perf_bam_ingest.py: its pool of seeded ONT-like records (2-kb reads, 36-character names,
flags 0 / 16 / 4 / 256 / 2048 / 272) compressed into BGZF blocks with zlib level 6 and repeated to about 1 GB of BAM
bytes.  The FASTQ text of the pool is what the device writes for the pool's reads (from_bam + fastq_text), compressed
and repeated the same way, so the two files hold the same reads.  Two routes, each in a child process of its own under
its own time limit:

  k  the loop of DeviceReads.stream_bam driven by hand, every buffer taken whole, so that each call's stage timers can
     be read: k_bgzf_inflate, the locator, bam_reads_size (k_bamr_size, the three scans, k_bamr_reads),
     bam_reads_unpack (k_bamr_offsets, k_bamr_unpack, k_bamr_names), summed over the buffers; then sarlacc_dev_copy of
     the largest buffer's output bytes by the host clock (the call returns when the device has finished)
  w  the whole from_bam call and the whole from_fastq call, alternating, host clock; the two batches must be equal

    python tools/perf_bam_reads.py [--pool 4096] [--gb 1.0] [--length 2000] [--limit 300]
"""
import argparse
import ctypes as C
import os
import subprocess
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from tools import perf_bam_ingest as P


def prepare(pool, gb, folder):
    """Writes x.bam (as perf_bam_ingest does) and x.fastq.gz; returns (paths, records, reads, BAM bytes, FASTQ bytes)."""
    from sarlacc_amd.resident import DeviceReads
    (bam_path, sam_path), nrec, nbytes, _ = P.prepare(pool, gb, folder)
    os.remove(sam_path)
    repeat = nrec // pool
    one = os.path.join(folder, "pool.bam")
    bam, _ = P.pool_records(pool, np.random.default_rng(1000))
    with open(bam_path, "rb") as fh:
        head = fh.read(1 << 16)
    first = head[:int.from_bytes(head[16:18], "little") + 1]          # the header's block
    with open(one, "wb") as fh:
        fh.write(first + P.bgzf(bam) + P.EOF_BLOCK)
    dev = DeviceReads.from_bam(one)
    text = dev.fastq_text()
    blocks = P.bgzf(text)
    fq_path = os.path.join(folder, "x.fastq.gz")
    with open(fq_path, "wb") as fh:
        for _ in range(repeat):
            fh.write(blocks)
        fh.write(P.EOF_BLOCK)
    os.remove(one)
    return [bam_path, fq_path], nrec, len(dev) * repeat, nbytes, len(text) * repeat


def route_k(path, nrec, nreads, nbytes, block_bytes):
    import sarlacc_amd
    from sarlacc_amd import _lib, bgzf as bg, sam
    from sarlacc_amd.resident import DevBuffer
    lib = _lib.lib()
    stages = ["bam_hops", "bam_chain", "bam_starts", "bam_reads_size", "bam_reads_unpack"]
    for rep in range(3):
        ms = dict.fromkeys(["inflate"] + stages, 0.0)
        t0 = time.perf_counter()
        with open(path, "rb") as fh:
            origin = sam.read_bam_header(fh)[2]
            fh.seek(origin[0])
            stream = bg.DeviceTextStream(fh, block_bytes, first_block=origin[1], skip=origin[2])
            record, carry, eof, reads, buffers, bases, name_bytes, largest = 1, None, False, 0, 0, 0, 0, 1
            while not eof:
                d_bam, n, eof = stream.next(carry)
                if d_bam is None or n == 0:
                    break
                ms["inflate"] += sarlacc_amd.last_kernel_ms()
                nr, used, nk = C.c_int64(0), C.c_int64(0), C.c_int64(0)
                _lib.check(lib.sarlacc_dev_bam_reads_index(d_bam, n, record, 1 if eof else 0, 0x900, C.byref(nr), C.byref(used),
                                                           C.byref(nk), None))
                tb, tn, nxt = C.c_int64(0), C.c_int64(0), C.c_int64(0)
                _lib.check(lib.sarlacc_dev_bam_reads_range(0, nk.value, C.byref(tb), C.byref(tn), C.byref(nxt)))
                out = [DevBuffer(max(tb.value, 1)), DevBuffer(max(tb.value, 1)), DevBuffer(8 * (nk.value + 1)), DevBuffer(max(tn.value, 1)),
                       DevBuffer(8 * (nk.value + 1))]
                _lib.check(lib.sarlacc_dev_bam_reads_extract(d_bam, 0, nk.value, 1, *out, None))
                for s in stages:
                    ms[s] += max(sarlacc_amd.stage_ms(s), 0.0)
                record += nr.value
                reads += nk.value
                bases += tb.value
                name_bytes += tn.value
                buffers += 1
                largest = max(largest, 2 * tb.value + tn.value)
                del out
                carry = (d_bam, used.value, n - used.value) if used.value < n else None
        dt = time.perf_counter() - t0
        assert record - 1 == nrec and reads == nreads, (record, nrec, reads, nreads)
        # packed SEQ + QUAL + names read once, seq / qual / names written once
        moved = (bases + 1) // 2 + bases + name_bytes + 2 * bases + name_bytes
        # the floor: the largest buffer's output bytes copied within device memory
        last = largest
        src, dst = DevBuffer(last), DevBuffer(last)
        copy = []
        for _ in range(6):
            t1 = time.perf_counter()
            _lib.check(lib.sarlacc_dev_copy(dst, src, last, None))
            copy.append((time.perf_counter() - t1) * 1e3)
        copy_ms = min(copy[1:]) * (2 * bases + name_bytes) / last     # scaled from that buffer to the whole file
        locator = ms["bam_hops"] + ms["bam_chain"] + ms["bam_starts"]
        print("k rep %d: %d records, %d reads, %d bases in %d buffers of %d MB | by HIP events, summed over the buffers: k_bgzf_inflate "
              "%.2f ms, locator %.2f ms (k_bam_hops %.2f, k_bam_chain %.2f, k_bam_starts %.2f), bam_reads_size %.2f ms, "
              "bam_reads_unpack %.2f ms = %.1f GB/s algorithmic (%.3f GB read and written) | sarlacc_dev_copy of the output "
              "bytes, host clock, best of 5 on the largest buffer scaled to the file: %.2f ms | unpack / inflate = %.3f, "
              "unpack / copy = %.2f, size / inflate = %.3f | the loop %.1f ms (%.2f GB/s of BAM bytes)"
              % (rep, nrec, reads, bases, buffers, block_bytes >> 20, ms["inflate"], locator, ms["bam_hops"], ms["bam_chain"],
                 ms["bam_starts"], ms["bam_reads_size"], ms["bam_reads_unpack"], moved / ms["bam_reads_unpack"] / 1e6, moved / 1e9,
                 copy_ms, ms["bam_reads_unpack"] / ms["inflate"], ms["bam_reads_unpack"] / copy_ms,
                 ms["bam_reads_size"] / ms["inflate"], dt * 1e3, nbytes / dt / 1e9), flush=True)


def route_w(paths, nreads, nbytes, ntext):
    from sarlacc_amd.resident import DeviceReads
    for rep in range(3):
        made = {}
        for path, what, size, make in ((paths[0], "from_bam", nbytes, DeviceReads.from_bam), (paths[1], "from_fastq", ntext, DeviceReads.from_fastq)):
            t0 = time.perf_counter()
            dev = make(path)
            dt = time.perf_counter() - t0
            print("w rep %d: DeviceReads.%s: %.1f ms, %d reads | %.2f GB/s of inflated bytes, %.2f M reads/s"
                  % (rep, what, dt * 1e3, len(dev), size / dt / 1e9, len(dev) / dt / 1e6), flush=True)
            made[what] = dev
        a, b = made["from_bam"], made["from_fastq"]
        assert len(a) == len(b) == nreads and np.array_equal(a.off_host, b.off_host)
        if rep == 0:
            for x, y in zip(a.download(), b.download()):
                assert np.array_equal(x.chars[:x.total], y.chars[:y.total])
            assert np.array_equal(a.names.ss.off, b.names.ss.off) and np.array_equal(a.names.ss.chars, b.names.ss.chars)
            print("w: the two batches are equal (%d reads, %d bases)" % (len(a), a.total), flush=True)
        del made, a, b, dev


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pool", type=int, default=4096, help="distinct records")
    ap.add_argument("--gb", type=float, default=1.0, help="BAM bytes, inflated")
    ap.add_argument("--length", type=int, default=P.L, help="bases per read (the pool's reads all have this length)")
    ap.add_argument("--block-mb", type=int, default=256)
    ap.add_argument("--limit", type=int, default=300, help="seconds per route")
    ap.add_argument("--route", choices=["k", "w"], help="run one route in this process")
    ap.add_argument("--folder", help="(child process) where the files are")
    ap.add_argument("--sizes", help="(child process) records, reads, BAM bytes, FASTQ text bytes")
    args = ap.parse_args()
    if args.route is None:
        with tempfile.TemporaryDirectory() as folder:
            t0 = time.perf_counter()
            # the files are written by a child too: this process never opens the device
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--route", "k", "--folder", folder, "--sizes", "prepare",
                                 "--pool", str(args.pool), "--gb", str(args.gb), "--length", str(args.length)], timeout=args.limit, stdout=subprocess.PIPE)
            if rc.returncode:
                sys.exit("writing the files failed with status %d" % rc.returncode)
            lines = rc.stdout.decode().splitlines()
            sizes = lines[-1]
            print("\n".join(lines[:-1]), flush=True)
            print("files written in %.0f s" % (time.perf_counter() - t0), flush=True)
            for route in "kw":     # a fresh process per route, each under its own limit; nothing runs after a failure
                rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--route", route, "--folder", folder, "--sizes", sizes,
                                     "--block-mb", str(args.block_mb)], timeout=args.limit).returncode
                if rc:
                    sys.exit("route %s failed with status %d" % (route, rc))
        return
    if args.sizes == "prepare":
        import platform
        import torch
        P.L = args.length
        print("box %s, %s" % (platform.node(), torch.cuda.get_device_name(0)), flush=True)
        paths, nrec, nreads, nbytes, ntext = prepare(args.pool, args.gb, args.folder)
        print("%d records of %d-base reads, %d of them reads: %.3f GB of BAM (%.3f GB as BGZF), %.3f GB of FASTQ text (%.3f GB as BGZF), "
              "zlib level 6, %d-byte blocks" % (nrec, P.L, nreads, nbytes / 1e9, os.path.getsize(paths[0]) / 1e9, ntext / 1e9,
                                                os.path.getsize(paths[1]) / 1e9, P.BLOCK), flush=True)
        print("%d,%d,%d,%d" % (nrec, nreads, nbytes, ntext), flush=True)
        return
    nrec, nreads, nbytes, ntext = (int(x) for x in args.sizes.split(","))
    paths = [os.path.join(args.folder, "x.bam"), os.path.join(args.folder, "x.fastq.gz")]
    if args.route == "k":
        route_k(paths[0], nrec, nreads, nbytes, args.block_mb << 20)
    else:
        route_w(paths, nreads, nbytes, ntext)


if __name__ == "__main__":
    main()
