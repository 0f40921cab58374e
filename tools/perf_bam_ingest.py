"""sam2ranges on a BAM file: the record locator and the field kernel of bam.hip by HIP events, and the whole call
against the same records as BGZF-compressed SAM text (the text path, which this work does not touch).

A pool of seeded ONT-like records (2-kb reads, 36-character names, about one CIGAR op per 6 bases, qualities from error
probabilities ~ U(0, 0.06) -- they compress poorly, which is what real files are like -- and three tags) is written
once as BAM records and once as SAM lines; each form is compressed into BGZF blocks with zlib level 6 and the blocks
are repeated to about 1 GB of BAM bytes (blocks are independent, and the pool is whole records, so the repeated file
is valid).  Two routes, each in a child process of its own under its own time limit:

  k  the loop of sarlacc_amd.sam._bam_parts driven by hand, so that every sarlacc_dev_bam_index call's stage timers
     can be read: k_bgzf_inflate, k_bam_hops, k_bam_chain, k_bam_starts (both passes and the scan between them),
     k_bam_fields, k_sam_scatter, summed over the buffers of the file
  w  the whole generics.sam2ranges call on the BAM file and on the BGZF SAM file, alternating, host clock (the call
     ends with the columns on the host); the two tables must be equal

    python tools/perf_bam_ingest.py [--pool 4096] [--gb 1.0] [--limit 300]
"""
import argparse
import ctypes as C
import os
import struct
import subprocess
import sys
import tempfile
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

THREADS = 16
BLOCK = 0xff00
L = 2000
REFS = ["chr%d" % i for i in range(1, 23)]
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
OPS = "MIDNSHP=X"


def pool_records(n, rng):
    """n records as (BAM bytes, SAM lines)."""
    bam, sam = [], []
    flags = rng.choice([0, 16, 4, 256, 2048, 272], n, p=[0.4, 0.35, 0.1, 0.05, 0.05, 0.05])
    for i in range(n):
        flag = int(flags[i])
        name = "%08x-%04x-%04x-%04x-%012x" % (i, i % 65536, 7, 9, i)
        nops = int(rng.integers(L // 6 - 30, L // 6 + 30))
        ops = rng.choice([0, 0, 0, 0, 1, 2, 7, 8], nops)
        lens = rng.integers(1, 12, nops)
        if rng.random() < 0.5:
            ops[0], lens[0] = 4, int(rng.integers(1, 200))
        if rng.random() < 0.5:
            ops[-1], lens[-1] = 4, int(rng.integers(1, 200))
        if flag & 4:
            ops, lens = ops[:0], lens[:0]
        refid = -1 if flag & 4 else i % 22
        pos = (i * 7919) % 10 ** 7
        mapq = int(rng.integers(0, 61))
        bases = rng.integers(0, 4, L)
        err = np.maximum(rng.random(L) * 0.06, 1e-9)
        qual = np.clip(np.rint(-10 * np.log10(err)), 0, 60).astype(np.uint8)
        nib = np.array([1, 2, 4, 8], np.uint8)[bases]
        tags = b"NMC" + bytes([i % 50]) + b"msI" + struct.pack("<I", i) + b"tpAP"
        body = struct.pack("<iiBBHHHiiii", refid, pos, len(name) + 1, mapq, 0, len(ops), flag, L, -1, -1, 0) + name.encode() + b"\0" + \
            ((lens.astype("<u4") << 4) | ops.astype("<u4")).tobytes() + ((nib[0::2] << 4) | nib[1::2]).tobytes() + qual.tobytes() + tags
        bam.append(struct.pack("<i", len(body)) + body)
        sam.append("%s\t%d\t%s\t%d\t%d\t%s\t*\t0\t0\t%s\t%s\tNM:i:%d\tms:i:%d\ttp:A:P\n"
                   % (name, flag, "*" if flag & 4 else REFS[refid], pos + 1, mapq,
                      "".join("%d%s" % (a, OPS[b]) for a, b in zip(lens, ops)) or "*",
                      np.frombuffer(b"ACGT", np.uint8)[bases].tobytes().decode(), (qual + 33).tobytes().decode(), i % 50, i))
    return b"".join(bam), "".join(sam).encode()


def bgzf_block(data):
    c = zlib.compressobj(6, zlib.DEFLATED, -15, 9)
    raw = c.compress(data) + c.flush()
    head = b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + (len(raw) + 25).to_bytes(2, "little")
    return head + raw + zlib.crc32(data).to_bytes(4, "little") + len(data).to_bytes(4, "little")


def bgzf(data):
    with ThreadPoolExecutor(THREADS) as pool:
        return b"".join(pool.map(bgzf_block, [data[i:i + BLOCK] for i in range(0, len(data), BLOCK)]))


def prepare(pool, gb, folder):
    """Writes x.bam and x.sam.gz; returns (paths, records, BAM bytes, SAM text bytes)."""
    bam, sam = pool_records(pool, np.random.default_rng(1000))
    repeat = max(int(gb * 1e9 / len(bam)), 1)
    text = "".join(["@HD\tVN:1.6\tSO:unsorted\n"] + ["@SQ\tSN:%s\tLN:%d\n" % (r, 10 ** 8) for r in REFS]).encode()
    head = b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(REFS)) + \
        b"".join(struct.pack("<i", len(r) + 1) + r.encode() + b"\0" + struct.pack("<i", 10 ** 8) for r in REFS)
    paths = []
    for name, first, body in (("x.bam", head, bam), ("x.sam.gz", text, sam)):
        blocks = bgzf(body)
        paths.append(os.path.join(folder, name))
        with open(paths[-1], "wb") as fh:
            fh.write(bgzf_block(first))
            for _ in range(repeat):
                fh.write(blocks)
            fh.write(EOF_BLOCK)
    return paths, pool * repeat, len(bam) * repeat, len(sam) * repeat


def route_k(path, nrec, nbytes, block_bytes):
    import sarlacc_amd
    from sarlacc_amd import _lib, bgzf as bg, sam
    lib = _lib.lib()
    stages = ["bam_hops", "bam_chain", "bam_starts", "bam_fields", "sam_scatter"]
    for rep in range(3):
        ms = dict.fromkeys(["inflate"] + stages, 0.0)
        t0 = time.perf_counter()
        with open(path, "rb") as fh:
            names, _, origin = sam.read_bam_header(fh)
            fh.seek(origin[0])
            stream = bg.DeviceTextStream(fh, block_bytes, first_block=origin[1], skip=origin[2])
            record, carry, eof, kept, buffers = 1, None, False, 0, 0
            host = [time.perf_counter() - t0, 0.0, 0.0, 0.0]     # header, stream.next, index, extract: each ends synchronised
            while not eof:
                t1 = time.perf_counter()
                d_bam, n, eof = stream.next(carry)
                t2 = time.perf_counter()
                host[1] += t2 - t1
                if d_bam is None or n == 0:
                    break
                ms["inflate"] += sarlacc_amd.last_kernel_ms()
                nr, used, nk, nb = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)
                _lib.check(lib.sarlacc_dev_bam_index(d_bam, n, record, 1 if eof else 0, len(names) - 1, None, 1, 10, C.byref(nr),
                                                     C.byref(used), C.byref(nk), C.byref(nb), None))
                t3 = time.perf_counter()
                sam._columns(lib.sarlacc_dev_bam_extract, d_bam, nk.value, nb.value)
                host[2] += t3 - t2
                host[3] += time.perf_counter() - t3
                for s in stages:
                    ms[s] += max(sarlacc_amd.stage_ms(s), 0.0)
                record += nr.value
                kept += nk.value
                buffers += 1
                carry = (d_bam, used.value, n - used.value) if used.value < n else None
        dt = time.perf_counter() - t0
        assert record - 1 == nrec, (record, nrec)
        print("k rep %d: %d records (%d kept) in %d buffers of %d MB | by HIP events, summed over the buffers: k_bgzf_inflate %.2f ms, "
              "k_bam_hops %.2f ms, k_bam_chain %.2f ms, k_bam_starts (two passes, the scan and the host's look between them) %.2f ms, k_bam_fields %.2f ms, "
              "k_sam_scatter %.2f ms | chain / inflate = %.3f, locator / inflate = %.3f | the loop with its downloads %.1f ms "
              "(%.2f GB/s of BAM bytes), by the host clock: header %.1f ms, the buffers (file read, block scan, upload, inflate "
              "with CRC, carry) %.1f ms, the index calls %.1f ms, the extract calls with their downloads %.1f ms"
              % (rep, nrec, kept, buffers, block_bytes >> 20, ms["inflate"], ms["bam_hops"], ms["bam_chain"], ms["bam_starts"],
                 ms["bam_fields"], ms["sam_scatter"], ms["bam_chain"] / ms["inflate"],
                 (ms["bam_hops"] + ms["bam_chain"] + ms["bam_starts"]) / ms["inflate"], dt * 1e3, nbytes / dt / 1e9,
                 *[h * 1e3 for h in host]), flush=True)


def route_w(paths, nrec, nbytes, ntext):
    from sarlacc_amd import generics
    tables = {}
    for rep in range(3):
        for path, what, size in ((paths[0], "BAM", nbytes), (paths[1], "BGZF SAM", ntext)):
            t0 = time.perf_counter()
            res = generics.sam2ranges(path, minq=10)
            dt = time.perf_counter() - t0
            print("w rep %d: generics.sam2ranges on the %s file: %.1f ms, %d of %d records kept | %.2f GB/s of inflated bytes, "
                  "%.2f M records/s" % (rep, what, dt * 1e3, len(res["start"]), nrec, size / dt / 1e9, nrec / dt / 1e6), flush=True)
            tables[what] = res
    a, b = tables["BAM"], tables["BGZF SAM"]
    for k in ("seqnames", "start", "end", "width", "left.clip", "right.clip", "strand"):
        assert np.array_equal(a[k], b[k]), k
    assert list(a["names"][:1000]) == list(b["names"][:1000]) and a["seqinfo"]["seqnames"] == b["seqinfo"]["seqnames"]
    print("w: the BAM and the BGZF SAM tables are equal (%d rows)" % len(a["start"]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pool", type=int, default=4096, help="distinct records")
    ap.add_argument("--gb", type=float, default=1.0, help="BAM bytes, inflated")
    ap.add_argument("--block-mb", type=int, default=256)
    ap.add_argument("--limit", type=int, default=300, help="seconds per route")
    ap.add_argument("--route", choices=["k", "w"], help="run one route in this process")
    ap.add_argument("--folder", help="(child process) where the files are")
    ap.add_argument("--sizes", help="(child process) records, BAM bytes, SAM text bytes")
    args = ap.parse_args()
    if args.route is None:
        with tempfile.TemporaryDirectory() as folder:
            t0 = time.perf_counter()
            import platform
            import torch
            print("box %s, %s" % (platform.node(), torch.cuda.get_device_name(0)), flush=True)
            paths, nrec, nbytes, ntext = prepare(args.pool, args.gb, folder)
            print("%d records of %d-base reads: %.3f GB of BAM (%.3f GB as BGZF), %.3f GB of SAM text (%.3f GB as BGZF), zlib level 6, "
                  "%d-byte blocks, written in %.0f s" % (nrec, L, nbytes / 1e9, os.path.getsize(paths[0]) / 1e9, ntext / 1e9,
                                                         os.path.getsize(paths[1]) / 1e9, BLOCK, time.perf_counter() - t0), flush=True)
            for route in "kw":     # a fresh process per route, each under its own limit; nothing runs after a failure
                rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--route", route, "--folder", folder, "--sizes",
                                     "%d,%d,%d" % (nrec, nbytes, ntext), "--block-mb", str(args.block_mb)],
                                    timeout=args.limit).returncode
                if rc:
                    sys.exit("route %s failed with status %d" % (route, rc))
        return
    nrec, nbytes, ntext = (int(x) for x in args.sizes.split(","))
    paths = [os.path.join(args.folder, "x.bam"), os.path.join(args.folder, "x.sam.gz")]
    if args.route == "k":
        route_k(paths[0], nrec, nbytes, args.block_mb << 20)
    else:
        route_w(paths, nrec, nbytes, ntext)


if __name__ == "__main__":
    main()
