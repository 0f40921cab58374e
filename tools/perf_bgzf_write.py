"""Output of BGZF-compressed FASTQ: the device deflate route against compressing on the host.

The synthetic FASTQ of tools/perf_bgzf_ingest.py (uniform ACGT bases; qualities from error probabilities ~ U(0, 0.06)
as Phred+33; 4 000-base reads), about 64 MB repeated to about 1 GB of text in device memory.  Four routes, each in a
child process of its own under its own time limit:

  k  the encode kernel alone (HIP events around k_bgzf_deflate) and the whole sarlacc_dev_bgzf_deflate call, per mode,
     with the compression ratio of every mode
  w  DeviceReads.to_fastq to /dev/shm, plain and compressed
  h  the host route a user has today: the text downloaded, then zlib level 1 and level 6 on 16 threads into BGZF blocks
     (the time of the download is reported apart)
  r  ratios on the text of the size tests (tests/bgzf_write_cases.py: 8 blocks of 2 000- and 100-base reads) against
     zlib level 6, Z_HUFFMAN_ONLY and Z_HUFFMAN_ONLY with a deflate block per line

    python tools/perf_bgzf_write.py [--mb 64] [--repeat 16] [--limit 300] [--out profiles/bgzf_write.txt]
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


def say(out, line):
    print(line, flush=True)
    with open(out, "a") as fh:
        fh.write(line + "\n")


def device_text(mb, repeat):
    from sarlacc_amd.resident import DevBuffer
    text, nrec = synth(mb << 20, 4000, np.random.default_rng(1000))
    whole = np.tile(text, repeat)
    return DevBuffer.from_numpy(whole), whole.size, nrec * repeat, text


def zlib_block(level):
    def work(data):
        c = zlib.compressobj(level, zlib.DEFLATED, -15, 9)
        raw = c.compress(data) + c.flush()
        return len(raw) + 26
    return work


def route_k(args):
    import sarlacc_amd
    from sarlacc_amd import bgzf
    d_text, total, _, text = device_text(args.mb, args.repeat)
    d_comp = None
    for mode in (0, 1, 2):
        for rep in range(3):
            t0 = time.perf_counter()
            d_comp, nbytes = bgzf.deflate_device(d_text, total, mode, out=d_comp)
            dt = time.perf_counter() - t0
            ms = sarlacc_amd.last_kernel_ms()
            say(args.out, "k mode %d rep %d: k_bgzf_deflate %.2f ms by HIP events | %.2f GB/s text | whole call %.2f ms | %.3f GB -> "
                "%.3f GB, ratio %.4f" % (mode, rep, ms, total / ms / 1e6, dt * 1e3, total / 1e9, nbytes / 1e9, nbytes / total))
        if mode == 0:
            head = d_comp.to_numpy(np.uint8, nbytes)[:40 << 20].tobytes()
            n, used, _, text_off, _ = bgzf.scan(head)
            back = gzip.decompress(head[:used])
            assert back == np.tile(text, 2)[:len(back)].tobytes() and len(back) == text_off[-1] > 0, "the blocks do not decode to the text"
    raw = text.tobytes()
    with ThreadPoolExecutor(THREADS) as pool:
        for level in (1, 6):
            size = sum(pool.map(zlib_block(level), [raw[i:i + BLOCK] for i in range(0, len(raw), BLOCK)]))
            say(args.out, "k zlib level %d on the same blocks: ratio %.4f" % (level, size / len(raw)))


def route_w(args):
    from sarlacc_amd.resident import DeviceReads
    d_text, total, nrec, _ = device_text(args.mb, args.repeat)
    reads = DeviceReads._from_device_text(d_text, total, None)
    assert len(reads) == nrec
    del d_text
    path = os.path.join(SHM, "perf_bgzf_write.%d" % os.getpid())
    try:
        for compress in (False, True, False, True):
            t0 = time.perf_counter()
            written = reads.to_fastq(path, compress=compress)
            dt = time.perf_counter() - t0
            say(args.out, "w to_fastq(compress=%s): %.1f ms | %.3f GB of text -> %.3f GB written | %.2f GB/s text"
                % (compress, dt * 1e3, total / 1e9, written / 1e9, total / dt / 1e9))
    finally:
        if os.path.exists(path):
            os.remove(path)


def route_h(args):
    d_text, total, _, _ = device_text(args.mb, args.repeat)
    t0 = time.perf_counter()
    host = d_text.to_numpy(np.uint8, total)
    download = time.perf_counter() - t0
    say(args.out, "h download of %.3f GB of text: %.1f ms" % (total / 1e9, download * 1e3))
    view = memoryview(host)
    spans = [(i, min(i + BLOCK, total)) for i in range(0, total, BLOCK)]
    for level in (1, 6):
        work = zlib_block(level)
        t0 = time.perf_counter()
        with ThreadPoolExecutor(THREADS) as pool:
            size = sum(pool.map(lambda s: work(view[s[0]:s[1]]), spans, chunksize=64))
        dt = time.perf_counter() - t0
        say(args.out, "h zlib level %d on %d threads: %.1f ms | %.2f GB/s text | ratio %.4f | with the download %.1f ms"
            % (level, THREADS, dt * 1e3, total / dt / 1e9, size / total, (dt + download) * 1e3))


def route_r(args):
    from sarlacc_amd import bgzf
    from sarlacc_amd.resident import DevBuffer
    from tests import bgzf_write_cases as W
    for L in (2000, 100):
        text, y = W.seeded_text(L), W.yardsticks(L)
        d_text = DevBuffer.from_numpy(np.frombuffer(text, np.uint8))
        for mode in (0, 1):
            buf, nbytes = bgzf.deflate_device(d_text, len(text), mode)
            assert gzip.decompress(buf.to_numpy(np.uint8, nbytes).tobytes()) == text
            say(args.out, "r %d-base reads, mode %d: %d bytes, ratio %.4f | to zlib level 6 %.4f, to Z_HUFFMAN_ONLY %.4f, to "
                "Z_HUFFMAN_ONLY per line %.4f" % (L, mode, nbytes, nbytes / len(text), nbytes / y["level6"], nbytes / y["huffman"],
                                                  nbytes / y["per_line"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=64)
    ap.add_argument("--repeat", type=int, default=16)
    ap.add_argument("--limit", type=int, default=300, help="seconds per route")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bgzf_write.txt"))
    ap.add_argument("--route", choices=["k", "w", "h", "r"], help="run one route in this process")
    args = ap.parse_args()
    if args.route is None:
        open(args.out, "w").close()
        say(args.out, "tools/perf_bgzf_write.py --mb %d --repeat %d: %d-byte blocks, %d host threads" % (args.mb, args.repeat, BLOCK, THREADS))
        for route in "rkwh":     # a fresh process per route, each under its own limit; nothing runs after a failure
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--mb", str(args.mb), "--repeat", str(args.repeat),
                                 "--out", args.out, "--route", route], timeout=args.limit).returncode
            if rc:
                sys.exit("route %s failed with status %d" % (route, rc))
        return
    {"k": route_k, "w": route_w, "h": route_h, "r": route_r}[args.route](args)


if __name__ == "__main__":
    main()
