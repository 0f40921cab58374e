"""Ingest of BGZF-compressed FASTQ: the device inflate route against inflating on the host.

About 64 MB of synthetic FASTQ (uniform ACGT bases; qualities from error probabilities ~ U(0, 0.06) as Phred+33, the
statistics of sarlacc_amd.devsynth -- qualities compress poorly, which is what real files are like) is compressed once
into BGZF blocks with zlib level 6, and the blocks are repeated to about 1 GB of text (blocks are independent, so the
repeated file is valid BGZF).  Three routes, each in a child process of its own under its own time limit:

  a  host route: the same blocks inflated by zlib on 16 threads into page-locked memory, the text uploaded, then
     DeviceReads._from_device_text -- what a caller had to do before, and the yardstick
  b  device route end to end: host block scan, upload of the compressed bytes, sarlacc_dev_bgzf_inflate with the CRC
     check, DeviceReads._from_device_text
  c  the inflate kernel alone (HIP events around k_bgzf_inflate), and the whole inflate call with and without the CRC pass

    python tools/perf_bgzf_ingest.py [--mb 64] [--repeat 16] [--limit 300]
"""
import argparse
import os
import subprocess
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

THREADS = 16
BLOCK = 0xff00


def synth(nbytes, L, rng):
    name = np.frombuffer(b"@read_0000000 ch=12 start_time=1234\n", dtype=np.uint8)
    n = max(nbytes // (name.size + 2 * L + 4), 1)
    rec = np.empty((n, name.size + L + 1 + 2 + L + 1), np.uint8)
    rec[:, :name.size] = name
    idx = np.arange(n)
    for d in range(7):
        rec[:, 6 + 6 - d] = 48 + (idx // 10 ** d) % 10
    o = name.size
    rec[:, o:o + L] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, (n, L))]
    rec[:, o + L] = 10
    rec[:, o + L + 1] = ord("+")
    rec[:, o + L + 2] = 10
    err = np.maximum(rng.random((n, L)) * 0.06, 1e-9)
    rec[:, o + L + 3:o + 2 * L + 3] = (33 + np.clip(np.rint(-10 * np.log10(err)), 0, 60)).astype(np.uint8)
    rec[:, -1] = 10
    return rec.reshape(-1), n


def bgzf_block(data):
    c = zlib.compressobj(6, zlib.DEFLATED, -15, 9)
    raw = c.compress(data) + c.flush()
    head = b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + (len(raw) + 25).to_bytes(2, "little")
    return head + raw + zlib.crc32(data).to_bytes(4, "little") + len(data).to_bytes(4, "little")


def prepare(mb, repeat):
    text, nrec = synth(mb << 20, 4000, np.random.default_rng(1000))
    raw = text.tobytes()
    with ThreadPoolExecutor(THREADS) as pool:
        blocks = list(pool.map(bgzf_block, [raw[i:i + BLOCK] for i in range(0, len(raw), BLOCK)]))
    comp = np.tile(np.frombuffer(b"".join(blocks), np.uint8), repeat)
    return comp, text.size * repeat, nrec * repeat, text


def offsets(comp):
    from sarlacc_amd import bgzf
    n, used, comp_off, text_off, _ = bgzf.scan(comp)
    assert used == comp.size
    return n, comp_off, text_off


def parse(d_text, nbytes):
    from sarlacc_amd.resident import DeviceReads
    return DeviceReads._from_device_text(d_text, nbytes, None)


def route_a(comp, total, nrec):
    from sarlacc_amd import _lib
    from sarlacc_amd.resident import DevBuffer
    n, comp_off, text_off = offsets(comp)
    host = _lib.host_array(total, np.uint8)
    view = memoryview(comp)

    def work(span):
        for k in range(*span):
            t = zlib.decompress(view[comp_off[k] + 18:comp_off[k + 1] - 8], -15)
            host[text_off[k]:text_off[k + 1]] = np.frombuffer(t, np.uint8)
    step = -(-n // (THREADS * 8))
    for rep in range(2):
        t0 = time.perf_counter()
        with ThreadPoolExecutor(THREADS) as pool:
            list(pool.map(work, [(a, min(a + step, n)) for a in range(0, n, step)]))
        t1 = time.perf_counter()
        d_text = DevBuffer(total)
        _lib.check(_lib.lib().sarlacc_dev_upload(d_text, host, total))
        t2 = time.perf_counter()
        reads = parse(d_text, total)
        t3 = time.perf_counter()
        assert len(reads) == nrec
        print("a rep %d: host inflate on %d threads %.1f ms (%.2f GB/s text) + upload %.1f ms + parse %.1f ms = %.1f ms | "
              "%.2f GB/s text, %.2f GB/s compressed" % (rep, THREADS, (t1 - t0) * 1e3, total / (t1 - t0) / 1e9, (t2 - t1) * 1e3,
                                                        (t3 - t2) * 1e3, (t3 - t0) * 1e3, total / (t3 - t0) / 1e9,
                                                        comp.size / (t3 - t0) / 1e9), flush=True)
        del reads, d_text


def route_b(comp, total, nrec):
    from sarlacc_amd import _lib
    from sarlacc_amd.resident import DevBuffer
    lib = _lib.lib()
    for rep in range(3):
        t0 = time.perf_counter()
        n, comp_off, text_off = offsets(comp)
        t1 = time.perf_counter()
        d_comp, d_co, d_to = DevBuffer.from_numpy(comp), DevBuffer.from_numpy(comp_off), DevBuffer.from_numpy(text_off)
        d_text = DevBuffer(total)
        t2 = time.perf_counter()
        _lib.check(lib.sarlacc_dev_bgzf_inflate(d_comp, d_co, d_to, n, 0, d_text, 1, None))
        t3 = time.perf_counter()
        reads = parse(d_text, total)
        t4 = time.perf_counter()
        assert len(reads) == nrec
        print("b rep %d: scan %.1f ms + upload of %.2f GB compressed %.1f ms + inflate with CRC %.1f ms + parse %.1f ms = %.1f ms | "
              "%.2f GB/s text, %.2f GB/s compressed" % (rep, (t1 - t0) * 1e3, comp.size / 1e9, (t2 - t1) * 1e3, (t3 - t2) * 1e3,
                                                        (t4 - t3) * 1e3, (t4 - t0) * 1e3, total / (t4 - t0) / 1e9,
                                                        comp.size / (t4 - t0) / 1e9), flush=True)
        del reads, d_text, d_comp


def route_c(comp, total, nrec, text):
    import sarlacc_amd
    from sarlacc_amd import _lib
    from sarlacc_amd.resident import DevBuffer
    lib = _lib.lib()
    n, comp_off, text_off = offsets(comp)
    d_comp, d_co, d_to = DevBuffer.from_numpy(comp), DevBuffer.from_numpy(comp_off), DevBuffer.from_numpy(text_off)
    d_text = DevBuffer(total)
    for rep in range(4):
        crc = rep % 2
        t0 = time.perf_counter()
        _lib.check(lib.sarlacc_dev_bgzf_inflate(d_comp, d_co, d_to, n, 0, d_text, crc, None))
        dt = time.perf_counter() - t0
        ms = sarlacc_amd.last_kernel_ms()
        print("c rep %d: k_bgzf_inflate %.2f ms by HIP events | %.2f GB/s text, %.2f GB/s compressed | whole call %s CRC %.2f ms "
              "(%d blocks)" % (rep, ms, total / ms / 1e6, comp.size / ms / 1e6, "with" if crc else "without", dt * 1e3, n), flush=True)
    assert d_text.to_numpy(np.uint8, text.size).tobytes() == text.tobytes(), "the inflated text differs from the input"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=64)
    ap.add_argument("--repeat", type=int, default=16)
    ap.add_argument("--limit", type=int, default=300, help="seconds per route")
    ap.add_argument("--route", choices=["a", "b", "c"], help="run one route in this process")
    args = ap.parse_args()
    if args.route is None:
        for route in "abc":     # a fresh process per route, each under its own limit; nothing runs after a failure
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--mb", str(args.mb), "--repeat", str(args.repeat),
                                 "--route", route], timeout=args.limit).returncode
            if rc:
                sys.exit("route %s failed with status %d" % (route, rc))
        return
    comp, total, nrec, text = prepare(args.mb, args.repeat)
    if args.route == "a":
        print("%d records, %.3f GB of FASTQ text, %.3f GB as BGZF (zlib level 6, ratio %.2f), %d-byte blocks"
              % (nrec, total / 1e9, comp.size / 1e9, total / comp.size, BLOCK), flush=True)
        route_a(comp, total, nrec)
    elif args.route == "b":
        route_b(comp, total, nrec)
    else:
        route_c(comp, total, nrec, text)


if __name__ == "__main__":
    main()
