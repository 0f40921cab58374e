"""Throughput of the device FASTQ writer: n synthetic resident reads of about L bases (sarlacc_amd.devsynth, generated in
HBM) with 35-byte names, back to 4-line FASTQ text.  One JSON line:
  (a) kernel time of the size pass and of the format pass (HIP events inside the two C-ABI calls) and the algorithmic
      rate of the format pass: the text is written once; seq, qual and names are read once;
  (b) a plain device-to-device copy of as many bytes as the text has, in the same process: the yardstick for (a);
  (c) wall time of DeviceReads.to_fastq to a file in /dev/shm (or the temporary directory);
  (d) wall time of the route without the device writer on the same reads: download() + Reads + the host loop of
      generics.write_fastq.  The two files are compared byte for byte.
Usage: perf_fastq_write.py [n_reads] [read_len]"""
import ctypes as C
import filecmp
import json
import os
import statistics
import sys
import tempfile
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from sarlacc_amd import _lib, generics
from sarlacc_amd._lib import check
from sarlacc_amd.devsynth import make_reads
from sarlacc_amd.resident import DevBuffer, DeviceReads
from sarlacc_amd.strset import StringSet, StrList

A1 = "ACGATCAGC" + "N" * 12 + "GTCAGTCAG"
A2 = "CACACTGAGCAGCGACTAGACA"
WARMUP, REPS = 2, 7


def synth_names(n):
    name = np.frombuffer(b"read_0000000 ch=12 start_time=1234", dtype=np.uint8)
    mat = np.tile(name, (n, 1))
    idx = np.arange(n)
    for d in range(7):  # decimal read number
        mat[:, 5 + 6 - d] = 48 + (idx // 10 ** d) % 10
    return StrList(StringSet.from_matrix(mat))


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 250000
    L = int(sys.argv[2]) if len(sys.argv) > 2 else 2000
    device = torch.device("cuda:0")
    seq, qual, off, _ = make_reads(n, L, A1, A2, 1000, device)
    torch.cuda.synchronize()
    h_off = off.cpu().numpy()
    bases = int(h_off[-1])
    dev = DeviceReads(DevBuffer.borrow(seq.data_ptr(), bases), DevBuffer.borrow(qual.data_ptr(), bases),
                      DevBuffer.borrow(off.data_ptr(), 8 * (n + 1)), h_off, None)
    dev.names = synth_names(n)
    lib = _lib.lib()

    # (a) the two passes over the whole batch, timed by the library's HIP events
    ss = dev.names.ss
    d_names, d_noff, rec_off = DevBuffer.from_numpy(ss.chars), DevBuffer.from_numpy(ss.off), DevBuffer(8 * (n + 1))
    total = C.c_int64(0)
    check(lib.sarlacc_dev_fastq_format_size(dev.off.ptr, C.c_int64(n), d_names.ptr, d_noff.ptr, C.c_int64(1), rec_off.ptr,
                                            C.byref(total), None))
    text_bytes = total.value
    d_text = DevBuffer(text_bytes)
    size_ms, format_ms = [], []
    for rep in range(WARMUP + REPS):
        check(lib.sarlacc_dev_fastq_format_size(dev.off.ptr, C.c_int64(n), d_names.ptr, d_noff.ptr, C.c_int64(1), rec_off.ptr,
                                                C.byref(total), None))
        s_ms = _lib.stage_ms("fastq_size")
        check(lib.sarlacc_dev_fastq_format(dev.seq.ptr, dev.qual.ptr, dev.off.ptr, d_names.ptr, d_noff.ptr, C.c_int64(1),
                                           rec_off.ptr, C.c_int64(0), C.c_int64(n), d_text.ptr, None))
        f_ms = _lib.stage_ms("fastq_format")
        if rep >= WARMUP:
            size_ms.append(s_ms)
            format_ms.append(f_ms)
    algorithmic = text_bytes + 2 * bases + ss.total   # written once + read once
    del d_text

    # (b) device-to-device copy of text_bytes bytes
    src, dst = torch.empty(text_bytes, dtype=torch.uint8, device=device), torch.empty(text_bytes, dtype=torch.uint8, device=device)
    src.fill_(65)
    copy_ms = []
    for rep in range(WARMUP + REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(src)
        e1.record()
        torch.cuda.synchronize()
        if rep >= WARMUP:
            copy_ms.append(e0.elapsed_time(e1))
    del src, dst
    torch.cuda.empty_cache()

    # (c) the whole call, to a file in memory; (d) the host route on the same reads
    where = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else tempfile.gettempdir()
    with tempfile.TemporaryDirectory(dir=where) as tmp:
        p_dev, p_host = os.path.join(tmp, "dev.fastq"), os.path.join(tmp, "host.fastq")
        dev_s = []
        for rep in range(1 + 3):
            t0 = time.perf_counter()
            written = dev.to_fastq(p_dev)
            if rep >= 1:
                dev_s.append(time.perf_counter() - t0)
        assert written == text_bytes == os.path.getsize(p_dev)
        host_s = []
        for rep in range(1 + 2):
            t0 = time.perf_counter()
            s, q = dev.download()
            generics.write_fastq(p_host, generics.Reads(s, q, dev.names))
            if rep >= 1:
                host_s.append(time.perf_counter() - t0)
            del s, q
        same = filecmp.cmp(p_dev, p_host, shallow=False)
    fmt = statistics.median(format_ms)
    cp = statistics.median(copy_ms)
    print(json.dumps({
        "tool": "perf_fastq_write", "reads": n, "read_len": L, "bases": bases, "name_bytes": ss.total, "text_bytes": text_bytes,
        "a_size_pass": spread(size_ms), "a_format_pass": spread(format_ms),
        "a_format_algorithmic_bytes": algorithmic, "a_format_algorithmic_GBps": round(algorithmic / fmt / 1e6, 1),
        "a_format_text_GBps": round(text_bytes / fmt / 1e6, 1),
        "b_d2d_copy": spread(copy_ms), "b_d2d_traffic_GBps": round(2 * text_bytes / cp / 1e6, 1),
        "format_over_copy_time": round(fmt / cp, 3),
        "c_to_fastq_wall_s": [round(x, 3) for x in dev_s], "d_host_route_wall_s": [round(x, 3) for x in host_s],
        "host_over_device_wall_min_over_min": round(min(host_s) / min(dev_s), 1), "files_identical": bool(same), "file_dir": where,
        "repeats": {"kernels_and_copy": {"warmup": WARMUP, "timed": REPS}, "c": {"warmup": 1, "timed": 3},
                    "d": {"warmup": 1, "timed": 2}}}))
    assert same, "device and host writers disagree"


if __name__ == "__main__":
    main()
