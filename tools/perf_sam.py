"""Throughput of the device SAM parser (sam2ranges, sam.hip) on a seeded ONT-like file: n records of L-base reads,
36-character QNAMEs, CIGARs of about one op per 6 bases, SEQ, QUAL and a few tags.  The body text is uploaded once,
then index + extract are timed (wall clock around the two C-ABI calls, which synchronise; one warm-up, best and median
of the repetitions).  Algorithmic bytes: the text read twice by the line passes, the bytes of every line up to the end
of its CIGAR read once by the field pass, the columns, names and offsets written once.  Also: the whole
generics.sam2ranges call on a file of up to `--generics` records that is in the page cache, and the restatement of
R/sam2ranges.R (tests/sam_restated.py) on 10^4 records as the CPU baseline.  Prints one JSON line.

usage: python tools/perf_sam.py n L [--reps R] [--generics M]"""
import argparse
import ctypes as C
import io
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from sarlacc_amd import _lib, generics, sam
from sarlacc_amd._lib import check, ptr
from sarlacc_amd.resident import DevBuffer

REFS = ["chr%02d" % i for i in range(1, 23)]
HBM_PEAK = 8.0e12


def header():
    return ("@HD\tVN:1.6\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % (r, 250000000 - 7 * i) for i, r in enumerate(REFS))
            + "@PG\tID:minimap2\tPN:minimap2\tVN:2.24\n").encode()


def synth(n, L, seed=1000, chunk=1 << 16):
    """n fixed-layout records as one uint8 array; returns (text, bytes of each record up to the end of its CIGAR)."""
    rng = np.random.default_rng(seed)
    nops = L // 6
    cig = []
    for _ in range(64):   # CIGARs of equal byte length: 2-digit soft clips around 1-digit ops over M/I/D/=/X
        ops = rng.choice(list("MMMMMIID=X"), nops)
        ln = rng.integers(1, 10, nops)
        cig.append(("%02dS" % rng.integers(10, 100) + "".join("%d%s" % (a, b) for a, b in zip(ln, ops))
                    + "%02dS" % rng.integers(10, 100)).encode())
    seqs = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (16, L))]
    quals = rng.integers(33, 75, (16, L)).astype(np.uint8)
    # QNAME(36) FLAG(4) RNAME(5) POS(9) MAPQ(2) CIGAR ... * 0 0 SEQ QUAL NM:i:dddd tp:A:P
    lay = [36, 4, 5, 9, 2, len(cig[0]), 1, 1, 1, L, L, 9, 6]
    reclen = sum(lay) + len(lay)
    upto = sum(lay[:6]) + 5
    text = np.empty(n * reclen, np.uint8)
    hexd = np.frombuffer(b"0123456789abcdef", np.uint8)
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        m = hi - lo
        idx = np.arange(lo, hi, dtype=np.int64)
        rec = text[lo * reclen:hi * reclen].reshape(m, reclen)
        rec[:, :] = ord("\t")
        o = 0
        name = rec[:, 0:36]
        name[:] = hexd[(idx[:, None] * 2654435761 >> (4 * (np.arange(36) % 15))) & 15]
        name[:, [8, 13, 18, 23]] = ord("-")
        o = 37
        flag = rng.choice(np.array([b"0000", b"0016", b"0004", b"0256", b"2048"]), m, p=[0.45, 0.4, 0.05, 0.05, 0.05])
        rec[:, o:o + 4] = np.frombuffer(flag.tobytes(), np.uint8).reshape(m, 4)
        o += 5
        rec[:, o:o + 5] = np.frombuffer(np.array([r.encode() for r in REFS])[idx % 22].tobytes(), np.uint8).reshape(m, 5)
        o += 6
        pos = rng.integers(1, 10 ** 8, m)
        for d in range(9):
            rec[:, o + 8 - d] = 48 + (pos // 10 ** d) % 10
        o += 10
        mq = rng.integers(0, 61, m)
        rec[:, o], rec[:, o + 1] = 48 + mq // 10, 48 + mq % 10
        o += 3
        cg = np.frombuffer(b"".join(cig), np.uint8).reshape(64, -1)
        rec[:, o:o + lay[5]] = cg[rng.integers(0, 64, m)]
        o += lay[5] + 1
        rec[:, o], rec[:, o + 2], rec[:, o + 4] = ord("*"), ord("0"), ord("0")
        o += 6
        rec[:, o:o + L] = seqs[idx % 16]
        o += L + 1
        rec[:, o:o + L] = quals[(idx + 5) % 16]
        o += L + 1
        rec[:, o:o + 9] = np.frombuffer(b"NM:i:0042", np.uint8)
        o += 10
        rec[:, o:o + 6] = np.frombuffer(b"tp:A:P", np.uint8)
        rec[:, -1] = ord("\n")
    return text, upto


def device_parse(d_text, nbytes, tables, first_line, use_minq=True, minq=10):
    lib = _lib.lib()
    nl, nk, nb = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    t0 = time.perf_counter()
    check(lib.sarlacc_dev_sam_index(d_text.ptr, C.c_int64(nbytes), C.c_int64(first_line), ptr(tables.ref), ptr(tables.ref_off),
                                    C.c_int64(tables.n_ref), None, None, ptr(tables.extra_off), C.c_int64(0), C.c_int(use_minq),
                                    C.c_int64(minq), C.byref(nl), C.byref(nk), C.byref(nb), None))
    t1 = time.perf_counter()
    n = nk.value
    cols, names, noff = DevBuffer(max(21 * n, 1)), DevBuffer(max(nb.value, 1)), DevBuffer(8 * (n + 1))
    b = cols.ptr.value
    t2 = time.perf_counter()
    check(lib.sarlacc_dev_sam_extract(d_text.ptr, C.c_void_p(b), C.c_void_p(b + 4 * n), C.c_void_p(b + 8 * n), C.c_void_p(b + 20 * n),
                                      C.c_void_p(b + 12 * n), C.c_void_p(b + 16 * n), names.ptr, noff.ptr, None))
    t3 = time.perf_counter()
    return (t1 - t0, t3 - t2), n, nb.value, (cols, names, noff)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", type=int, nargs="?", default=100000)
    ap.add_argument("L", type=int, nargs="?", default=2000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--generics", type=int, default=200000)
    a = ap.parse_args()
    body, upto = synth(a.n, a.L)
    head = header()
    names, _, nhead, _ = sam.read_header(io.BytesIO(head))
    tables = sam._Tables(names, None)
    d_text = DevBuffer.from_numpy(body)
    times = []
    for rep in range(a.reps + 1):
        (ti, te), nk, nb, keep = device_parse(d_text, body.size, tables, nhead + 1)
        if rep:
            times.append((ti, te))
        del keep
    tot = sorted(ti + te for ti, te in times)
    best, med = tot[0], tot[len(tot) // 2]
    alg = 2 * body.size + a.n * upto + 21 * nk + nb + 8 * (nk + 1)
    res = {"tool": "perf_sam", "n": a.n, "L": a.L, "text_bytes": int(body.size), "kept": int(nk),
           "index_ms_best": round(min(t[0] for t in times) * 1e3, 3), "extract_ms_best": round(min(t[1] for t in times) * 1e3, 3),
           "device_ms_best": round(best * 1e3, 3), "device_ms_median": round(med * 1e3, 3),
           "algorithmic_bytes": int(alg), "tb_per_s": round(alg / best / 1e12, 3),
           "share_of_8tbs_peak": round(alg / best / HBM_PEAK, 3), "text_gb_per_s": round(body.size / best / 1e9, 1)}
    # whole generics call on a file in the page cache; checked against a direct parse of the same records
    m = min(a.n, a.generics)
    reclen = body.size // a.n
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "perf.sam")
        with open(path, "wb") as fh:
            fh.write(head)
            fh.write(body[:m * reclen].tobytes())
        with open(path, "rb") as fh:
            while fh.read(1 << 26):
                pass
        generics.sam2ranges(path)                     # warm-up
        t0 = time.perf_counter()
        out = generics.sam2ranges(path)
        tg = time.perf_counter() - t0
        res.update({"generics_records": m, "generics_file_bytes": os.path.getsize(path), "generics_s": round(tg, 4),
                    "generics_gb_per_s": round(os.path.getsize(path) / tg / 1e9, 2), "generics_kept": len(out["start"])})
    # CPU baseline: the restatement on 10^4 records, compared with the device on the same records
    from tests import sam_restated as R
    k = min(a.n, 10000)
    small = head + body[:k * reclen].tobytes()
    t0 = time.perf_counter()
    want = R.sam2ranges(small, 10)
    tr = time.perf_counter() - t0
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "small.sam")
        open(path, "wb").write(small)
        ok = R.as_table(generics.sam2ranges(path, 10)) == R.as_table(want)
    res.update({"restated_records": k, "restated_s": round(tr, 3), "restated_records_per_s": round(k / tr),
                "device_records_per_s": round(a.n / best), "device_equals_restated_on_restated_records": ok})
    print(json.dumps(res), flush=True)
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
