"""barcodeAlign over a whole panel: n reads of 24 +- 3 bases (Phred+33, seeded) against panels of 1, 12, 96 and
384 barcodes of 24 columns and one panel of 96 barcodes of 16 columns with two N columns.  Three routes in one process,
warmed and alternating, each timed as wall time around a call that ends in a synchronise:
  (a) one DeviceReads.align_scores(local=False) per barcode + the numpy fold (what generics.barcodeAlign did before the panel call),
  (b) DeviceReads.barcode_panel with align_panel = -1 (every barcode by k_align, folded on the device),
  (c) DeviceReads.barcode_panel (k_barcode_panel).
The three must return identical arrays at the timed size before any time is printed.  For (b) and (c) the DP launches'
own time is sarlacc_last_kernel_ms; the share of the fp64 VALU peak uses the README's definition for k_align: 10 fp64
lane-operations per cell over 39.32 T/s.

usage: perf_barcode_panel.py [n=1000000] [repeats=5] [--out record.json]"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import sarlacc_amd
from sarlacc_amd import _lib, calls, generics
from sarlacc_amd.resident import DeviceReads
from sarlacc_amd.strset import StringSet

PEAK_LANE_OPS = 39.32e12
OPS_PER_CELL = 10


def reads(n, rng):
    lengths = rng.integers(21, 28, n)
    off = np.zeros(n + 1, np.int64)
    np.cumsum(lengths, out=off[1:])
    seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(off[-1]))]
    qual = rng.integers(33 + 5, 33 + 41, int(off[-1])).astype(np.uint8)
    return generics.Reads(StringSet(seq, off), StringSet(qual, off.copy()))


def panel(nb, cols, rng, n_columns=0):
    out = []
    for _ in range(nb):
        bc = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, cols)].copy()
        bc[rng.choice(cols, n_columns, replace=False)] = ord("N")
        out.append(bc.tobytes().decode())
    return out


def route_a(dev, barcodes, go, ge):
    n = len(dev)
    cur, nxt, ident = np.full(n, -np.inf), np.full(n, -np.inf), np.zeros(n, np.int32)
    for b, bc in enumerate(barcodes):
        scores = dev.align_scores(bc, go, ge, local=False)
        keep = scores > cur
        second = ~keep & (scores > nxt)
        ident[keep] = b + 1
        nxt[keep] = cur[keep]
        cur[keep] = scores[keep]
        nxt[second] = scores[second]
    return ident, cur, nxt


def route_panel(dev, barcodes, go, ge, option):
    calls.set_option("align_panel", option)
    try:
        out = dev.barcode_panel(barcodes, go, ge)
        return out, _lib.last_kernel_ms(), _lib.stage_count("panel_launches")
    finally:
        calls.set_option("align_panel", 0)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    if out_path:
        args.remove(out_path)
    n = int(args[0]) if args else 1000000
    repeats = max(int(args[1]) if len(args) > 1 else 5, 5)
    if sarlacc_amd.device_count() < 1:
        raise SystemExit("perf_barcode_panel needs a HIP device")
    rng = np.random.default_rng(20240)
    rd = reads(n, rng)
    dev = DeviceReads.upload(rd)
    bases = dev.total
    go, ge = 5, 1
    record = {"n": n, "bases": bases, "repeats": repeats, "penalties": [go, ge], "cases": []}
    cases = [(1, 24, 0), (12, 24, 0), (96, 24, 0), (384, 24, 0), (96, 16, 2)]
    for nb, cols, ncol in cases:
        barcodes = panel(nb, cols, rng, ncol)
        cells = float(bases) * cols * nb
        # warm every route at the timed size and compare their results
        ra = route_a(dev, barcodes, go, ge)
        (rb, _, lb), (rc, _, lc) = route_panel(dev, barcodes, go, ge, -1), route_panel(dev, barcodes, go, ge, 0)
        for x, y, z in zip(ra, rb, rc):
            xb, yb, zb = (np.ascontiguousarray(v).view(np.int64 if v.dtype == np.float64 else np.int32) for v in (x, y, z))
            if not (np.array_equal(xb, yb) and np.array_equal(xb, zb)):
                raise SystemExit("routes disagree at %d barcodes of %d columns" % (nb, cols))
        wall = {"a": [], "b": [], "c": []}
        kms = {"b": [], "c": []}
        for _ in range(repeats):
            t0 = time.perf_counter(); route_a(dev, barcodes, go, ge); wall["a"].append(time.perf_counter() - t0)
            t0 = time.perf_counter(); _, k, _ = route_panel(dev, barcodes, go, ge, -1); wall["b"].append(time.perf_counter() - t0); kms["b"].append(k)
            t0 = time.perf_counter(); _, k, _ = route_panel(dev, barcodes, go, ge, 0); wall["c"].append(time.perf_counter() - t0); kms["c"].append(k)
        case = {"barcodes": nb, "columns": cols, "n_columns": ncol, "cells": cells, "launches_b": lb, "launches_c": lc,
                "wall_s": {k: [min(v), max(v)] for k, v in wall.items()}, "kernel_ms": {k: [min(v), max(v)] for k, v in kms.items()}}
        kc, kb = min(kms["c"]) / 1e3, min(kms["b"]) / 1e3
        case["c_gcups_kernel"] = cells / kc / 1e9
        case["b_gcups_kernel"] = cells / kb / 1e9
        case["c_share_of_fp64_valu_peak"] = cells * OPS_PER_CELL / kc / PEAK_LANE_OPS
        case["b_share_of_fp64_valu_peak"] = cells * OPS_PER_CELL / kb / PEAK_LANE_OPS
        case["c_gcups_wall"] = cells / min(wall["c"]) / 1e9
        case["wall_ratio_a_over_c"] = [min(wall["a"]) / max(wall["c"]), max(wall["a"]) / min(wall["c"])]
        case["c_faster_than_a_over_the_whole_spread"] = max(wall["c"]) < min(wall["a"])
        record["cases"].append(case)
        print("%3d barcodes x %2d columns (%d N): identical results; wall s min-max  (a) %.4f-%.4f  (b) %.4f-%.4f  (c) %.4f-%.4f"
              % (nb, cols, ncol, *case["wall_s"]["a"], *case["wall_s"]["b"], *case["wall_s"]["c"]))
        print("      kernel ms min-max  (b) %.3f-%.3f in %d launches  (c) %.3f-%.3f in %d launch(es)"
              % (*case["kernel_ms"]["b"], lb, *case["kernel_ms"]["c"], lc))
        print("      (c) %.1f GCUPS in-kernel = %.1f %% of the fp64 VALU peak, %.1f GCUPS wall; (b) %.1f GCUPS in-kernel = %.1f %%; "
              "wall (a)/(c) %.1f-%.1f x" % (case["c_gcups_kernel"], 100 * case["c_share_of_fp64_valu_peak"], case["c_gcups_wall"],
                                          case["b_gcups_kernel"], 100 * case["b_share_of_fp64_valu_peak"], *case["wall_ratio_a_over_c"]), flush=True)
    print(json.dumps(record))
    if out_path:
        with open(out_path, "w") as fh:
            json.dump(record, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
