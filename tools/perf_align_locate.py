"""A/B of option values of adaptor_align on the benchmark's DP workload (bench.py's reads: same generator, seed and resident
format), one data set and one process for every variant:
    python tools/perf_align_locate.py [reads] [option] [values, comma separated] [rounds] [steps]
Every round runs the variants in turn (the order alternating from round to round), `steps` calls each; a line per variant
and round with the wall time per call and the kernel event time, then min / median / max per variant and, once per variant,
the locator's counters (window steps, class histogram, oversize, redo, stalls).  Option "-": no option is set."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import sarlacc_amd
from sarlacc_amd import _lib, calls, device as sdev, devsynth
import bench

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
opt = sys.argv[2] if len(sys.argv) > 2 else "-"
values = [int(v) for v in sys.argv[3].split(",")] if len(sys.argv) > 3 and opt != "-" else [0]
rounds = int(sys.argv[4]) if len(sys.argv) > 4 else 6
steps = int(sys.argv[5]) if len(sys.argv) > 5 else 10
dev = torch.device("cuda", 0)
sarlacc_amd.set_device(0)
enc = sarlacc_amd.phred_encoding()
seq, qual, off, max_len = devsynth.make_reads(n, 2000, bench.ADAPTOR1, bench.ADAPTOR2, seed=1000, device=dev)
total = int(off[-1].item())
scores = torch.empty(n, dtype=torch.float64, device=dev)
starts = torch.empty(n, dtype=torch.int32, device=dev); ends = torch.empty_like(starts)
sso = torch.empty_like(starts); swo = torch.empty_like(starts)
st = torch.cuda.current_stream().cuda_stream
packed = torch.empty(total // 4 + 2, dtype=torch.uint8, device=dev)
nmask = torch.empty(total // 8 + 1, dtype=torch.uint8, device=dev)
sdev.dev_pack_reads(seq, total, packed, nmask, st)
torch.cuda.synchronize()


def step():
    sdev.dev_align(packed, qual, off, n, max_len, enc, bench.GAP_OPEN, bench.GAP_EXT, bench.ADAPTOR1, True,
                   bench.UMI_SECTION[0], bench.UMI_SECTION[1], scores, starts, ends, sso, swo, st, d_nmask=nmask)
    return sarlacc_amd.last_kernel_ms()


def select(v):
    if opt != "-":
        calls.set_option(opt, v)


wall = {v: [] for v in values}
kern = {v: [] for v in values}
first = None
for v in values:   # warm-up, the counters, and the outputs against the first variant's
    select(v)
    step(); step()
    torch.cuda.synchronize()
    names = ["align_window_steps", "align_oversize", "align_redo", "align_stalls", "align_locate_k"]
    print("%s=%d counters: %s | classes %s" % (opt, v, " ".join("%s %d" % (k[6:], _lib.stage_count(k)) for k in names),
          " ".join("%d:%d" % (c, _lib.stage_count("align_window_class_%d" % c)) for c in range(1, 32)
                   if _lib.stage_count("align_window_class_%d" % c) > 0)), flush=True)
    got = [t.cpu().numpy().copy() for t in (scores, starts, ends, sso, swo)]
    got[0] = got[0].view(np.int64)
    if first is None:
        first = got
    else:
        print("%s=%d outputs identical to %s=%d: %s" % (opt, v, opt, values[0], all(np.array_equal(a, b) for a, b in zip(first, got))), flush=True)
for r in range(rounds):
    for v in (values if r % 2 == 0 else values[::-1]):
        select(v)
        step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        k = [step() for _ in range(steps)]
        torch.cuda.synchronize()
        wall[v].append((time.perf_counter() - t0) / steps * 1e3)
        kern[v].append(sum(k) / len(k))
        print("round %d %s=%d ms_per_step %.3f kernel_ms %.3f" % (r, opt, v, wall[v][-1], kern[v][-1]), flush=True)
for v in values:
    w, k = sorted(wall[v]), sorted(kern[v])
    print("%s=%d ms_per_step min %.3f median %.3f max %.3f | kernel_ms min %.3f median %.3f max %.3f" %
          (opt, v, w[0], float(np.median(w)), w[-1], k[0], float(np.median(k)), k[-1]), flush=True)
select(0)
