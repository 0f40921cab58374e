# rocprofv3 kernel stats of one full bench run (top kernels by total time)
#   usage: tools/kstats.sh <tag> [extra bench.py args]; the stats go under $KSTATS_OUT/<tag> (default: kstats_out/ in the repository)
TAG=${1:-kstats}; shift || true
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=${KSTATS_OUT:-$ROOT/kstats_out}
mkdir -p "$OUT"
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/$TAG" -o st -- python3 "$ROOT/bench.py" --full --no-cpu --no-host-pointer --steps 1 "$@" > "$OUT/$TAG.log" 2>&1
cd "$ROOT"
python3 - "$OUT/$TAG" <<'PY'
import csv, glob, sys
for f in glob.glob(sys.argv[1] + "/**/*kernel_stats.csv", recursive=True):
    rows = list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: -float(r["TotalDurationNs"]))
    for r in rows[:12]:
        print("%-70s calls %5s total %9.1f ms avg %8.3f ms" % (r["Name"][:70], r["Calls"], float(r["TotalDurationNs"])/1e6, float(r["AverageNs"])/1e6))
PY
find "$OUT/$TAG" -name "*kernel_trace.csv" -delete
