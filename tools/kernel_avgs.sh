# average kernel durations of a short bench run under rocprofv3 (1024 frames): bash tools/kernel_avgs.sh [workload, default cnn+solver] [output directory, default a new one under /tmp]
WL=${1:-cnn+solver}
R=$(cd "$(dirname "$0")/.." && pwd)
K=${2:-$(mktemp -d /tmp/kavg.XXXXXX)}
mkdir -p "$K" && K=$(cd "$K" && pwd)      # absolute: the run below starts from /tmp
cd /tmp && export TMPDIR=/tmp
rm -rf $K/trace
rocprofv3 --kernel-trace --stats --output-format csv -d $K/trace -o t -- python3 $R/bench.py --full --workload $WL --steps 5 --warmup 2 --no-cpu-baseline > /dev/null 2> $K/bench.err || exit 1
python3 - <<PY
import csv,glob
f=glob.glob("$K/trace/**/t_kernel_stats.csv",recursive=True)[0]
for r in csv.DictReader(open(f)):
    n=r["Name"].split("(")[0]
    if float(r["Percentage"])>0.5: print("%-40s %4s calls  avg %8.1f us  %5s %%" % (n[:40], r["Calls"], float(r["AverageNs"])/1e3, r["Percentage"]))
PY
