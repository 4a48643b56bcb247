# usage (on an MI355X): bash tools/profile_round.sh [round tag, default r04]; raw output under $OUT (default profile_out/)
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
T=${1:-r04}
OUT=${OUT:-$R/profile_out}
export TMPDIR=/tmp
cd $R
mkdir -p $OUT
for S in 512 1024; do
  rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${T}a_s$S -- python3 bench.py --full --no-cpu-baseline --no-extra --size $S > $OUT/${T}a_bench_$S.json 2> $OUT/${T}a_s$S.err
  echo "stats $S done"
  rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $OUT/${T}a_f$S -- python3 bench.py --full --no-cpu-baseline --no-extra --size $S --steps 3 --warmup 2 > /dev/null 2> $OUT/${T}a_f$S.err
  echo "fetch $S done"
  rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $OUT/${T}a_w$S -- python3 bench.py --full --no-cpu-baseline --no-extra --size $S --steps 3 --warmup 2 > /dev/null 2> $OUT/${T}a_w$S.err
  echo "write $S done"
  python tools/gap_report.py $OUT/${T}a_s$S > $OUT/${T}_step_timeline_$S.txt
done
python tools/summarize_profile.py $T $OUT/${T}a
ls -la profiles | tail -8
# keep only the small outputs
find $OUT/${T}a_s512 $OUT/${T}a_s1024 $OUT/${T}a_f512 $OUT/${T}a_f1024 $OUT/${T}a_w512 $OUT/${T}a_w1024 -name "*kernel_trace.csv" -delete || true
find $OUT -name "*counter_collection.csv" -size +5M -delete || true
