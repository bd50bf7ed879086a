# rocprofv3 kernel trace of the default bench workload: prof_bench.sh [tag]  ->  $KT_PROF_OUT/prof_<tag>/ + prof_<tag>_bench.json (default: prof_out/)
R=$(cd "$(dirname "$0")/.." && pwd); T=${1:-r05_final}; O=${KT_PROF_OUT:-$R/prof_out}; mkdir -p $O
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_$T -- python $R/bench.py --full --steps 200 --warmup 20 --no-cpu-baseline --no-contract-ab --no-stress > $O/prof_${T}_bench.log 2>&1
# the bench's JSON line, NOT the log's last line (rocprofv3 writes its own finalisation message behind it)
grep '^{"metric"' $O/prof_${T}_bench.log | tail -1 > $O/prof_${T}_bench.json
cut -c1-200 $O/prof_${T}_bench.json
python $R/scripts/split_kernel_stats.py "$(find $O/prof_$T -name '*kernel_stats.csv' | head -1)" $O/prof_${T}_kernel_stats.csv   # counting variants below a separator
head -24 $O/prof_${T}_kernel_stats.csv | cut -c1-160
