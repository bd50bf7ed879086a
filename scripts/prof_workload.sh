# rocprofv3 kernel trace of one workload: prof_workload.sh <workload> <steps> <tag>  ->  $KT_PROF_OUT/prof_<tag>_kernel_stats.csv + prof_<tag>_bench.json (default: prof_out/)
R=$(cd "$(dirname "$0")/.." && pwd); O=${KT_PROF_OUT:-$R/prof_out}; mkdir -p $O
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_$3 -- python $R/bench.py --full --workload $1 --steps $2 --warmup 10 --no-cpu-baseline --no-contract-ab > $O/prof_$3.log 2>&1
grep '^{"metric"' $O/prof_$3.log | tail -1 > $O/prof_$3_bench.json
cut -c1-150 $O/prof_$3_bench.json
python $R/scripts/split_kernel_stats.py "$(find $O/prof_$3 -name '*kernel_stats.csv' | head -1)" $O/prof_$3_kernel_stats.csv
cut -c1-150 $O/prof_$3_kernel_stats.csv | head -24
