# every bench workload once; results -> $KT_PROF_OUT/workloads_r06.jsonl (default: prof_out/)
R=$(cd "$(dirname "$0")/.." && pwd); O=${KT_PROF_OUT:-$R/prof_out}; mkdir -p $O
out=$O/workloads_r06.jsonl; : > $out
for w in orbit512 orbit256 crabwalk512 farwall768; do
  steps=200; [ $w = farwall768 ] && steps=40
  timeout 600 python $R/bench.py --full --workload $w --steps $steps --warmup 10 --cpu-frames 6 --no-stress 2>$O/$w.err | tail -1 >> $out || echo "{\"workload\": \"$w\", \"failed\": true}" >> $out
  tail -2 $O/$w.err
done
python - <<PY
import json
for l in open('$out'):
    try: d=json.loads(l)
    except Exception as e: print('bad line', l[:200]); continue
    if 'value' not in d: print(d); continue
    print(d['config']['workload'][:40], round(d['value'],1), 'fps', d['roofline']['frac'], d['roofline']['avg_launch_ms'], d['roofline']['U_voxels_updated'], d.get('cpu_baseline',{}).get('value'), d['config']['pose_err_m_at_end'])
PY
