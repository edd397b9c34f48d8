#!/bin/bash
# Regenerates the round-5 measurement artefacts under gpurun_out/r05/ (copy into profiles/ what is to be judged):
#   bench lines (default = f16x3 with every extra; fp32; bf16x6; tail_x3; config 5's architecture), rocprofv3 kernel stats of the same command (two
#   streams and single stream = true durations), SQ counters of EVERY kernel of the step (two --pmc passes, kernel-trace only),
#   SQ counters + HBM-side traffic of the dominant kernel on the stand-alone harness, the inference forward trace.
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
O=gpurun_out/r05; rm -rf $O; mkdir -p $O
timeout -k 10 700 python3 bench.py --full --steps 20 --warmup 3 > $O/bench_f16x3.json 2> $O/bench_f16x3.err || { tail -5 $O/bench_f16x3.err; exit 1; }
echo "bench default done: $(python3 -c "import json;d=json.load(open('$O/bench_f16x3.json'));print(d['ms_per_step'], d['value'])")"
for m in fp32 bf16x6 tail_x3; do
  timeout -k 10 300 python3 bench.py --full --steps 20 --warmup 3 --no-cpu-baseline --no-extras --math $m > $O/bench_$m.json 2> /dev/null
  echo "bench $m: $(python3 -c "import json;d=json.load(open('$O/bench_$m.json'));print(d['ms_per_step'], d['roofline']['launch_ms'], d['roofline']['frac'])")"
done
timeout -k 10 400 python3 bench.py --F 40 --genotype 40_5e_38_lr/genotype_1 --steps 10 --warmup 2 --no-cpu-baseline --no-extras > $O/bench_config5_F40_genotype1.json 2> /dev/null
echo "config 5 (F=40 g1): $(python3 -c "import json;d=json.load(open('$O/bench_config5_F40_genotype1.json'));print(d['ms_per_step'], d['value'], d['plan_device_gb'])")"
for s in 2 1; do
  rm -rf $O/pt; mkdir -p $O/pt
  ADDK_STREAMS=$s timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $O/pt -- python3 bench.py --steps 5 --warmup 2 --no-cpu-baseline --no-extras > /dev/null 2>&1
  cp $(ls $O/pt/*/*kernel_stats.csv | head -1) $O/step_kernel_stats_${s}stream.csv
  python3 scripts/trace_summary.py $(ls $O/pt/*/*kernel_trace.csv | head -1) 90 > $O/step_last_step_summary_${s}stream.txt
  python3 scripts/overlap.py $(ls $O/pt/*/*kernel_trace.csv | head -1) > $O/step_overlap_${s}stream.txt
  rm -rf $O/pt
done
head -3 $O/step_last_step_summary_2stream.txt
# SQ counters of every kernel of the step: two passes of 8 counters, single stream, kernel-trace only
rm -rf $O/pmc_a $O/pmc_b
ADDK_STREAMS=1 timeout -k 10 400 rocprofv3 --pmc SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_INSTS_VALU SQ_VALU_MFMA_BUSY_CYCLES --kernel-trace --output-format csv -d $O/pmc_a -- python3 bench.py --steps 2 --warmup 1 --no-cpu-baseline --no-extras --no-graph > /dev/null 2>&1
ADDK_STREAMS=1 timeout -k 10 400 rocprofv3 --pmc SQ_WAVES SQ_WAVE_CYCLES SQ_INSTS_LDS SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_WAIT_INST_LDS SQ_INSTS_MFMA SQ_ACTIVE_INST_LDS --kernel-trace --output-format csv -d $O/pmc_b -- python3 bench.py --steps 2 --warmup 1 --no-cpu-baseline --no-extras --no-graph > /dev/null 2>&1
python3 - <<'PY' > gpurun_out/r05/pmc_step_sq_summary.txt
import csv, glob, collections
O = 'gpurun_out/r05'
agg = collections.defaultdict(lambda: collections.defaultdict(float)); cnt = collections.Counter()
for d in ('pmc_a', 'pmc_b'):
    f = glob.glob('%s/%s/*/*counter_collection.csv' % (O, d))
    if not f: continue
    seen = set()
    for r in csv.DictReader(open(f[0])):
        k = r['Kernel_Name'].replace('(anonymous namespace)::', '').replace('void ', '').split('(')[0][:48]
        agg[k][d + ':' + r['Counter_Name']] += float(r['Counter_Value'])
        if d == 'pmc_a' and (r['Dispatch_Id'], k) not in seen: seen.add((r['Dispatch_Id'], k)); cnt[k] += 1
print('# SQ counters per kernel over 3 eager single-stream steps of bench.py (rocprofv3 --pmc, two passes); sorted by wave cycles')
for k, v in sorted(agg.items(), key=lambda kv: -kv[1]['pmc_a:SQ_WAVE_CYCLES'])[:40]:
    n = max(cnt[k], 1); wc = v['pmc_a:SQ_WAVE_CYCLES']
    if not wc: continue
    wb = v['pmc_b:SQ_WAVE_CYCLES'] or 1
    print('%-50s launches %4d  waves/launch %6.0f  issuing %4.1f%%  wait_any %4.1f%%  wait_inst %4.1f%%  VALU/wave %6.0f  MFMA/wave %5.0f  LDS/wave %5.0f  LDS conflict cyc/idx-active %.3f  wait_inst_lds %4.1f%%' % (
        k, n, v['pmc_a:SQ_WAVES'] / n, 100 * v['pmc_a:SQ_ACTIVE_INST_ANY'] / wc, 100 * v['pmc_a:SQ_WAIT_ANY'] / wc, 100 * v['pmc_a:SQ_WAIT_INST_ANY'] / wc,
        v['pmc_a:SQ_INSTS_VALU'] / max(v['pmc_a:SQ_WAVES'], 1), v['pmc_b:SQ_INSTS_MFMA'] / max(v['pmc_b:SQ_WAVES'], 1), v['pmc_b:SQ_INSTS_LDS'] / max(v['pmc_b:SQ_WAVES'], 1),
        v['pmc_b:SQ_LDS_BANK_CONFLICT'] / max(v['pmc_b:SQ_LDS_IDX_ACTIVE'], 1), 100 * v['pmc_b:SQ_WAIT_INST_LDS'] / wb))
PY
rm -rf $O/pmc_a $O/pmc_b
head -12 $O/pmc_step_sq_summary.txt
ADDK_MATH=f16x3 bash scripts/pmc_traffic.sh $O | tail -1      # SQ counters + HBM-side traffic of the dominant launch (decoder 3x3), stand-alone harness
ADDK_MATH=bf16x6 bash scripts/pmc_traffic.sh $O | tail -1
# the list the model really runs (level-ordered, batched, two streams): inference and training forward, kernel by kernel
for m in eval train; do
  rm -rf $O/ft; timeout -k 10 300 rocprofv3 --kernel-trace --output-format csv -d $O/ft -- python3 scripts/fwd_trace.py --mode $m --real > /dev/null 2>&1 && python3 scripts/fwd_trace.py --csv $(ls $O/ft/*/*kernel_trace.csv | head -1) --top 50 > $O/fwd_${m}_kernels_two_streams_batched.txt 2>&1; rm -rf $O/ft
done
# inference forward, kernel by kernel
rm -rf $O/ft; timeout -k 10 300 rocprofv3 --kernel-trace --output-format csv -d $O/ft -- python3 scripts/fwd_trace.py --mode eval > /dev/null 2>&1 && python3 scripts/fwd_trace.py --csv $(ls $O/ft/*/*kernel_trace.csv | head -1) --top 60 > $O/fwd_eval_kernels.txt 2>&1; rm -rf $O/ft
head -3 $O/fwd_eval_kernels.txt
