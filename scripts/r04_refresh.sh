#!/bin/bash
# Round-4 measurement refresh on the GPU box: device suite, the default bench line, kernel-trace summaries (env step, PPO epoch), PMC traffic and SQ counters.
O=gpurun_out/${1:-r4r}
mkdir -p $O
if [ -z "$SKIP_PYTEST" ]; then timeout 1500 python -m pytest tests -m gpu -q > $O/pytest_gpu.log 2>&1; tail -3 $O/pytest_gpu.log; fi
python __graft_entry__.py --smoke > $O/smoke.log 2>&1; tail -1 $O/smoke.log
python bench.py --full > $O/bench_default.json 2> $O/bench_default.err; tail -c 400 $O/bench_default.err
python bench.py --full --actions tracking --no-cpu-baseline --no-pmc --ppo-epochs 0 > $O/bench_tracking.json 2>> $O/bench_default.err
python bench.py --full --config 5 --ppo-epochs 0 --no-cpu-baseline --no-pmc > $O/bench_h1.json 2>> $O/bench_default.err
python bench.py --full --steps 20 --warmup 5 > $O/bench_driver_style.json 2>> $O/bench_default.err
python bench.py --full --robot g1 --ppo-epochs 0 --no-cpu-baseline --no-pmc --no-other-workloads > $O/bench_g1.json 2>> $O/bench_default.err
if [ -n "$WITH_CONFIG3" ]; then python bench.py --full --config 3 --ppo-epochs 0 --no-cpu-baseline --no-pmc > $O/bench_config3.json 2>> $O/bench_default.err; fi
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
rocprofv3 --kernel-trace --stats -d /tmp/prof -o bench -- python bench.py --full --steps 200 --warmup 20 --ppo-epochs 0 --no-cpu-baseline --no-pmc --no-other-workloads > $O/prof_bench.json 2> $O/prof.err
python profiles/summarize_rocpd.py $(find /tmp/prof -name '*.db' | head -1) > $O/env_step_kernel_stats.txt
rocprofv3 --kernel-trace --stats -d /tmp/prof2 -o ppo -- python bench.py --full --steps 20 --warmup 5 --ppo-epochs 1 --no-cpu-baseline --no-pmc --no-other-workloads > $O/prof_ppo.json 2>> $O/prof.err
python profiles/summarize_rocpd.py $(find /tmp/prof2 -name '*.db' | head -1) > $O/ppo_epoch_kernel_stats.txt
python profiles/dump_step.py $(find /tmp/prof2 -name '*.db' | head -1) > $O/ppo_optimizer_step_kernels.txt 2>> $O/prof.err || true
bash profiles/collect_pmc.sh > $O/pmc_traffic.txt 2>> $O/prof.err
bash profiles/collect_pmc_valu.sh > $O/pmc_valu.txt 2>> $O/prof.err
python - <<PY
import json
d=json.load(open('$O/bench_default.json'))
print('value', round(d['value']/1e6,2), 'M; ms', round(d['ms_per_step'],4), 'stepper us', round(d['roofline']['kernel_ms']*1e3,1), 'frac', round(d['roofline']['frac'],4), 'traffic', d['roofline']['traffic'])
print({k: (round(v,1) if isinstance(v,float) else v) for k, v in d.items() if k.startswith('ppo_') and not isinstance(v, dict)})
for n in ('tracking','h1'):
    t=json.load(open('$O/bench_%s.json'%n)); print(n, round(t['value']/1e6,2), round(t['roofline']['kernel_ms']*1e3,1))
PY
head -7 $O/env_step_kernel_stats.txt | cut -c1-150; cat $O/pmc_traffic.txt | cut -c1-200 | tail -8
