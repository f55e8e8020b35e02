# The measurement set behind profiles/r03t_* (one MI355X):  bash scripts/r03_final.sh <tag>
set -x
TAG=${1:-r03t}
O=gpurun_out/$TAG; mkdir -p $O
nproc > $O/host.txt; lscpu | grep "Model name" >> $O/host.txt; cat /sys/fs/cgroup/cpu.max >> $O/host.txt 2>/dev/null
timeout 2400 python -m pytest tests -q -s -m gpu > $O/gpu_tests.log 2>&1; echo "tests rc=$?"
timeout 900 python bench.py --full > $O/bench_line.json 2> $O/bench.err; echo "bench rc=$?"
timeout 600 python bench.py --full --gpus 1 --steps 20 --warmup 3 --no-cpu-baseline > $O/bench_driverargs_line.json 2>/dev/null
timeout 600 python bench.py --full --force-comm --no-cpu-baseline > $O/bench_forcecomm_line.json 2>/dev/null
timeout 600 python bench.py --full --dtype bf16 --batch-per-gpu 128 --no-cpu-baseline > $O/bench_bf16_b128_line.json 2>/dev/null
timeout 600 python bench.py --full --workload audio_tower --no-cpu-baseline > $O/audio_tower_line.json 2>/dev/null
timeout 600 python bench.py --full --workload vision_tower --no-cpu-baseline > $O/vision_tower_line.json 2>/dev/null
L3_DEBUG_KNOBS=1 L3_WINO4=0 timeout 600 python bench.py --full --no-cpu-baseline > $O/bench_f2x2_line.json 2>/dev/null
R=$GRAFT_REPO_ROOT
cd /tmp && export TMPDIR=/tmp
timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d $R/$O/prof_f32 -o f32 -- python $R/bench.py --full --serial --steps 10 --no-cpu-baseline --roofline-steps 0 > $R/$O/prof_f32.log 2>&1
cd $R
cp $(find $O/prof_f32 -name "*kernel_stats.csv" | head -1) $O/bench_serial_kernel_stats.csv
python scripts/wgw_layers.py $(find $O/prof_f32 -name "*kernel_trace.csv" | head -1) conv_w > $O/conv_kernel_durations.txt
python scripts/wino_layers_by_order.py $(find $O/prof_f32 -name "*kernel_trace.csv" | head -1) > $O/wino4_layer_durations.txt
bash scripts/pmc_conv.sh $O/pmc > $O/pmc.log 2>&1
timeout 600 python scripts/train_e2e_throughput.py concurrent > $O/train_e2e.txt 2>&1
find $O -name "*.db" -delete; find $O -name "*kernel_trace.csv" -delete; find $O -size +4M -delete
grep -a "passed\|failed" $O/gpu_tests.log | tail -2
