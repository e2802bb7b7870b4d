# Full GPU check on one MI355X box (gpurun --timeout 2400 -- "bash tools/gpu_full_check.sh [tag]"): pytest -m gpu, smoke, bench.py,
# rocprofv3 --kernel-trace --stats of the bench command and of the pipeline, and the three --pmc passes (SQ / FETCH_SIZE / WRITE_SIZE).
# Outputs under $VTTS_OUT (default out/), files named after <tag>.
R=$PWD; T=${1:-full}; O=$(realpath -m "${VTTS_OUT:-out}"); mkdir -p "$O"
timeout 1200 python -m pytest tests -m gpu -q -x --timeout 300 > $O/pytest_gpu.log 2>&1; echo "pytest rc=$?" >> $O/pytest_gpu.log
grep -a "passed\|failed\|rc=\|bf16 B=" $O/pytest_gpu.log | tail -5
timeout 300 python __graft_entry__.py smoke 2>&1 | tail -1
timeout 600 python bench.py --full > $O/bench_$T.json 2> $O/bench_$T.err; cut -c1-400 $O/bench_$T.json; tail -2 $O/bench_$T.err
cd /tmp && export TMPDIR=/tmp
timeout 600 rocprofv3 --kernel-trace --stats -d $O/prof_$T -o r -- python $R/bench.py --steps 2 --warmup 1 --no-cpu-baseline --no-rtf --no-f32 > $O/prof_$T.log 2>&1
python $R/tools/rocprof_summary.py $(find $O/prof_$T -name "*results.db" | head -1) $O/prof_${T}_stats.md
timeout 600 rocprofv3 --kernel-trace --stats -d $O/profpipe_$T -o r -- python $R/tools/pipeline_bench.py 256 > $O/profpipe_$T.log 2>&1
python $R/tools/rocprof_summary.py $(find $O/profpipe_$T -name "*results.db" | head -1) $O/profpipe_${T}_stats.md
for pass in "SQ_VALU_MFMA_BUSY_CYCLES SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE GRBM_GUI_ACTIVE" "FETCH_SIZE" "WRITE_SIZE TCC_HIT_sum TCC_MISS_sum"; do
  tag=$(echo $pass | cut -d' ' -f1)
  timeout 600 rocprofv3 --kernel-trace --pmc $pass --output-format csv -d $O/pmc_$T/$tag -- python $R/bench.py --steps 1 --warmup 1 --no-cpu-baseline --no-rtf --no-f32 > $O/pmc_${T}_$tag.log 2>&1
done
python $R/tools/pmc_csv_summary.py $O/pmc_$T > $O/pmc_${T}_summary.txt 2>&1
find $O -name "*.csv" -size +5M -delete; find $O -name "*.db" -size +20M -delete
