#!/bin/bash
# Round-5 GPU sessions.  Usage: gpurun --timeout N -- 'bash tools/gpu_round5.sh [stage...]'
# Every stage writes under gpurun_out/ (merged back by gpurun); summaries that are kept get copied into profiles/ by hand.
set -u
mkdir -p gpurun_out
cd "$(dirname "$0")/.."
export TMPDIR=/tmp
R="$PWD"
STAGES="${*:-headline benchq}"
BENCHQ="--full --steps 3 --warmup 1 --no-cpu-baseline --h2d-steps 0 --plain-steps 0"
for s in $STAGES; do
  case $s in
    alltests)
      timeout 1800 python -m pytest tests -m gpu -q --tb=short -p no:cacheprovider -s --durations=15 > gpurun_out/pytest_gpu.log 2>&1
      echo "pytest rc=$?" >> gpurun_out/pytest_gpu.log; tail -3 gpurun_out/pytest_gpu.log ;;
    headline)
      # the configuration `value` is measured on, all at once (bf16 weights + e4m3 pre-activation everywhere + last-block pruning)
      timeout 900 python -m pytest tests/test_model_gpu.py tests/test_dist_gpu.py -m gpu -q --tb=short -p no:cacheprovider -s \
        -k "${HEADLINE_K:-headline or per_tensor or two_rank_step or unpadded}" > gpurun_out/pytest_headline.log 2>&1
      echo "pytest rc=$?" >> gpurun_out/pytest_headline.log; grep -a "worst\|passed\|failed\|rc=" gpurun_out/pytest_headline.log | tail -20 ;;
    newtests)
      timeout 1200 python -m pytest ${NEWTESTS_FILES:-tests/test_kernels_gpu.py} -m gpu -q --tb=short -p no:cacheprovider -s \
        -k "${NEWTESTS_K:-attention}" > gpurun_out/pytest_new.log 2>&1
      echo "pytest rc=$?" >> gpurun_out/pytest_new.log; tail -5 gpurun_out/pytest_new.log ;;
    h8conv)
      # VERDICT r4 next #1b: bf16 with and without the e4m3 pre-activation tier, same seeds / data / optimizer
      for seed in ${H8CONV_SEEDS:-1 2}; do
        timeout 600 python tools/fp8_convergence.py --arms bf16,bf16_h8 --steps 200 --batch 256 --lr ${H8CONV_LR:-3e-4} --seed $seed --oracle-steps 0 \
          > gpurun_out/h8_convergence_seed$seed.jsonl 2> gpurun_out/h8_convergence_seed$seed.err; echo "rc=$?" >> gpurun_out/h8_convergence_seed$seed.err
        tail -1 gpurun_out/h8_convergence_seed$seed.jsonl | cut -c1-600
      done ;;
    bench)
      timeout 900 python bench.py --shapes > gpurun_out/bench.log 2>&1; echo "rc=$?" >> gpurun_out/bench.log; tail -2 gpurun_out/bench.log | cut -c1-1500 ;;
    benchq)
      timeout 600 python bench.py --shapes $BENCHQ ${BENCHQ_ARGS:-} > gpurun_out/benchq.log 2>&1; echo "rc=$?" >> gpurun_out/benchq.log
      grep -a "^{" gpurun_out/benchq.log | cut -c1-1800; grep -a "SHAPE attention" gpurun_out/benchq.log | head -8 ;;
    benchq2)
      timeout 600 python bench.py --shapes $BENCHQ ${BENCHQ2_ARGS:-} > gpurun_out/benchq2.log 2>&1; echo "rc=$?" >> gpurun_out/benchq2.log
      grep -a "^{" gpurun_out/benchq2.log | cut -c1-1800 ;;
    benchdist)
      # the multi-rank code path (RCCL group, DDP, vote-based keep plan, per-rank record) on one GPU
      CLIPA_BENCH_FORCE_DIST=1 timeout 600 python -m torch.distributed.run --nnodes=1 --nproc-per-node 1 --master-addr 127.0.0.1 --master-port 29655 \
        bench.py --gpus 1 $BENCHQ ${BENCHDIST_ARGS:-} > gpurun_out/bench_dist1.log 2>&1; echo "rc=$?" >> gpurun_out/bench_dist1.log
      grep -a "^{" gpurun_out/bench_dist1.log | cut -c1-1200 ;;
    driverbench)
      timeout 900 python bench.py --gpus 1 --steps 20 --warmup 5 > gpurun_out/bench_driver_form.log 2>&1; echo "rc=$?" >> gpurun_out/bench_driver_form.log
      grep -a "^{" gpurun_out/bench_driver_form.log | cut -c1-1500 ;;
    attnab)
      # several builds of the attention kernels side by side (tools/probes/attn_ab.hip): outputs compared on the device, timed interleaved
      timeout 600 ./tools/probes/attn_ab ${ATTNAB_ARGS:-} > gpurun_out/attn_ab.jsonl 2>&1; echo "rc=$?" >> gpurun_out/attn_ab.jsonl; tail -30 gpurun_out/attn_ab.jsonl | cut -c1-400 ;;
    flagsweep)
      # clipa_gemm_nt at the production launch shapes under a list of experiment-flag words (tile-group size override = gm << 20)
      timeout 600 ./tools/probes/gemm_flag_sweep ${FLAGSWEEP_ARGS:-0 2097152 4194304 8388608 16777216 33554432} > gpurun_out/gemm_flag_sweep.jsonl 2>&1; echo "rc=$?" >> gpurun_out/gemm_flag_sweep.jsonl
      cat gpurun_out/gemm_flag_sweep.jsonl | cut -c1-400 ;;
    smoke)
      timeout 300 python __graft_entry__.py smoke > gpurun_out/smoke.log 2>&1; echo "rc=$?" >> gpurun_out/smoke.log; tail -2 gpurun_out/smoke.log ;;
    vendor)
      # hipBLASLt vs gemm_nta on the production shapes, same process, interleaved, rocm-smi power / clock sampled during each
      timeout 600 python tools/hipblaslt_compare.py ${VENDOR_ARGS:-} > gpurun_out/vendor_gemm_comparison.jsonl 2> gpurun_out/vendor_gemm_comparison.err
      echo "rc=$?" >> gpurun_out/vendor_gemm_comparison.err; tail -12 gpurun_out/vendor_gemm_comparison.jsonl | cut -c1-500 ;;
    others)
      timeout 400 python bench.py --model ViT-B-16 $BENCHQ --exact-steps 0 --unpad-steps 0 > gpurun_out/bench_b16.log 2>&1
      for prec in bf16 fp8; do
        timeout 500 python bench.py --model ViT-H-14 --batch 2048 --precision $prec --steps 2 --warmup 1 --no-cpu-baseline --h2d-steps 0 --plain-steps 0 --exact-steps 0 --unpad-steps 0 --shapes > gpurun_out/bench_h14_$prec.log 2>&1
      done
      timeout 400 python bench.py --model ViT-L-16 --image-size 84 $BENCHQ --exact-steps 0 --unpad-steps 0 > gpurun_out/bench_l16_84.log 2>&1
      grep -ah "^{" gpurun_out/bench_b16.log gpurun_out/bench_h14_bf16.log gpurun_out/bench_h14_fp8.log gpurun_out/bench_l16_84.log | cut -c1-400 ;;
    stats)
      # rocprofv3 kernel trace of the FINAL binary under the AUTO plan (VERDICT r4 missing #5): summary only travels back
      (cd /tmp && timeout 900 rocprofv3 --kernel-trace --stats -d "$R/gpurun_out/prof" -o r05 -- python "$R/bench.py" --steps 3 --warmup 1 --no-cpu-baseline --h2d-steps 0 --plain-steps 0 --exact-steps 0 --unpad-steps 0 > "$R/gpurun_out/bench_prof.log" 2>&1)
      grep -a "^{" gpurun_out/bench_prof.log | cut -c1-600
      db=$(find gpurun_out/prof -name '*.db' | head -1)
      [ -n "$db" ] && python tools/rocpd_stats.py "$db" > gpurun_out/kernel_stats.csv 2>&1
      head -12 gpurun_out/kernel_stats.csv
      rm -rf gpurun_out/prof ;;      # (only <= 64 MiB of gpurun_out/ travel back: the summaries, not the databases)
    pmcbench)
      # one bench step per counter set, each in its own rocprofv3 pass (MI355X_MICROARCH.md: FETCH_SIZE / WRITE_SIZE never share a
      # pass; no tracing domains next to --pmc), AUTO plan: traffic, MFMA busy + wait states + effective clock, LDS conflicts, L2 hit rate
      mkdir -p gpurun_out/pmcbench
      declare -A SETS=( [FETCH_SIZE]="FETCH_SIZE" [WRITE_SIZE]="WRITE_SIZE"
                        [MFMA]="SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE"
                        [LDS]="SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_LDS_ADDR_CONFLICT SQ_INSTS_LDS SQ_WAIT_INST_LDS SQ_INSTS_VALU SQ_INST_CYCLES_VMEM"
                        [L2]="TCC_HIT_sum TCC_MISS_sum TCC_REQ_sum TCC_EA_RDREQ_sum TCC_EA_WRREQ_sum TCC_EA_WRREQ_STALL_sum" )
      for set in ${PMC_SETS:-FETCH_SIZE WRITE_SIZE MFMA LDS L2}; do
        (cd /tmp && timeout 400 rocprofv3 --pmc ${SETS[$set]} -d "$R/gpurun_out/pmcbench/$set" -o pmc -- \
           python "$R/bench.py" --steps 1 --warmup 0 --no-cpu-baseline --h2d-steps 0 --plain-steps 0 --exact-steps 0 --unpad-steps 0 ${PMC_BENCH_ARGS:-} > "$R/gpurun_out/pmcbench/$set.log" 2>&1)
        tail -2 "$R/gpurun_out/pmcbench/$set.log" | cut -c1-300
      done
      python tools/pmc_summary.py gpurun_out/pmcbench gemm attn ln_ > gpurun_out/pmcbench_summary.txt 2>&1
      find gpurun_out/pmcbench -name '*.db' -delete ;;
    *) echo "unknown stage $s" ;;
  esac
done
ls -la gpurun_out | tail -30
