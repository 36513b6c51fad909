#!/bin/bash
# Round-6 experiments, one function each; run on the GPU box as
#   bash tools/exp_r6.sh <id>
# Each writes under gpurun_out/r6_<id>/; the committed results are in profiles/r06/.
set -e
cd "$GRAFT_REPO_ROOT"

C5="--width 3840 --height 2160 --frames 128 --threshold 8 --count 12 --nms sad"

# config 5's one-lane regression (0.643 -> 0.71 ms when every lane got its
# own input copy).  Interleaved A/B of (lanes, copies) = (1,1) (1,3) (3,1) (3,3): ms per step
# and per-launch durations, then FETCH_SIZE and TCC hit/miss passes for each (own rocprofv3
# run per counter set, nothing else traced).
exp_c5ab() {
  O=gpurun_out/r6_c5ab
  mkdir -p $O
  : > $O/ab.jsonl
  for r in 1 2 3; do
    for lc in "1 1" "1 3" "3 1" "3 3"; do
      set -- $lc
      timeout -k 10 150 python3 bench.py $C5 --lanes $1 --copies $2 --full --no-extras --no-parity \
          --cpu-seconds 0 --steps 30 --warmup 5 > $O/run.json 2> $O/run.err
      python3 -c "import json,sys; d=json.load(open('$O/run.json')); r=d['roofline']; print(json.dumps({'round': $r, 'lanes': $1, 'copies': $2, 'ms_per_step': d['ms_per_step'], 'kernel_ms_avg': r['kernel_ms_avg'], 'launch_ms_avg': r['launch_ms_avg']}))" >> $O/ab.jsonl
    done
  done
  cat $O/ab.jsonl
  cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
  SHORT="--no-extras --no-parity --cpu-seconds 0 --steps 6 --warmup 1 --settle-seconds 0"
  for lc in "1 1" "1 3" "3 1" "3 3"; do
    set -- $lc
    T=l$1_c$2
    timeout -k 10 150 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $O/fetch_$T -o p -- \
        python3 bench.py $C5 $SHORT --lanes $1 --copies $2 > $O/fetch_$T.json 2> $O/fetch_$T.log
    timeout -k 10 150 rocprofv3 --pmc TCC_HIT_sum TCC_MISS_sum --output-format csv -d $O/tcc_$T -o p -- \
        python3 bench.py $C5 $SHORT --lanes $1 --copies $2 > $O/tcc_$T.json 2> $O/tcc_$T.log
    python3 tools/pmc_summary.py $O/fetch_$T $O/tcc_$T > $O/pmc_$T.json
    rm -rf $O/fetch_$T $O/tcc_$T
  done
  echo c5ab done
}

# Two full-test batches in flight per wave (FDF_BATCH_SLOTS=2: each evaluated 6 rows after its
# issue instead of 3) against the product build: interleaved, 3 rounds, one stream.
exp_slots_ab() {
  O=gpurun_out/r6_slots_ab
  mkdir -p $O
  timeout -k 10 400 bash tools/ab_interleave.sh $O/ab_1080.txt 3 "maxt:0,off:0,sad:0" "" \
      feature_detector_fast_amd/libfdf.so build/libfdf_slots2.so
  timeout -k 10 400 bash tools/ab_interleave.sh $O/ab_4k.txt 3 "sad:0" \
      "--width 3840 --height 2160 --frames 128 --threshold 8 --count 12" \
      feature_detector_fast_amd/libfdf.so build/libfdf_slots2.so
  echo slots_ab done
}

# The headline protocol with and without timestamps on the timed region's own dispatches
# (--inline-timing: rounds 1-5), interleaved, 3 rounds each, no extras.
exp_timing_ab() {
  O=gpurun_out/r6_timing_ab
  mkdir -p $O
  : > $O/ab.jsonl
  for r in 1 2 3; do
    for mode in separate inline; do
      extra=""; [ $mode = inline ] && extra="--inline-timing"
      timeout -k 10 200 python3 bench.py --full --no-extras --no-parity --cpu-seconds 0 $extra > $O/run.json 2> $O/run.err
      python3 -c "import json; d=json.load(open('$O/run.json')); r=d['roofline']; print(json.dumps({'round': $r, 'mode': '$mode', 'value': d['value'], 'ms_per_step': d['ms_per_step'], 'kernel_ms_avg': r['kernel_ms_avg'], 'launch_ms_avg': r['launch_ms_avg']}))" >> $O/ab.jsonl
    done
  done
  cat $O/ab.jsonl
}

# fdf_detect end to end on one 1080p frame (pinned / pageable in and out), 3 rounds
exp_host() {
  O=gpurun_out/r6_host
  mkdir -p $O
  for r in 1 2 3; do
    timeout -k 10 120 python3 tools/host_latency.py --iters 300 --modes off,maxt --mem pinned,pageable --chunks 0 >> $O/host.txt
  done
  cat $O/host.txt
}

# Lane-row byte shifts through LDS instead of v_alignbyte + DPP (FDF_LDS_SHIFT=1: the W flags;
# 2: also the x + 3 row): whole-batch parity of each variant, then the interleaved A/B against
# the product build (1080p three modes, 4K SAD), then VALU / LDS instruction counts.
exp_lds_ab() {
  O=gpurun_out/r6_lds_ab
  mkdir -p $O
  for v in lds1 lds2; do
    FDF_LIB_PATH=build/libfdf_$v.so timeout -k 10 300 python3 -u -m pytest -q --timeout 200 --timeout-method thread \
        tests/test_gpu_stress.py::test_config4_exact_batch tests/test_gpu_geometry.py::test_config5_batch_repeated \
        tests/test_gpu_parity.py > $O/parity_$v.txt 2>&1 || { tail -20 $O/parity_$v.txt; exit 1; }
    tail -1 $O/parity_$v.txt
  done
  timeout -k 10 500 bash tools/ab_interleave.sh $O/ab_1080.txt 3 "maxt:0,off:0,sad:0" "" \
      feature_detector_fast_amd/libfdf.so build/libfdf_lds1.so build/libfdf_lds2.so
  timeout -k 10 400 bash tools/ab_interleave.sh $O/ab_4k.txt 3 "sad:0" \
      "--width 3840 --height 2160 --frames 128 --threshold 8 --count 12" \
      feature_detector_fast_amd/libfdf.so build/libfdf_lds1.so build/libfdf_lds2.so
  echo lds_ab done
}

# The x + 3 row from its own unaligned 16-byte load, 2 steps ahead (FDF_ROW_PLUS3=2), against
# the product build: parity, then the interleaved A/B (1080p three modes, 4K SAD).
exp_p3_ab() {
  O=gpurun_out/r6_p3_ab
  mkdir -p $O
  FDF_LIB_PATH=build/libfdf_p2.so timeout -k 10 300 python3 -u -m pytest -q --timeout 200 --timeout-method thread \
      tests/test_gpu_stress.py::test_config4_exact_batch tests/test_gpu_geometry.py::test_config5_batch_repeated \
      tests/test_gpu_parity.py > $O/parity_p2.txt 2>&1 || { tail -20 $O/parity_p2.txt; exit 1; }
  tail -1 $O/parity_p2.txt
  timeout -k 10 400 bash tools/ab_interleave.sh $O/ab_1080.txt 3 "maxt:0,off:0,sad:0" "" \
      feature_detector_fast_amd/libfdf.so build/libfdf_p2.so
  timeout -k 10 300 bash tools/ab_interleave.sh $O/ab_4k.txt 3 "sad:0" \
      "--width 3840 --height 2160 --frames 128 --threshold 8 --count 12" \
      feature_detector_fast_amd/libfdf.so build/libfdf_p2.so
  echo p3_ab done
}

# Final-tree instruction counts per detector launch (one lane, serialised dispatches): the
# round-5 t25 passes (tools/exp_r5.sh t25_pmcv) into gpurun_out/r6_pmcv.
exp_pmcv() {
  cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
  O=gpurun_out/r6_pmcv
  mkdir -p $O
  SHORT="--steps 6 --warmup 1 --settle-seconds 0 --cpu-seconds 0 --no-extras --no-parity --lanes 1"
  run() {
    local tag=$1; shift
    timeout -k 10 180 rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_VMEM SQ_WAVES \
        --output-format csv -d "$O/$tag" -o p -- python3 bench.py $SHORT "$@" > "$O/$tag.json" 2> "$O/$tag.log"
    python3 tools/pmc_summary.py "$O/$tag" > "$O/${tag}_summary.json"
    rm -rf "$O/$tag"
  }
  run maxt --nms maxt
  run off --nms off
  run sad --nms sad
  run 4k --width 3840 --height 2160 --frames 128 --threshold 8 --count 12 --nms sad
  cat $O/*_summary.json
}

# fdf_detect returning on the launch's completion word (the product) against the runtime's
# completion (FDF_NO_DONE_FLAG build): the host-call tests on the product build, then
# interleaved end-to-end host latency, 3 rounds, pinned and pageable frames.  Measured and not
# kept: the sources it needs are the completion-word commits in git history
# (profiles/r06/t17_host_word_ab/README.txt).
exp_host_word_ab() {
  O=gpurun_out/r6_host_word_ab
  mkdir -p $O
  timeout -k 10 300 python3 -u -m pytest -q --timeout 200 --timeout-method thread \
      tests/test_gpu_host_inplace.py tests/test_gpu_api.py tests/test_gpu_parity.py \
      > $O/tests.txt 2>&1 || { tail -30 $O/tests.txt; exit 1; }
  tail -1 $O/tests.txt
  : > $O/host.txt
  for r in 1 2 3; do
    for lib in feature_detector_fast_amd/libfdf.so build/libfdf_nodone.so; do
      echo "== round $r $lib" >> $O/host.txt
      FDF_LIB_PATH=$lib timeout -k 10 120 python3 tools/host_latency.py --iters 300 \
          --modes off,maxt --mem pinned,pageable --chunks 0 >> $O/host.txt
    done
  done
  cat $O/host.txt
}

# Full-test issue cadence (FDF_ISSUE: a batch every 2 / 3 / 4 rows) at 4K t=8 n=12 SAD, where a
# wave queues ~35 candidates per row (FIFO overflow -> synchronous batches), and at 1080p:
# parity of the 4K batch on each variant, then interleaved A/B (3 rounds, one stream).
exp_issue_ab() {
  O=gpurun_out/r6_issue_ab
  mkdir -p $O
  for v in issue2 issue4; do
    FDF_LIB_PATH=build/libfdf_$v.so timeout -k 10 200 python3 -u -m pytest -q --timeout 150 --timeout-method thread \
        tests/test_gpu_geometry.py::test_config5_batch_repeated > $O/parity_$v.txt 2>&1 || { tail -20 $O/parity_$v.txt; exit 1; }
    tail -1 $O/parity_$v.txt
  done
  timeout -k 10 400 bash tools/ab_interleave.sh $O/ab_4k.txt 3 "sad:0" \
      "--width 3840 --height 2160 --frames 128 --threshold 8 --count 12" \
      feature_detector_fast_amd/libfdf.so build/libfdf_issue2.so build/libfdf_issue4.so
  timeout -k 10 400 bash tools/ab_interleave.sh $O/ab_1080.txt 3 "maxt:0,sad:0" "" \
      feature_detector_fast_amd/libfdf.so build/libfdf_issue2.so build/libfdf_issue4.so
  echo issue_ab done
}

# Candidate FIFO of 512 / 1024 entries per wave (an FDF_PIXEL_Q macro for kSweepPixelQ, 256;
# measured and not kept, the macro is not in the product header): at 4K t=8
# the 256-entry FIFO overflows and its overflow path tests batches synchronously.  Parity on
# the config-5 batch and test_gpu_parity.py, then interleaved A/B at 4K and 1080p.
exp_fifo_ab() {
  O=gpurun_out/r6_fifo_ab
  mkdir -p $O
  for v in q512 q1024; do
    FDF_LIB_PATH=build/libfdf_$v.so timeout -k 10 300 python3 -u -m pytest -q --timeout 200 --timeout-method thread \
        tests/test_gpu_geometry.py::test_config5_batch_repeated tests/test_gpu_stress.py::test_config4_exact_batch \
        tests/test_gpu_parity.py > $O/parity_$v.txt 2>&1 || { tail -20 $O/parity_$v.txt; exit 1; }
    tail -1 $O/parity_$v.txt
  done
  timeout -k 10 400 bash tools/ab_interleave.sh $O/ab_4k.txt 3 "sad:0" \
      "--width 3840 --height 2160 --frames 128 --threshold 8 --count 12" \
      feature_detector_fast_amd/libfdf.so build/libfdf_q512.so build/libfdf_q1024.so
  timeout -k 10 400 bash tools/ab_interleave.sh $O/ab_1080.txt 3 "maxt:0,off:0,sad:0" "" \
      feature_detector_fast_amd/libfdf.so build/libfdf_q512.so build/libfdf_q1024.so
  echo fifo_ab done
}

case "${1:-}" in
  c5ab|slots_ab|timing_ab|host|lds_ab|p3_ab|pmcv|host_word_ab|issue_ab|fifo_ab) "exp_$1" ;;
  *) echo "usage: $0 {c5ab|slots_ab|timing_ab|host|lds_ab|p3_ab|pmcv|host_word_ab|issue_ab|fifo_ab}" >&2; exit 2 ;;
esac
