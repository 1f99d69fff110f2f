#!/bin/bash
# Counter passes of the hot kernels: separate rocprofv3 --pmc runs of the SAME bench command (counters do
# not mix with other trace domains; FETCH_SIZE and WRITE_SIZE do not fit one pass), summarised per kernel into $OUT/*.json by
# tools/pmc_summary.py / tools/pmc_traffic.py.
# Usage: tools/pmc_collect.sh <out dir> [commit] [pass ...]      passes: fetch write sq lds (default: all four)
#   PMC_PASS_TIMEOUT=<seconds> per pass (default 900): size it from one timed plain run of the bench command below.
# The script stops at the first pass that fails or runs into its time limit: nothing more is started on the GPU after that.
set -u
OUT=${1:-gpurun_out/pmc}
COMMIT=${2:-unknown}
shift $(( $# < 2 ? $# : 2 ))
PASSES=${*:-fetch write sq lds}
LIMIT=${PMC_PASS_TIMEOUT:-900}
mkdir -p "$OUT"
export TMPDIR=/tmp
ROOT=$(cd "$(dirname "$0")/.." && pwd)
CMD="python $ROOT/bench.py --steps 5 --warmup 1 --full --no-cpu-baseline --no-api-e2e --no-costmap --no-telemetry --no-ka-points"
CS=$ROOT/pixel-perfect-sfm_amd/csrc
# (pmc_summary.py and pmc_traffic.py match kernel names by substring)
KERNELS="ba_eval_kernel ka_solve_kernel k_schur_lds k_inner_gram_packed k_gram_build k_gram_eval k_jac k_img k_point k_chol_step"
counters() {
  case $1 in
    fetch) echo FETCH_SIZE ;;
    write) echo WRITE_SIZE ;;
    sq) echo SQ_INSTS_VALU SQ_WAIT_INST_ANY SQ_WAVE_CYCLES SQ_ACTIVE_INST_VALU SQ_WAVES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_ACTIVE_INST_ANY ;;
    lds) echo SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_INSTS_LDS SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_INSTS_SALU TCC_HIT_sum TCC_MISS_sum ;;
    *) return 1 ;;
  esac
}
has_pass() { case " $PASSES " in *" $1 "*) return 0 ;; *) return 1 ;; esac; }
for name in $PASSES; do
  ctrs=$(counters "$name") || { echo "unknown pass '$name' (fetch write sq lds)" >&2; exit 2; }
  rm -rf "/tmp/pmc_$name"
  ( cd /tmp && timeout -k 10 "$LIMIT" rocprofv3 --pmc $ctrs --kernel-trace --output-format csv -d "/tmp/pmc_$name" -- $CMD \
      > "$ROOT/$OUT/$name.stdout" 2> "$ROOT/$OUT/$name.stderr" )
  rc=$?
  echo "pass $name rc=$rc" >> "$ROOT/$OUT/passes.log"
  if [ $rc -ne 0 ]; then
    echo "pass $name exited with status $rc (see $OUT/$name.stderr): stopping" >&2
    exit $rc
  fi
  for k in $KERNELS; do
    python "$ROOT/tools/pmc_summary.py" "/tmp/pmc_$name" $k "$ROOT/$OUT/${name}_$k.json" > /dev/null 2>> "$ROOT/$OUT/passes.log" \
      || echo "summary of $k in pass $name failed" >> "$ROOT/$OUT/passes.log"
  done
done
if has_pass fetch && has_pass write; then
  traffic() {   # per-kernel traffic from the two passes; a failure is logged and fails the script at the end
    python "$ROOT/tools/pmc_traffic.py" /tmp/pmc_fetch /tmp/pmc_write "$@" > /dev/null 2>> "$ROOT/$OUT/passes.log" && return 0
    echo "pmc_traffic.py $3 failed" >> "$ROOT/$OUT/passes.log"; failed=1
  }
  failed=0
  # roofline.traffic of the dominant kernel (with-Jacobian instantiation), stamped with the commit it was measured at
  traffic ba_eval_kernelIDF16_Li128ELb1ELb0 "$ROOT/$OUT/ba_eval_pmc.json" "$CMD" "$COMMIT" $CS/pxr_ba_eval.hip $CS/pxr_interp.h $CS/pxr_device.h
  PMC_PER_KERNEL=ka_order_kernel traffic ka_solve_kernel "$ROOT/$OUT/ka_solve_kernel_traffic.json" "$CMD" "$COMMIT" $CS/pxr_ka.hip $CS/pxr_interp.h $CS/pxr_device.h
  for k in k_schur_lds k_inner_gram_packed k_gram_build k_gram_eval; do
    traffic $k "$ROOT/$OUT/${k}_traffic.json" "$CMD" "$COMMIT"
  done
  [ $failed -eq 0 ] || { echo "a traffic summary failed (see $OUT/passes.log)" >&2; exit 1; }
fi
rm -f "$ROOT/$OUT"/*.stdout
