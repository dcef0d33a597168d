#!/bin/bash
# The transposed (D x H) output written by the chain itself (fused_kernel TRO) under bench.py, as a matrix of
# (label, library variant, environment, bench arguments) runs.
# usage (on the GPU):  bash tools/tro_probe.sh [base] [variant ...]      -> tro_base_probe.txt in the script's output directory
#   base [variants]  row-major, the two-pass path (FDOCT_NO_TRO=1) and the fused store of each library variant
# (The presets of rounds 3 to 6 -- align, cost, d512, final, slack -- compared builds that no longer exist: 32-row tiles, fixed
# rings of 28 / 40 slots, the last-arriver write-out and the store probes.  Their records are profiles/r03_tro_*_probe.txt;
# their source is `git show 9d3e109:tools/tro_probe.sh` and `git show 9d3e109:fdoct_amd/csrc/fdoct_kernels.hip`.)
# Variants are libfdoct_hip_<name>.so built with tools/mkvariant.sh;
# "base" is the shipped library.
root="$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)"
cd "$root" || exit 1
mkdir -p gpurun_out
preset=${1:-base}; [ $# -gt 0 ] && shift
out=gpurun_out/tro_${preset}_probe.txt
: > "$out"
lib() { [ "$1" = base ] && echo "$root/fdoct_amd/libfdoct_hip.so" || echo "$root/fdoct_amd/libfdoct_hip_$1.so"; }
run() {  # label, variant, "ENV=.. ENV2=.." (or -), bench args...
  local label=$1 v=$2 envs=$3; shift 3
  [ "$envs" = - ] && envs=""
  # shellcheck disable=SC2086
  env FDOCT_LIB="$(lib "$v")" $envs python3 bench.py --full --steps ${AB_STEPS:-400} --warmup 20 --no-cpu-baseline --half-chip-steps 0 --sustained-seconds 0 --stage-steps 0 --precise-steps 0 "$@" 2>/dev/null | python3 -c "
import json,sys
for l in sys.stdin:
    if l.startswith('{'):
        d=json.loads(l); p=d.get('power') or {}
        print('%-46s %.1f M A-scans/s  step %.4f ms  frac %.4f  %s W %s MHz  parity %s' % ('$label', d['value']/1e6, d['roofline']['kernel_ms_avg'], d['roofline']['frac'], p.get('package_w_last_half'), p.get('sclk_mhz_avg'), d['parity'].get('worst_db_err_over_tol', d['parity'])))
" | tee -a "$out"
}
T="--layout transposed"
for round in 1 2; do
  case $preset in
    base)
      run "r$round rowmajor base" base -
      run "r$round transposed two-pass" base FDOCT_NO_TRO=1 $T
      for v in "${@:-base}"; do run "r$round transposed fused $v" "$v" - $T; done ;;
    *) echo "unknown preset $preset"; exit 1 ;;
  esac
done
