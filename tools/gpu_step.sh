#!/bin/bash
# Run one GPU step under its own time limit; stop the whole call on a fault.
#   tools/gpu_step.sh <name> <seconds> <cmd...>
# rc 0/1 (pass / ordinary test failure) → continue; anything else (abort 134,
# segfault 139, timeout 124/137, …) → exit 99 so the caller's && chain stops.
name=$1; secs=$2; shift 2
OUT="${LFA_GPU_OUT:-gpu_out}"
mkdir -p "$OUT"
echo "== $name: $*" >> $OUT/steps.log
timeout -k 10 "$secs" "$@" > "$OUT/$name.log" 2>&1
rc=$?
echo "== $name rc=$rc" >> $OUT/steps.log
tail -5 "$OUT/$name.log"
if [ $rc -ne 0 ] && [ $rc -ne 1 ]; then
  echo "STOP: $name exited $rc"; exit 99
fi
exit 0
