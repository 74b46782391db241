#!/bin/bash
# The gate in front of every kernel commit (round 5 validated kernel commits with the bench, which cannot see a 1e-3
# error): the FULL oracle suite on the GPU + run-to-run bit stability of every instantiation.  Runs on the GPU box:
#     gpurun --timeout 2400 -- 'bash tools/gate.sh [label]'
# and leaves gpurun_out/gate_<label>.txt (copy it to profiles/ with the commit it gates).
cd "$(dirname "$0")/.." || exit 1
LABEL=${1:-$(date +%H%M)}
OUT=gpurun_out/gate_$LABEL.txt; mkdir -p gpurun_out
{
  echo "gate $LABEL: $(python -c 'from surfd_amd import _native as N; print(N.lib().surfd_build_config().decode())' 2>&1 | tail -1)"
  echo "sha256 of the kernel sources:"; sha256sum surfd_amd/csrc/*.hip surfd_amd/csrc/*.h surfd_amd/csrc/*.cpp | cut -c1-16,65-
  echo "== pytest -m gpu (full suite)"
  timeout -k 10 2400 python -m pytest tests -m gpu -q 2>&1 | tail -25
  RC=${PIPESTATUS[0]}
  echo "pytest rc=$RC"
  # a step that died (abort, segmentation fault, time limit: any status but 0 / 1) ends the gate: nothing more is started on that GPU
  STEP=${OUT%.txt}.step
  step() { [ "$RC" -le 1 ] || return; timeout -k 10 300 "$@" > $STEP 2>&1; RC=$?; [ "$RC" -le 1 ] || echo "rc=$RC from: $* -- gate stopped"; }
  echo "== determinism_check: 40 evaluations of one input, every form"
  for c in "8 0" "80 80" "160 160"; do step python tools/determinism_check.py 40 $c && grep -E "distinct|differs" $STEP; done
  for c in "80 64 32" "40 64 80"; do step python tools/diag_l64.py $c && grep -E '^\{' $STEP | cut -c1-330; done
  rm -f $STEP
} > $OUT 2>&1
cat $OUT
