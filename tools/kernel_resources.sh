#!/bin/bash
# usage: tools/kernel_resources.sh [extra hipcc flags] — VGPRs / scratch / spills / occupancy / LDS of every kernel of the device files named in
# `units` as the Makefile compiles them (LLVM's kernel-resource-usage remarks; no GPU needed).  Exits 1 with the compiler's output when a file fails.
units="kernels trace_kernels denoise adaptive exposure bloom matte selection film ao view camera_lists projection sky"
cd "$(dirname "${BASH_SOURCE[0]}")/../platinum_amd/csrc"

# device_compile <unit> <flags...>: the device pass of one unit under the Makefile's flags (HIPFLAGS without the warnings; its rules for kernels.o
# and trace_kernels.o)
device_compile() {
  local unit=$1 licm=""
  shift
  [ "$unit" = kernels ] && licm="-mllvm -disable-machine-licm"
  [ "$unit" = trace_kernels ] && licm="-mllvm -disable-machine-licm -fno-slp-vectorize"
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off $licm --cuda-device-only "$@" "$unit.hip"
}
return 0 2> /dev/null   # sourced (tests/kernel_report.py takes device_compile for a unit's assembly): the definitions alone

tmp=$(mktemp -d)
trap 'rm -rf "$tmp"' EXIT
for f in $units; do
  { device_compile $f -Rpass-analysis=kernel-resource-usage "$@" -c -o "$tmp/$f.o" > "$tmp/$f.log" 2>&1 || mv "$tmp/$f.log" "$tmp/$f.failed"; } &
done
wait
if ls "$tmp"/*.failed > /dev/null 2>&1; then
  cat "$tmp"/*.failed >&2
  exit 1
fi
cat "$tmp"/*.log |
  awk '/remark: Function Name:/ {name=$5} /remark:     VGPRs:/ {v=$4} /ScratchSize/ {s=$5} /Occupancy/ {o=$5} /VGPRs Spill/ {sp=$5} /LDS Size/ {print name, "VGPRs", v, "scratch", s, "spill", sp, "occ", o, "LDS", $6}' | c++filt | sed -e 's/pt:://g' -e 's/(.*)//' | sort -u
