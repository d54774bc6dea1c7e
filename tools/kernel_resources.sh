#!/bin/bash
# usage: tools/kernel_resources.sh [extra hipcc flags] — VGPRs / scratch / spills / occupancy / LDS of every kernel of kernels.hip, denoise.hip,
# adaptive.hip, exposure.hip, bloom.hip, matte.hip, selection.hip, film.hip, view.hip and camera_lists.hip as the Makefile compiles them (LLVM's kernel-resource-usage remarks; no GPU needed)
cd "$(dirname "$0")/../platinum_amd/csrc"
tmp=$(mktemp -d)
trap 'rm -rf "$tmp"' EXIT
for f in kernels denoise adaptive exposure bloom matte selection film view camera_lists; do
  licm=""
  [ "$f" = kernels ] && licm="-mllvm -disable-machine-licm"   # (the Makefile's rule for kernels.o)
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off $licm -Rpass-analysis=kernel-resource-usage "$@" -c $f.hip -o "$tmp/$f.o" > "$tmp/$f.log" 2>&1 &
done
wait
cat "$tmp"/*.log |
  awk '/remark: Function Name:/ {name=$5} /remark:     VGPRs:/ {v=$4} /ScratchSize/ {s=$5} /Occupancy/ {o=$5} /VGPRs Spill/ {sp=$5} /LDS Size/ {print name, "VGPRs", v, "scratch", s, "spill", sp, "occ", o, "LDS", $6}' | c++filt | sed -e 's/pt:://g' -e 's/(.*)//' | sort -u
