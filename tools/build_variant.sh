#!/bin/bash
# usage: tools/build_variant.sh <tag> [-DFLAG ...] — libptamd_<tag>.so = the library with every translation unit that sees the layout and
# kernel switches (kernels, denoise, adaptive, renderer: all include pt_layout.h) compiled under extra flags
# (experiments only; select with PTAMD_LIB=platinum_amd/csrc/libptamd_<tag>.so; tools/ab.sh benches them)
set -e
tag=$1; shift
cd "$(dirname "$0")/../platinum_amd/csrc"
make -s all
F="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -Wall -Wno-unused-function -Wno-unused-result"
/opt/rocm/bin/hipcc $F -mllvm -disable-machine-licm "$@" -c kernels.hip -o /tmp/kernels_$tag.o   # same flags as the Makefile's kernels.o
objs=/tmp/kernels_$tag.o
for u in denoise adaptive renderer; do
  /opt/rocm/bin/hipcc $F "$@" -c $u.hip -o /tmp/${u}_$tag.o
  objs="$objs /tmp/${u}_$tag.o"
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o libptamd_$tag.so $objs multi_device.o camera_lists.o exposure.o bloom.o math_probe.o lbvh.o scene_io.o scene_gltf.o scene_image.o scene_jpeg.o -lz -ldl -lpthread
echo built libptamd_$tag.so
