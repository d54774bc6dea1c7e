#!/bin/bash
# usage: tools/build_variant.sh <tag> [-DFLAG ...] — libptamd_<tag>.so = the library with every HIP translation unit compiled under extra
# flags: each of them includes pt_layout.h (most through kernels.h), so each sees the layout and kernel switches.  The object list is the
# Makefile's OBJS, so a new file cannot be forgotten here; the host-only scene_*.o are linked as `make` built them.
# (experiments only; select with PTAMD_LIB=platinum_amd/csrc/libptamd_<tag>.so; tools/ab.sh benches them)
set -e
tag=$1; shift
cd "$(dirname "$0")/../platinum_amd/csrc"
make -s all
F="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -Wall -Wno-unused-function -Wno-unused-result"
objs=
for o in $(sed -n 's/^OBJS = //p' Makefile); do
  u=${o%.o}
  if [ -f $u.hip ]; then
    extra=; [ $u = kernels ] && extra="-mllvm -disable-machine-licm"   # same flags as the Makefile's kernels.o
    [ $u = trace_kernels ] && extra="-mllvm -disable-machine-licm -fno-slp-vectorize"   # ... and as its trace_kernels.o
    /opt/rocm/bin/hipcc $F $extra "$@" -c $u.hip -o /tmp/${u}_$tag.o
    o=/tmp/${u}_$tag.o
  fi
  objs="$objs $o"
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o libptamd_$tag.so $objs -lz -ldl -lpthread
echo built libptamd_$tag.so
