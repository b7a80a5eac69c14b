#!/bin/bash
# build a variant of libdevias_amd.so into tools/exp/libdevias_amd_<tag>.so with extra -D flags on the GEMM units (devias_amd/build.py: GEMM_SOURCES) only: tools/build_variant.sh <tag> <flags...>
set -e
cd "$(dirname "$0")/.."
tag=$1; shift
FLAGS="--offload-arch=gfx950 -O3 -fPIC -std=c++17 -ffp-contract=fast -Wno-unused-result -fno-gpu-rdc -mllvm -amdgpu-early-inline-all=true -mllvm -amdgpu-mfma-vgpr-form"
gemm=$(python3 -c "from devias_amd import build; print(' '.join(s[:-4] for s in build.GEMM_SOURCES))")
pids=""; vobjs=""
for f in $gemm; do
    /opt/rocm/bin/hipcc $FLAGS "$@" -c devias_amd/csrc/$f.hip -o tools/exp/${f}_$tag.o & pids="$pids $!"
    vobjs="$vobjs tools/exp/${f}_$tag.o"
done
for p in $pids; do wait $p; done
objs=""
for f in $(python3 -c "from devias_amd import build; print(' '.join(s[:-4] for s in build.SOURCES if s not in build.GEMM_SOURCES))"); do objs="$objs devias_amd/csrc/$f.o"; done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o tools/exp/libdevias_amd_$tag.so $vobjs $objs
rm -f $vobjs
echo built tools/exp/libdevias_amd_$tag.so
