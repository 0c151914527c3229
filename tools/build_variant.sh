#!/bin/bash
# Build a variant of libnadm.so into tools/abl/<name>.so:  tools/build_variant.sh <name> [-DFLAG=..]...
# (A/B runs: NADM_LIB=tools/abl/<name>.so python bench.py ...; tools/abl_run.sh runs bench.py against every variant.)
# The compile lines of csrc/build.sh, side by side; no test hooks (nadm_hooks.cpp without the macro).
set -e
name=$1; shift
R=$(cd "$(dirname "$0")/.." && pwd)
src=$R/neural-admixture_amd/csrc
out=$R/tools/abl
tmp=/tmp/abl_$name
mkdir -p $out $tmp
HOST="-O3 -std=c++17 -fPIC -ffp-contract=off -Wall -Wno-unused-function"
FLAGS="--offload-arch=gfx950 $HOST"
objs=""
for u in nadm_genotype_passes nadm_small_kernels nadm_step nadm_gmm_dev nadm_calib nadm_project; do
    hipcc $FLAGS -c $src/$u.hip -o $tmp/$u.o "$@" &
    objs="$objs $tmp/$u.o"
done
for u in nadm_gmm nadm_host_io nadm_layout nadm_hooks; do
    hipcc $HOST -c $src/$u.cpp -o $tmp/$u.o "$@" &
    objs="$objs $tmp/$u.o"
done
wait
hipcc --offload-arch=gfx950 -shared -fPIC -Wl,-soname,libnadm.so -o $out/$name.so $objs -lpthread -ldl
echo "built $out/$name.so"
