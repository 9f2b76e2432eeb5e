#!/bin/bash
# the library with -DRZ_NET_PROFILE (phase ticks in the trunk kernels) -> profiles/microbench/librlzero_netprof.so
# NETPROF_EXTRA: more flags, e.g. "-DRZ_SEL_TICKS=3" / "-DRZ_SEL_TICKS=28" (the selection's own rows in k_delta_res, two placements) or
# "-DRZ_DELTA_PRESCAN=0" (the selection scans the root itself): profiles/r09/delta_resident_phases.txt; "-DRZ_BKP_TICKS=1": the rows of
# k_delta_res' expand + backup and wave 1's conv2, in the slots of the selection's ticks 1 .. 3 (RZ_SEL_TICKS 0 or 1 beside it)
set -e
cd "$(dirname "$0")/../.."
F="--offload-arch=gfx950 -O3 -ffp-contract=off -fno-fast-math -fno-slp-vectorize -std=c++17 -fPIC -Wno-unused-function -Iinclude"
H=$(python -c "import rlzero_amd._build as b; print(b.source_hash())")
O=$(mktemp -d)
for f in rz_engine rz_net rz_muzero rz_replay rz_mz_replay rz_mz_learn; do
  hipcc $F -DRZ_NET_PROFILE $NETPROF_EXTRA -DRZ_SOURCE_HASH="\"$H\"" -c rlzero_amd/csrc/$f.hip -o $O/$f.o &
done
wait
hipcc --offload-arch=gfx950 -shared -fPIC $O/*.o -o profiles/microbench/librlzero_netprof.so
