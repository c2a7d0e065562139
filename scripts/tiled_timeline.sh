#!/bin/bash
# wave timeline of search_tiled_kernel (as scripts/fused_timeline.sh): profiling build, bench workload mref50 by default
set -e
cd "$(dirname "$0")/.."
mkdir -p gpurun_out
python3 -m cryo_ralib_amd.build -DRALIGN_PROFILE_SWITCHES -o $_/libralign_prof.so      # $_: the directory made above
RALIGN_LIB=$PWD/gpurun_out/libralign_prof.so RALIGN_TIMELINE=$PWD/gpurun_out/tiled_timeline.bin \
    python bench.py --workload ${1:-mref50} --steps 1 --warmup 0 --particles 7000 --no-cpu-baseline --no-parity --no-pcie --function none > gpurun_out/tiled_timeline.log 2>&1
python scripts/tiled_timeline.py gpurun_out/tiled_timeline.bin
