#!/bin/bash
# Host-only build of the noise generator and its driver:  tests/host_rng/build.sh OUT [CSRC_DIR]
# (CSRC_DIR: another tree's csrc to take rng_core.cuh / rng_seed.cuh from; this tree's by default.)
set -e
here=$(cd "$(dirname "$0")" && pwd)
root=$(cd "$here/../.." && pwd)
csrc=${2:-$root/henbun_amd/csrc}
HIPCC=${HIPCC:-$(command -v hipcc || echo /opt/rocm/bin/hipcc)}
$HIPCC --offload-host-only -x c++ -std=c++17 -O1 -ffp-contract=off -I"$csrc" -I"$here" "$here/driver.cpp" -o "$1"
