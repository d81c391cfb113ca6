#!/bin/bash
# Host-only build of the elementwise op table and its driver:  tests/host_ew/build.sh OUT [CSRC_DIR]
# (CSRC_DIR: another tree's csrc to take ew_math.cuh / ew_apply.cuh from; this tree's by default.  A tree from before
# hb_digamma's step bound has no trip hook: the driver then times each call instead, see driver.cpp.)
set -e
here=$(cd "$(dirname "$0")" && pwd)
root=$(cd "$here/../.." && pwd)
csrc=${2:-$root/henbun_amd/csrc}
HIPCC=${HIPCC:-$(command -v hipcc || echo /opt/rocm/bin/hipcc)}
$HIPCC --offload-host-only -x c++ -std=c++17 -O1 -ffp-contract=off -Wno-unused-value -I"$csrc" -I"$here" "$here/driver.cpp" -o "$1"
