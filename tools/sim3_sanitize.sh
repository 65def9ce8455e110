#!/bin/bash
# AddressSanitizer + UndefinedBehaviorSanitizer over the HOST side of orbm_sim3_hypotheses, on the CPU: the library's translation
# units are compiled with the host code instrumented (device code as usual) and linked into the stand-alone program
# tests/cxx/sim3_host_checks.cpp (its own main: no Python, no preloaded runtime), which is then run.  It covers the argument checks
# and the no-launch paths; without a device the valid call returns ORBX_ERR_NO_DEVICE.  usage: tools/sim3_sanitize.sh
set -e -o pipefail
cd "$(dirname "$0")/.."
OUT=${SANITIZE_OUT:-/tmp/orbx_sim3_sanitize}
mkdir -p "$OUT"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
SAN="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined -Xarch_host -fno-omit-frame-pointer"
FLAGS="--offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -fno-fast-math $SAN"
for f in orbx_extract orbx_stereo orbm_match orbm_search orbm_pose orbm_sim3 fem; do
    $HIPCC $FLAGS -c orb_slam2_e_amd/csrc/$f.hip -o "$OUT/$f.o" &
done
wait
$HIPCC $FLAGS -I include -c tests/cxx/sim3_host_checks.cpp -o "$OUT/sim3_host_checks.o"
$HIPCC --offload-arch=gfx950 -fno-gpu-sanitize -fsanitize=address,undefined "$OUT"/*.o -o "$OUT/sim3_host_checks"
ASAN_OPTIONS=detect_leaks=0:abort_on_error=1 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 "$OUT/sim3_host_checks"
