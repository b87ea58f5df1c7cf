#!/bin/bash
# The job code's launch sequence on the CPU: builds the host side of CSRC's api.hip (+ job.hip where it exists) against stand-ins for the HIP runtime and for every
# kernel launcher (mock.cpp; the launchers' bodies are generated from CSRC's sfa_internal.h by gen.py), runs driver.cpp's 768 parameter combinations through the
# C-ABI and writes the log of every launch with its arguments, every copy, memset, event and synchronisation to OUT.  Two trees issue the same sequence when their
# logs are the same file:   tools/launch_log/run.sh <csrc of tree A> a.txt && tools/launch_log/run.sh <csrc of tree B> b.txt && cmp a.txt b.txt && cmp a.txt.stderr b.txt.stderr
# No GPU is needed or used; it says nothing about the kernels.
set -e
CSRC=$(cd "$1" && pwd); OUT=$(realpath "$2"); HERE=$(cd "$(dirname "$0")" && pwd)
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
B=$(mktemp -d); trap 'rm -rf "$B"' EXIT
FLAGS="--offload-arch=gfx950 --offload-host-only -fPIE -O1 -std=c++17 -ffp-contract=off -Wno-unused-function"
python3 "$HERE/gen.py" "$CSRC/sfa_internal.h" > "$B/launchers.inc"
objs=""
for s in api.hip job.hip; do [ -f "$CSRC/$s" ] || continue; $HIPCC $FLAGS -c "$CSRC/$s" -o "$B/${s%.hip}.o"; objs="$objs $B/${s%.hip}.o"; done
$HIPCC $FLAGS -x hip -I"$CSRC" -I"$B" -c "$HERE/mock.cpp" -o "$B/mock.o"
$HIPCC $FLAGS -x hip -I"$CSRC/../../include" -c "$HERE/driver.cpp" -o "$B/driver.o"
${CXX:-c++} -o "$B/run" "$B/driver.o" "$B/mock.o" $objs
"$B/run" > "$OUT" 2> "$OUT.stderr"     # (stderr: the SFA_DEBUG_ACTIVE lines; compare it too)
grep -c "^====" "$OUT"
