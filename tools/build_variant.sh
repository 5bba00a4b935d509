#!/bin/bash
# Build a kernel variant from the working tree with one text substitution, applied to whichever of
# the .hip files and bhrt_trace_core.h contain the text:
# tools/build_variant.sh NAME 'python-expression-on-s' -> raytracing-engine-in-c_amd/ab/libbhrt_NAME.so
# e.g. tools/build_variant.sh w5 "s.replace('SPIN0) ? 4', 'SPIN0) ? 5')"
set -e
cd "$(dirname "$0")/.."
NAME=$1; EXPR=$2
T=$(mktemp -d)
mkdir -p "$T/raytracing-engine-in-c_amd" raytracing-engine-in-c_amd/ab
cp -r raytracing-engine-in-c_amd/csrc "$T/raytracing-engine-in-c_amd/"
cp -r include "$T/"
rm -f "$T"/raytracing-engine-in-c_amd/csrc/*.o
python3 - "$EXPR" "$T"/raytracing-engine-in-c_amd/csrc/*.hip \
    "$T/raytracing-engine-in-c_amd/csrc/bhrt_trace_core.h" <<'PY'
import sys
e, changed = sys.argv[1], 0
for p in sys.argv[2:]:
    s = open(p).read()
    t = eval(e)
    if t != s:
        open(p, "w").write(t)
        changed += 1
assert changed, "substitution changed nothing"
PY
make -s -C "$T/raytracing-engine-in-c_amd/csrc" OUT="$PWD/raytracing-engine-in-c_amd/ab/libbhrt_$NAME.so" >/dev/null
rm -rf "$T"
echo "built ab/libbhrt_$NAME.so"
