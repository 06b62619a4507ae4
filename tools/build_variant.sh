#!/bin/bash
# Builds a variant of the library with extra device-code defines (tuning only):
#   tools/build_variant.sh name -DKC_UP_RU=2 -DKC_UP_HARDWIRE   ->  profiles/ab_libs/name.so   (git-ignored, travels with gpurun)
# Every device unit (.hip) and resize.cpp (which sizes the tiles by kc_internal.hpp's KC_UP_RU) are compiled again with the
# defines; the other objects are those of the last regular build (python -m kanter_core_amd.build), taken by name.  The sources,
# their objects' names and the flags are kanter_core_amd/build.py's.
set -eu
name=$1; shift
R=$(cd "$(dirname "$0")/.." && pwd)
B=$R/kanter_core_amd/csrc/build
T=/tmp/kc_variant_$name
mkdir -p $R/profiles/ab_libs $T
ask() { (cd $R && python3 -c "from kanter_core_amd import build as b; print(' '.join($1))"); }
F=$(ask 'b.FLAGS')
D=$(ask 'b.DEVICE_FLAGS')
objs=$B/jit_texts.o
pids=
for pair in $(ask 's + ":" + b.object_name(s) for s in b.SOURCES'); do
    src=$R/kanter_core_amd/csrc/${pair%%:*}; obj=${pair##*:}
    case $src in
    *.hip) /opt/rocm/bin/hipcc $F $D -x hip "$@" -c $src -o $T/$obj & pids="$pids $!"; objs="$objs $T/$obj" ;;
    */resize.cpp) /opt/rocm/bin/hipcc $F "$@" -c $src -o $T/$obj & pids="$pids $!"; objs="$objs $T/$obj" ;;
    *) objs="$objs $B/$obj" ;;
    esac
done
for p in $pids; do wait $p; done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $R/profiles/ab_libs/$name.so $objs -lz -ldl
echo $R/profiles/ab_libs/$name.so
