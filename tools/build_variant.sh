#!/bin/bash
# Diagnostic build of the library with extra macros on ONE translation unit (instrumentation; never shipped):
#   tools/build_variant.sh stamps -DRFD_CLOCK_STAMPS        ->  tools/bin/librfd_hip_stamps.so   (load with RFD_HIP_LIB=...)
#   UNIT=network tools/build_variant.sh diag -DRFD_DIAG     (UNIT: the csrc/*.hip file rebuilt; default kernels_conv)
set -e
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
NAME="$1"; shift
PKG="$ROOT/rs-face-detection_amd"
UNIT="${UNIT:-kernels_conv}"
mkdir -p "$ROOT/tools/bin"
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fvisibility=hidden -Wno-unused-function "$@" \
    -c "${SRC:-$PKG/csrc/$UNIT.hip}" -o "$ROOT/tools/bin/${UNIT}_$NAME.o"
OBJS=""
for src in "$PKG"/csrc/*.hip; do
  f="$(basename "$src" .hip)"
  if [ "$f" = "$UNIT" ]; then OBJS="$OBJS $ROOT/tools/bin/${UNIT}_$NAME.o"; else OBJS="$OBJS $PKG/build/$f.o"; fi
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o "$ROOT/tools/bin/librfd_hip_$NAME.so" $OBJS -ldl
rm -f "$ROOT/tools/bin/${UNIT}_$NAME.o"
echo "built tools/bin/librfd_hip_$NAME.so"
