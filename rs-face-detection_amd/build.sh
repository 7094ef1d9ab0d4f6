#!/bin/bash
# Builds librfd_hip.so for gfx950 (MI355X) in-tree.  hipcc cross-compiles without a GPU.
set -e
HERE="$(cd "$(dirname "$0")" && pwd)"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fvisibility=hidden -Wall -Wno-unused-function"
OBJ="$HERE/build"
mkdir -p "$OBJ"
pids=()
objs=()
for src in "$HERE"/csrc/*.hip; do   # every translation unit of csrc/ is part of the library
  f="$(basename "$src" .hip)"
  objs+=("$OBJ/$f.o")
  if [ ! -f "$OBJ/$f.o" ] || [ "$src" -nt "$OBJ/$f.o" ] || [ -n "$(find "$HERE/csrc" "$HERE/../include" -name '*.h' -newer "$OBJ/$f.o")" ]; then
    $HIPCC $FLAGS -c "$src" -o "$OBJ/$f.o" &
    pids+=($!)
  fi
done
for p in "${pids[@]}"; do wait $p; done
$HIPCC --offload-arch=gfx950 -shared -fPIC -o "$HERE/librfd_hip.so" "${objs[@]}" -ldl
echo "built $HERE/librfd_hip.so"
# compiled-language user of the C ABI through include/rfd.hpp (tests/test_cpp_facade_*.py)
g++ -std=c++17 -O2 -Wall -I"$HERE/../include" "$HERE/../tests/cpp/facade_demo.cpp" -o "$OBJ/facade_demo" -L"$HERE" -lrfd_hip -Wl,-rpath,'$ORIGIN/..' -Wl,-rpath,"$HERE" -Wl,-rpath,/opt/rocm/lib
echo "built $OBJ/facade_demo"
# the gallery's identity calls through include/rfd.hpp (tests/test_gallery_identity_cpp_gpu.py)
g++ -std=c++17 -O2 -Wall -I"$HERE/../include" "$HERE/../tests/cpp/gallery_identity_demo.cpp" -o "$OBJ/gallery_identity_demo" -L"$HERE" -lrfd_hip -Wl,-rpath,'$ORIGIN/..' -Wl,-rpath,"$HERE" -Wl,-rpath,/opt/rocm/lib
echo "built $OBJ/gallery_identity_demo"
# the tracker through include/rfd.hpp (tests/test_tracker_cpp_gpu.py)
g++ -std=c++17 -O2 -Wall -I"$HERE/../include" "$HERE/../tests/cpp/tracker_demo.cpp" -o "$OBJ/tracker_demo" -L"$HERE" -lrfd_hip -Wl,-rpath,'$ORIGIN/..' -Wl,-rpath,"$HERE" -Wl,-rpath,/opt/rocm/lib
echo "built $OBJ/tracker_demo"
# the track identities through include/rfd.hpp (tests/test_track_identity_cpp_gpu.py)
g++ -std=c++17 -O2 -Wall -I"$HERE/../include" "$HERE/../tests/cpp/track_identity_demo.cpp" -o "$OBJ/track_identity_demo" -L"$HERE" -lrfd_hip -Wl,-rpath,'$ORIGIN/..' -Wl,-rpath,"$HERE" -Wl,-rpath,/opt/rocm/lib
echo "built $OBJ/track_identity_demo"
# the track shots through include/rfd.hpp (tests/test_track_shots_cpp_gpu.py)
g++ -std=c++17 -O2 -Wall -I"$HERE/../include" "$HERE/../tests/cpp/track_shots_demo.cpp" -o "$OBJ/track_shots_demo" -L"$HERE" -lrfd_hip -Wl,-rpath,'$ORIGIN/..' -Wl,-rpath,"$HERE" -Wl,-rpath,/opt/rocm/lib
echo "built $OBJ/track_shots_demo"
# the annotation through include/rfd.hpp (tests/test_annotate_cpp_gpu.py)
g++ -std=c++17 -O2 -Wall -I"$HERE/../include" "$HERE/../tests/cpp/annotate_demo.cpp" -o "$OBJ/annotate_demo" -L"$HERE" -lrfd_hip -Wl,-rpath,'$ORIGIN/..' -Wl,-rpath,"$HERE" -Wl,-rpath,/opt/rocm/lib
echo "built $OBJ/annotate_demo"
