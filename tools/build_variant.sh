#!/bin/bash
# libsnpgpu variant with extra -D flags for ONE translation unit (timing ablations):
#   tools/build_variant.sh <name> <flags...> [<unit>.hip]        (default unit: kernels_syrk_uv.hip)
#   -> snprelate_amd/libsnpgpu_<name>.so (use with SNPGPU_LIB / tools/bench_lib.sh)
# The unit is rebuilt with the Makefile's flags plus <flags>; every other object of csrc/ is linked as the last `make` left it.
set -e
name=$1; shift
unit=kernels_syrk_uv.hip
flags=()
for a in "$@"; do case "$a" in *.hip) unit=$a ;; *) flags+=("$a") ;; esac; done
cd "$(dirname "$0")/../snprelate_amd/csrc"
make -s
tmp=$(mktemp -d); trap 'rm -rf "$tmp"' EXIT
/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wall -Wno-unused-function "${flags[@]}" -c "$unit" -o "$tmp/variant.o"
others=$(ls *.o | grep -v "^${unit%.hip}\.o$")
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ../libsnpgpu_$name.so $others "$tmp/variant.o" -L/opt/rocm/lib -lhipsolver -lrocblas -ldl
echo built libsnpgpu_$name.so
