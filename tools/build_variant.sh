#!/bin/bash
# usage: tools/build_variant.sh <name> "<extra hipcc flags>" [source dir]  -> ab/libhybkf_<name>.so built from the working tree, or from the csrc/ of
# another checkout (a worktree of the parent commit) given as third argument (A/B runs on ONE gpu box:
# boxes differ by up to ~15 %, so two variants are only comparable inside one gpurun call: KF_LIB=$PWD/ab/libhybkf_<name>.so)
set -e
cd "$(dirname "$0")/.."
name=$1; flags=$2; src=${3:-hybkinectfu_amd/csrc}; inc=${3:+$3/../../include}; inc=${inc:-include}
mkdir -p ab/obj_$name
pids=()
srcs=$(make -C hybkinectfu_amd/csrc -pn 2>/dev/null | sed -n 's/^SRCS := //p' | head -1)   # this tree's list, as tools/device_listing_sha.sh takes it
for f in $srcs; do
  f=${f%.hip}
  [ -f $src/$f.hip ] || continue                              # (an older checkout has fewer translation units)
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fno-slp-vectorize -fPIC -std=c++17 -Wno-unused-value -I$inc $flags -c $src/$f.hip -o ab/obj_$name/$f.o &
  pids+=($!)
done
for p in "${pids[@]}"; do wait $p; done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ab/libhybkf_$name.so ab/obj_$name/*.o
echo built ab/libhybkf_$name.so
