#!/bin/bash
# usage: tools/build_variant.sh <name> <extra hipcc flags...>  -> build/ab/libmvrt_<name>.so (A/B builds; load with MVRT_LIB=...)
# built with -DMVRT_EXPERIMENT: the tuning constants of the product (mvrtKnob) can then be overridden from the environment
name=$1; shift
d=build/ab/$name; mkdir -p $d
F="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -fvisibility=hidden -fno-gpu-rdc -Wno-unused-result -DMVRT_EXPERIMENT $@"
S=$(python3 -c "import sys; sys.path.insert(0, 'massivevoxelraytracing_amd'); import build; print(' '.join(s[:-4] for s in build.SOURCES))") # the library's own list
for s in $S; do
  if [ $s = kernels_rt ] || [ ! -f $d/$s.o ]; then /opt/rocm/bin/hipcc $F -c massivevoxelraytracing_amd/csrc/$s.hip -o $d/$s.o & fi
done
wait
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o build/ab/libmvrt_$name.so $(for s in $S; do echo $d/$s.o; done) && echo built build/ab/libmvrt_$name.so
