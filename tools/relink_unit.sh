#!/bin/bash
# Development: recompile ONE translation unit of the library and relink (the other units' objects
# from the last full build are reused).   tools/relink_unit.sh pre32s|main|post|aux|host [extra hipcc flags]
set -e
R=$(cd $(dirname $0)/.. && pwd); O=$R/build/libbrutus_amd.so.o; mkdir -p $O
fl=""
case $1 in
  pre32s) src=pre32s_unit.hip; fl="-fno-slp-vectorize";;
  main) src=brutus_kernels.hip;;
  post|aux|host) src=$1_unit.hip;;
  *) echo "unknown unit: $1" >&2; exit 2;;
esac
shift
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-value $fl "$@" -c $R/brutus_amd/csrc/$src -o $O/$src.o
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC $O/*.hip.o -o $R/brutus_amd/libbrutus_amd.so
