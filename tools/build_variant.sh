#!/bin/bash
# builds deltarice_amd/variants/lib_<name>.so with extra -D flags: A/B of kernel variants on one box via DRX_LIB_PATH
# usage: tools/build_variant.sh name -DFOO=1 ...   (from the repository root; the sources are the Makefile's HIP_SRCS)
set -e
name=$1; shift
srcs=$(make -s --no-print-directory print-hip-srcs)
[ -n "$srcs" ] || { echo "build_variant.sh: make print-hip-srcs gave no sources" >&2; exit 1; }
mkdir -p deltarice_amd/variants
/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wall -Wno-unused-function "$@" -shared \
  $srcs -o deltarice_amd/variants/lib_$name.so
