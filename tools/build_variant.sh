#!/bin/bash
# Timing experiments: build the library with extra -D flags into gcc_amd/csrc/variants/lib_<name>.so (git-ignored; it travels to
# the GPU box with the snapshot, unlike gpurun_out/).  On the box a script swaps it in for the run only:
#     cp gcc_amd/csrc/libgcc_amd.so /tmp/lib_default.so
#     cp gcc_amd/csrc/variants/lib_<name>.so gcc_amd/csrc/libgcc_amd.so;  python bench.py ...;  cp /tmp/lib_default.so gcc_amd/csrc/libgcc_amd.so
# or passes it to tools/graph_probe.py --lib.  The product never loads anything but gcc_amd/csrc/libgcc_amd.so (_cabi.load).
#   tools/build_variant.sh quad4 -DGCC_POSEMB_QUAD_OCC=4
#   tools/build_variant.sh j4 -DGIN_GATHER_J=4 -DGIN_IN_PER_CU=4
# Knobs: GIN_GATHER_J, GIN_IN_PER_CU, GIN_IN_LDS_W, GIN_DBG_SKIP, GATHER_DBG, GCC_KREP (statistics replicas: 8 / 16) (encoder.hip / encoder_common.h); BWD_GATHER_J, BWD_C_PER_CU
# (encoder_bwd.hip); NCE_DQ_BATCH, GCC_NCE_WGS_DEFAULT (nce.hip; run time: GCC_NCE_WGS); GCC_POSEMB_MID_THREADS, GCC_POSEMB_SMALL_T, GCC_POSEMB_QUAD_OCC, GCC_POSEMB_W48_OCC, GCC_POSEMB_CH_THREADS, GCC_POSEMB_CH_LONGDEG, GCC_POSEMB_CH_NARROW_WANT, GCC_POSEMB_ABLATE_MID / _CHEB / _WAVE (timing only: that eigensolver class returns at once) (posemb.hip).
set -eu
name=$1; shift
cd "$(dirname "$0")/../gcc_amd/csrc"
mkdir -p variants
# the library's sources are the Makefile's (a variant that lacks one of them lacks symbols that gcc_amd/_cabi.py binds)
srcs=$(sed -n 's/^SRCS[[:space:]]*:=[[:space:]]*//p' Makefile)
[ -n "$srcs" ] || { echo "build_variant.sh: no SRCS in gcc_amd/csrc/Makefile" >&2; exit 1; }
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -Wall -Wno-unused-function "$@" -o variants/lib_$name.so $srcs
ls -la variants/lib_$name.so
