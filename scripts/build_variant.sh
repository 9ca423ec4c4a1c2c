#!/bin/bash
# Build an A/B variant of the library: scripts/build_variant.sh <suffix> <-DFLAGS...>
# -> promonet_amd/lib/libpromonet_hip_<suffix>.so (select with PROMONET_HIP_LIB).
# The Makefile's objects and per-object flags, plus the flags given here.
# Variants in use:
#   direct   -DPM_UPSAMPLE_ROWS=0 -DPM_SINGLE_ROWS=0   the upsamplers' direct stores
#   rows0    -DPM_OUT_ROWS=0   the Block kernels' direct `out` stores everywhere
#   rowsN    -DPM_OUT_ROWS=N   row stores at the sites of the bits of N: 1 the
#            pair kernel, 2 the skewed whole-Block walk, 4 block3_body (pm_conv.h)
set -e
cd $(dirname $0)/..
SUF=$1; shift
make -j16 OBJ=build/obj_$SUF LIB=promonet_amd/lib/libpromonet_hip_$SUF.so EXTRA="$*"
