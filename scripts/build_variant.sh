#!/bin/bash
# Build an A/B variant of the library: scripts/build_variant.sh <suffix> <-DFLAGS...>
# -> promonet_amd/lib/libpromonet_hip_<suffix>.so (select with PROMONET_HIP_LIB).
# The Makefile's objects and per-object flags, plus the flags given here.
set -e
cd $(dirname $0)/..
SUF=$1; shift
make -j16 OBJ=build/obj_$SUF LIB=promonet_amd/lib/libpromonet_hip_$SUF.so EXTRA="$*"
