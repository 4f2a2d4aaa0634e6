#!/bin/bash
# HERE (build container): a second library with direct binning compiled out, next to the real one, for same-box A/B runs:
#   bash tools/ab_direct.sh build     -> sings_amd/libsings_hip_nodirect.so (git-ignored, travels with gpurun)
# On the GPU box:  SINGS_HIP_LIB=$PWD/sings_amd/libsings_hip_nodirect.so python bench.py ...   against   python bench.py ...
# The same sources and flags as the product (sings_amd/csrc/Makefile) plus -DSG_NO_DIRECT, objects under build/nodirect.
set -e
cd "$(dirname "$0")/.."
make -C sings_amd/csrc -j8 OBJDIR=../../build/nodirect LIB=../libsings_hip_nodirect.so XFLAGS=-DSG_NO_DIRECT
ls -la sings_amd/libsings_hip_nodirect.so
