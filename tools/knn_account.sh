#!/bin/bash
# Accounting build of the k-NN query (SG_KNN_ACCOUNT: per-point counters) -> build/dbg/libsings_hip_knnacct.so, then
# tools/knn_account.py prints what a point costs.  bash tools/knn_account.sh  (on the GPU box; `build`: the library only)
# The same sources and flags as the product (sings_amd/csrc/Makefile), sg_knn.hip with -DSG_KNN_ACCOUNT, objects under build/dbg.
set -e
cd "$(dirname "$0")/.."
make -C sings_amd/csrc -j8 OBJDIR=../../build/dbg LIB=../../build/dbg/libsings_hip_knnacct.so FLAGS_sg_knn=-DSG_KNN_ACCOUNT
[ "$1" = "build" ] || SINGS_HIP_LIB=$PWD/build/dbg/libsings_hip_knnacct.so python3 tools/knn_account.py
