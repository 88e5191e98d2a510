#!/bin/bash
# NNEST_STAMP diagnostic build of the quad / solo kernels and the training kernels into tools/ab/lib_STAMP.so (the other objects come
# from the normal build, which has to be there).  The solo kernel's stamps are those of its launch prologue and epilogue
# (tools/stamp_prologue.py); STEPS=1 adds its per-step stamps (tools/stamp_run.py), which slow the loop; VOTE=1 adds the stamps of an
# exact step's vote chain on the relay wave and the first net wave (tools/stamp_solo_vote.py) and builds lib_STAMP.so only.
set -e
cd "$(dirname "$0")/../nnest_amd/csrc"
mkdir -p ../../tools/ab
T=$(mktemp -d)
trap 'rm -rf "$T"' EXIT
HIPCC="/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -fno-gpu-rdc -DNNEST_STAMP"
$HIPCC -c nnest_quad.hip -o "$T/quad_stamp.o"
$HIPCC ${STEPS:+-DNNEST_STAMP_STEPS} ${VOTE:+-DNNEST_STAMP_VOTE} -c nnest_solo.hip -o "$T/solo_stamp.o"
$HIPCC -c nnest_train.hip -o "$T/train_stamp.o"
OTHERS=$(ls *.o | grep -v -x -e nnest_quad.o -e nnest_solo.o -e nnest_train.o)
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ../../tools/ab/lib_STAMP.so $OTHERS "$T/quad_stamp.o" "$T/solo_stamp.o" "$T/train_stamp.o" -lpthread
[ -n "$VOTE" ] && exit 0   # (the vote's stamps are the solo kernel's alone: tools/stamp_solo_vote.py)
# the rows form of the spline training step with its stamps (tools/time_spline_train.py prints them through NNEST_HIP_LIB)
$HIPCC -c nnest_spline_rows.hip -o "$T/rows_stamp.o"
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ../../tools/ab/lib_ROWS_STAMP.so $(ls *.o | grep -v -x nnest_spline_rows.o) "$T/rows_stamp.o" -lpthread
