#!/bin/bash
# Builds tools/bin/libbasisu_hip_tqprof.so: libbasisu_hip.so with the one-workgroup split kernel instrumented (-DTQ_PROFILE: clock64() deltas of thread 0 per
# phase of a split, summed over all workgroups; tsvq_profile_read). Development aid for tools/tsvq_split_profile.py; never loaded by the product.
set -e
cd "$(dirname "$0")/../basis_universal_amd/csrc"
PROF=../../tools/bin
# The object list, the compile rule and its flags are the Makefile's: the product's objects as they are (built here only where missing or stale), the instrumented
# ones by the same rule into $PROF/obj with the -D added.
OBJS=$(make -s print-objs)
make -j8 $OBJS
INSTRUMENTED="tsvq_kernels.o"
make -j8 OUT=$PROF EXTRA_CXXFLAGS=-DTQ_PROFILE $(for o in $INSTRUMENTED; do echo $PROF/obj/$o; done)
LINK=""
for o in $OBJS; do case " $INSTRUMENTED " in *" $(basename $o) "*) LINK="$LINK $PROF/obj/$(basename $o)";; *) LINK="$LINK $o";; esac; done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $PROF/libbasisu_hip_tqprof.so $LINK
echo built tools/bin/libbasisu_hip_tqprof.so
