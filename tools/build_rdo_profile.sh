#!/bin/bash
# Builds tools/bin/libbasisu_hip_rdoprof.so: libbasisu_hip.so with the RDO strips kernel instrumented (-DRDO_PROFILE: clock64() deltas per phase of
# the serial step, strip 0, printed to stderr by bu_hip_k_uastc_rdo). Development aid for tools/rdo_step_profile.py; never loaded by the product.
set -e
cd "$(dirname "$0")/../basis_universal_amd/csrc"
PROF=../../tools/bin
# The object list, the compile rule and its flags are the Makefile's: the product's objects as they are (built here only where missing or stale), the instrumented
# ones by the same rule into $PROF/obj with the -D added.
OBJS=$(make -s print-objs)
make -j8 $OBJS
INSTRUMENTED="uastc_rdo_kernels.o api_uastc.o"
make -j8 OUT=$PROF EXTRA_CXXFLAGS=-DRDO_PROFILE $(for o in $INSTRUMENTED; do echo $PROF/obj/$o; done)
LINK=""
for o in $OBJS; do case " $INSTRUMENTED " in *" $(basename $o) "*) LINK="$LINK $PROF/obj/$(basename $o)";; *) LINK="$LINK $o";; esac; done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $PROF/libbasisu_hip_rdoprof.so $LINK
echo built tools/bin/libbasisu_hip_rdoprof.so
