#!/bin/bash
# Diagnostic only: builds libwcqp variants that differ in the flags given to the kernels
#   tools/build_variant.sh NAME [-Dflag ...]   ->  walking-controllers_amd/csrc/build/diag/libwcqp_NAME.so   (pick it up with WCQP_LIB_PATH)
# WCQP_VARIANT_NO_DIAG=1: without -DWCQP_DIAG_KERNELS (the product's own flags + the ones given)
# The translation units are the Makefile's SRCS: every .hip of them is compiled with the flags, what is left (the host-only files) is the product's.
set -e
name=$1; shift
cd "$(dirname "$0")/../walking-controllers_amd/csrc"
make -s >/dev/null      # NOTE: rebuilds the PRODUCT library from the working tree as well - A/B a source change against a variant built from a stash, not against "the product"
mkdir -p build/diag
diag=-DWCQP_DIAG_KERNELS
[ -n "$WCQP_VARIANT_NO_DIAG" ] && diag=
pids=()
objs=(build/host_WalkingControllers.o)
for src in $(make -s print-srcs); do
  f=${src%.hip}
  if [ "$f" = "$src" ]; then objs+=(build/$src.o); continue; fi
  /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -I../../include -I. $diag "$@" -x hip -c $src -o build/diag/${f}_$name.o &
  pids+=($!)
  objs+=(build/diag/${f}_$name.o)
done
for p in "${pids[@]}"; do wait $p; done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o build/diag/libwcqp_$name.so "${objs[@]}"
echo built build/diag/libwcqp_$name.so
