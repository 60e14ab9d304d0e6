#!/bin/bash
# Builds one variant of the engine into variants/<name>.so (git-ignored, travels with gpurun): tools/build_variant.sh <name> [extra hipcc flags]
# A copy of the sources is built by their own Makefile in a scratch directory: no unit or per-file flag is repeated here, and the product build in
# rust-pathtracer_amd/csrc is left alone.  VARIANT_SHADOW_FLAGS, VARIANT_SHADE_FLAGS, VARIANT_SHADE_NT and VARIANT_EXTEND_FLAGS, where set (empty counts),
# replace the Makefile's SHADOW_FLAGS, SHADE_FLAGS, SHADE_NT and EXTEND_FLAGS.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd); name=${1:?usage: build_variant.sh <name> [extra hipcc flags]}; shift
WORK=${TMPDIR:-/tmp}/pt_variant_$name; CSRC=$WORK/rust-pathtracer_amd/csrc
rm -rf $WORK; mkdir -p $WORK/rust-pathtracer_amd $ROOT/variants
cp -r $ROOT/include $WORK/include; cp -r $ROOT/rust-pathtracer_amd/csrc $CSRC   # (the sources include ../../include by relative path)
make -s -C $CSRC clean   # the product's objects came along: they were built with its flags
overrides=()
for v in SHADOW_FLAGS SHADE_FLAGS SHADE_NT EXTEND_FLAGS; do var=VARIANT_$v; [ -z "${!var+set}" ] || overrides+=("$v=${!var}"); done
make -C $CSRC -j16 libptamd.so EXTRA="$*" "${overrides[@]}"
cp $CSRC/libptamd.so $ROOT/variants/$name.so
echo built variants/$name.so
