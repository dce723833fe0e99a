#!/bin/bash
# Build the working tree as an experimental variant library, through the Makefile:
#   tools/build_variant.sh <name> [extra hipcc flags...]   -> mc-path-tracer_amd/libmcpt_<name>.so
set -e
name=$1; shift
root=$(cd "$(dirname "$0")/.." && pwd)
pkg=mc-path-tracer_amd
make -C "$root" -j"${MAX_JOBS:-16}" "$pkg/libmcpt_$name.so" LIB="mcpt_$name" BUILD="$pkg/build_$name" EXTRA_HIPFLAGS="$*"
rm -rf "$root/$pkg/build_$name"
