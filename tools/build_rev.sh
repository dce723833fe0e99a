#!/bin/bash
# Build the product library of a git revision, through that revision's own Makefile (A/B baselines):
#   tools/build_rev.sh <name> <rev> [extra hipcc flags...]   -> mc-path-tracer_amd/libmcpt_<name>.so
# The working tree is untouched.  (Extra flags reach revisions whose Makefile has EXTRA_HIPFLAGS.)
set -e
name=$1; rev=$2; shift 2
root=$(cd "$(dirname "$0")/.." && pwd)
pkg=mc-path-tracer_amd
wt=$(mktemp -d "${TMPDIR:-/tmp}/mcpt_rev.XXXXXX")
git -C "$root" worktree add -f --detach "$wt" "$rev" > /dev/null
trap 'git -C "$root" worktree remove --force "$wt" 2>/dev/null || rm -rf "$wt"' EXIT
make -C "$wt" -j"${MAX_JOBS:-16}" "$pkg/libmcpt.so" EXTRA_HIPFLAGS="$*"
cp "$wt/$pkg/libmcpt.so" "$root/$pkg/libmcpt_$name.so"
