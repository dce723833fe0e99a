#!/bin/bash
# Build the library of a git revision as an A/B variant: tools/build_rev_variant.sh <name> [rev]
# -> mc-path-tracer_amd/libmcpt_<name>.so (rev defaults to HEAD; the working tree is untouched).
exec "$(dirname "$0")/build_rev.sh" "$1" "${2:-HEAD}"
