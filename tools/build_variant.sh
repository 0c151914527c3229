#!/bin/bash
# Build a variant of libnadm.so into tools/abl/<name>.so:  tools/build_variant.sh <name> [-DFLAG=..]...
# (A/B runs: NADM_LIB=tools/abl/<name>.so python bench.py ...; tools/abl_run.sh runs bench.py against every variant.)
# csrc/build.sh is the one list of units and flags: this calls it with an output path; no test hooks (nadm_hooks.cpp without the macro).
set -e
name=$1; shift
R=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p "$R/tools/abl"
bash "$R/neural-admixture_amd/csrc/build.sh" -o "$R/tools/abl/$name.so" "$@"
