#!/bin/bash
# Build the in-tree library and its phase-trace build (the one build-time variant left: tools/scan_trace.py and
# tools/imag_trace.py load it), here in the build container (hipcc cross-compiles gfx950); they travel to the GPU box
# with the tree. Usage: bash tools/build_variants.sh
set -e
cd "$(dirname "$0")/../safe-dreamer_amd/csrc"
make -j8 >/dev/null
make -j8 OUT=../sdreamer/_lib_trace BUILD=build_trace EXTRA=-DSD_SCAN_TRACE >/dev/null
echo "variants built"
