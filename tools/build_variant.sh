#!/bin/bash
# tools/build_variant.sh <name> [extra hipcc flags]: another build of the library for tools/ab.sh -> tools/_build/ab_<name>.so (never the
# package directory), by the product's own recipe (__graft_entry__.build_library: same units, same flags) plus -DFR_AB: the experiment rig
# of csrc/fr_rig.inc (the host switches of FR_DEBUG_MODE and the FR_GV / FR_VC / FR_GROUPS / FR_TILE_PRIO / FR_PART_MIN / FR_SPLIT_BLOCKS /
# FR_PART_BLOCKS knobs); add -UFR_AB for a variant of the plain product code.
# (-DFR_LOOPSTATS and -DFR_ABLATE builds read FR_LOOPSTATS_MODE / FR_ABLATE_MODE: tools/loopstats.py, tools/fe_ablate.py.)
name=$1; shift
cd "$(dirname "$0")/.." || exit 1
python -c 'import sys, __graft_entry__ as g; g.build_library(sys.argv[1], ["-DFR_AB"] + sys.argv[2:])' "tools/_build/ab_$name.so" "$@" \
    && ls -la "tools/_build/ab_$name.so"
