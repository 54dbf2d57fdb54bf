#!/bin/bash
# decomposition of the p24 step by compiling mechanisms out of the sweeps (wrong results: only the clock is read)
R=${GRAFT_REPO_ROOT:-/root/repo}
AB_FLAGS="--no-config3 --opt stash=7" AB_STEPS=20 bash $R/tools/ab.sh "-" "DUDF_LIB=$R/dbg/libdudf_swdbg1.so" "DUDF_LIB=$R/dbg/libdudf_swdbg2.so" "DUDF_LIB=$R/dbg/libdudf_swdbg3.so" "DUDF_LIB=$R/dbg/libdudf_swdbg4.so"
