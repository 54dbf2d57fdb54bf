#!/bin/bash
# A/B runs of bench.py: bash tools/ab.sh "<cfg>" "<cfg>" ...   ("-" = defaults).  A cfg is a list of words: NAME=VALUE with an
# upper-case name is an environment variable (DUDF_LIB=dbg/libdudf_x.so: another build), a lower-case one a library option
# (bench.py --opt stash=7; include/dudf_hip.h lists them).
# prints ms/step and every MFMA kernel's launch time per configuration.  Extra bench flags through AB_FLAGS; the JSON lines and
# stderr of every run go to $AB_OUT (default: ab_out/ in the repository).
R=${GRAFT_REPO_ROOT:-$(cd "$(dirname "$0")/.." && pwd)}
O=${AB_OUT:-$R/ab_out}
mkdir -p "$O"
i=0
for cfg in "$@"; do
  i=$((i+1))
  [ "$cfg" = "-" ] && cfg=""
  envs=""; opts=""
  for w in $cfg; do case "$w" in [A-Z]*) envs="$envs $w";; *) opts="$opts --opt $w";; esac; done
  env $envs python3 "$R/bench.py" --steps ${AB_STEPS:-40} --warmup 5 --full --no-cpu-baseline $opts $AB_FLAGS > "$O/ab_$i.json" 2>"$O/ab_$i.err"
  python3 - "$O/ab_$i.json" "$cfg" <<'PY'
import json, sys
try:
    d = json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
    k = d["roofline"]["all_mfma_kernels"]
    print("[%s]" % sys.argv[2], "ms/step %.3f" % d["ms_per_step"], "pts/s %.2fM" % (d["value"] / 1e6),
          {n.replace("sweep_", "").replace("wgrad_", "wg_"): round(k[n]["avg_ms"], 3) for n in k}, "loss %.3f" % d["final_loss"])
except Exception as e:
    print("[%s] FAILED" % sys.argv[2], e)
PY
done
