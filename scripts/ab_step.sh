#!/bin/bash
# A/B of the whole bench line (or one part of it) between other builds of libxpbd_hip.so and this one, alternated in one
# GPU job: every run its own process under its own time limit, the job ends at the first failure.  The first library is
# the baseline (the parent commit's build); further ones are variants of this build (one step of a change alone, say),
# and "new" is the library as built.  The result file is rewritten after every round.
# Usage: scripts/ab_step.sh <out.json> <runs> <name>=<libxpbd_hip.so> [<name>=<lib> ...] [-- bench.py arguments after --gpus 1 --steps 20 --warmup 5]
# A build counts as a gain only if its slowest run beats the baseline's fastest.
set -eo pipefail
OUT=$1; RUNS=$2; shift 2
NAMES=(); declare -A LIBS
while [ $# -gt 0 ] && [ "$1" != "--" ]; do NAMES+=("${1%%=*}"); LIBS[${1%%=*}]=${1#*=}; shift; done
[ "$1" = "--" ] && shift
NAMES+=(new)
TMP=$(mktemp -d)
for r in $(seq 1 "$RUNS"); do
  for which in "${NAMES[@]}"; do
    if [ $which = new ]; then unset XPBD_HIP_LIB; else export XPBD_HIP_LIB=${LIBS[$which]}; fi
    timeout -k 10 400 python3 bench.py --gpus 1 --steps 20 --warmup 5 "$@" 2> "$TMP/$which.$r.err" | tail -1 > "$TMP/$which.$r.json"
    echo "$which run $r: $(python3 -c "import json,sys; d=json.load(open('$TMP/$which.$r.json')); print(d['value'], (d.get('roofline') or {}).get('launch_us'))")"
  done
  python3 - "$TMP" "$r" "$*" "${NAMES[@]}" > "$OUT" <<'PY'
import json, statistics, sys
tmp, runs, args, names = sys.argv[1], int(sys.argv[2]), sys.argv[3], sys.argv[4:]
res = {"command": "bench.py --gpus 1 --steps 20 --warmup 5 " + args, "order": ", ".join(names) + ", " + names[0] + ", ...", "baseline": names[0]}
for which in names:
    rows = [json.load(open("%s/%s.%d.json" % (tmp, which, r))) for r in range(1, runs + 1)]
    res[which] = {"metric": rows[0].get("metric"), "values": [r["value"] for r in rows], "median": statistics.median(r["value"] for r in rows),
                  "launch_us": [(r.get("roofline") or {}).get("launch_us") for r in rows]}
    for key in ("roofline_unfused", "roofline_hbm_resident"):            # --full only
        if rows[0].get(key):
            res[which][key] = [r[key]["achieved"] for r in rows]
            res[which][key + "_median"] = statistics.median(res[which][key])
    if which != names[0]:
        res[which]["median_ratio_over_baseline"] = res[which]["median"] / res[names[0]]["median"]
        res[which]["gain_beyond_spread"] = min(res[which]["values"]) > max(res[names[0]]["values"])
        res[which]["loss_beyond_spread"] = max(res[which]["values"]) < min(res[names[0]]["values"])
print(json.dumps(res, indent=1))
PY
done
cat "$OUT"
