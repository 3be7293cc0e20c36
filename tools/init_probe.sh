#!/bin/bash
# Driver of tools/init_probe.py on one MI355X: every GPU step under its own time limit, chained so that the first
# failure ends the script; the four records are then gathered into profiles/init_probe.json.
#   tools/init_probe.sh [OUTDIR]
set -o pipefail
cd "$(dirname "$0")/.." || exit 1
OUT=${1:-out/init_probe}
mkdir -p "$OUT" || exit 1
step() {  # seconds, record, arguments of the probe
    local limit=$1 rec=$2
    shift 2
    timeout -k 10 "$limit" python tools/init_probe.py "$@" > "$OUT/$rec" || { echo "init_probe $* failed or ran out of time" >&2; return 1; }
    tail -c 400 "$OUT/$rec"
}
step 120 time_ns.json time ns &&
step 240 time_c5.json time c5 &&
step 400 trap_1e5.json trap 1e5 96 &&
step 400 trap_1e6.json trap 1e6 10 &&
python tools/init_probe.py merge "$OUT/time_ns.json" "$OUT/time_c5.json" "$OUT/trap_1e5.json" "$OUT/trap_1e6.json"
