#!/usr/bin/env bash
# Round-end check on a GPU box (run from the repo root):
#   bash profiles/round_check.sh <tag>
# the whole GPU suite, smoke(), the bench line with every leg (--full), then
# the rocprof passes of run_profile.sh; stops at the first failing step.
# The logs and the bench line land in $NRMS_OUT_DIR (relative to the repo
# root; default: results/), run_profile.sh's passes in its prof_<tag>/ and
# pmc_<tag>_<stage>/ subfolders.
set -euo pipefail
TAG=${1:-r3d}
OUT=${NRMS_OUT_DIR:-results}
mkdir -p "$OUT"
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > "$OUT/${TAG}_gputests.log" 2>&1 \
  || { tail -30 "$OUT/${TAG}_gputests.log"; exit 1; }
tail -2 "$OUT/${TAG}_gputests.log"
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')"
timeout -k 10 600 python bench.py --full > "$OUT/${TAG}_bench.json" 2> "$OUT/${TAG}_bench.err"
cat "$OUT/${TAG}_bench.json"
timeout -k 10 700 bash profiles/run_profile.sh "$TAG" > "$OUT/${TAG}_prof.log" 2>&1
tail -3 "$OUT/${TAG}_prof.log"
