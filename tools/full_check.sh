#!/bin/bash
# Round-end style check: the whole GPU suite, smoke(), and the bench line with every secondary
# measurement (--full). Logs go to $OUT (default build/full_check, git-ignored).
set -o pipefail
export TMPDIR=/tmp
OUT=${OUT:-build/full_check}
mkdir -p "$OUT"
timeout -k 10 1000 python -u -m pytest tests -m gpu -q -x -p no:cacheprovider --timeout 300 --timeout-method thread \
  > "$OUT/full_pytest.log" 2>&1
rc=$?; tail -3 "$OUT/full_pytest.log"; [ $rc -eq 0 ] || exit $rc
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > "$OUT/full_smoke.log" 2>&1 || { tail -5 "$OUT/full_smoke.log"; exit 1; }
tail -1 "$OUT/full_smoke.log"
timeout -k 10 600 python bench.py --full > "$OUT/full_bench.json" 2> "$OUT/full_bench.err" || { tail -5 "$OUT/full_bench.err"; exit 1; }
cat "$OUT/full_bench.json"
