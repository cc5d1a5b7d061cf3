#!/bin/bash
# The --full bench line without the parity-mode / CPU legs, and a readable dump of its `variants` block
OUT=${1:-bench_out}; mkdir -p "$OUT"      # where the bench line and its stderr go
python bench.py --full --no-parity-mode --no-cpu-baseline > "$OUT/variants.json" 2> "$OUT/variants.err"; tail -c 400 "$OUT/variants.err"
OUT="$OUT" python - <<'PY'
import json, os
r=json.loads(open(os.path.join(os.environ['OUT'], 'variants.json')).read().strip().splitlines()[-1])
print(r['value'], r['ms_per_step'])
print(json.dumps(r.get('variants'), indent=1)[:3500])
PY
