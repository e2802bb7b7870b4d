#!/bin/bash
# N > 1 code path of bench.py on a one-GPU box: 2 ranks share cuda:0, gloo collectives (development check, not a measurement)
cd "$(dirname "$0")/.."
export O=${VTTS_OUT:-out}; mkdir -p "$O"  # output folder
VTTS_DIST_BACKEND=gloo VTTS_SHARE_GPU=1 timeout 600 python \
  bench.py --gpus 2 --steps 2 --warmup 1 --no-cpu-baseline --no-f32 --full > "$O/dryrun2.json" 2> "$O/dryrun2.err"
echo "rc=$?"; tail -3 "$O/dryrun2.err" | cut -c1-300; python - <<'PY'
import json, os
d=json.loads(open(os.path.join(os.environ['O'], 'dryrun2.json')).read().strip().splitlines()[-1])
print({k:d[k] for k in ('n_gpus','value','ms_per_step')}); print(d.get('pipeline_256'))
PY
