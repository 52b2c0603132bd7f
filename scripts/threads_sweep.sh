#!/bin/bash
# Host threads x who decides x library variant on the GPU box (developer tool).
#   scripts/threads_sweep.sh "steps warmup" "lib:threads:mode ..."
#   lib = base | <name> (build/<name>.so);  mode = host (bench.py --accept host: the host's threads
#   decide, a launch per step) | dev (--accept kernel: the move kernel decides, one launch of a group
#   in flight)
R=${GRAFT_REPO_ROOT:-$(cd "$(dirname "$0")/.." && pwd)}
mkdir -p $R/gpurun_out/tsweep
set -- $1 "$2"
STEPS=$1; WARM=$2; shift 2
for spec in $1; do
  IFS=: read lib th mode <<< "$spec"
  if [ "$lib" = base ]; then unset MMC_HIP_LIB; else export MMC_HIP_LIB=$R/build/$lib.so; fi
  case "$mode" in host) accept=host;; dev) accept=kernel;; *) echo "$spec: mode is host or dev"; exit 1;; esac
  f=$R/gpurun_out/tsweep/${lib}_${th}_${mode}_s$STEPS
  timeout -k 10 300 python3 $R/bench.py --no-cpu --no-secondary --steps $STEPS --warmup $WARM --threads $th \
      --accept $accept > $f.json 2> $f.err || { echo "$spec FAILED"; tail -5 $f.err; exit 1; }
  python3 -c "import json;d=json.load(open('$f.json'));r=d['roofline'];print('%-22s steps %4d  value %.4e  cost/launch %.1f us  span %.1f us  acc %.4f'%('$spec',$STEPS,d['value'],r.get('avg_launch_us',0),r.get('launch_span_us') or 0,d['acceptance']))"
done
