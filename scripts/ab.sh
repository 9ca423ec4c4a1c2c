#!/bin/bash
# On the GPU box: interleaved A/B of library variants (scripts/build_variant.sh),
# 3 rounds each. usage: [AB_FILTER=substr] scripts/ab.sh "" _suffix1 _suffix2 ...
# Every run has a time limit, and the first run that fails ends the script.
set -o pipefail
ROOT=${GRAFT_REPO_ROOT:-$(pwd)}
for round in 1 2 3; do
  for v in "$@"; do
    PROMONET_HIP_LIB=$ROOT/promonet_amd/lib/libpromonet_hip$v.so timeout -k 10 180 python $ROOT/bench.py --full --steps 6 --warmup 2 --sustain 0 --no-cpu-baseline --no-traffic --no-secondary 2>/dev/null | AB_FILTER=$AB_FILTER python -c "
import json,sys,os; r=json.loads(sys.stdin.read()); k=r['kernels']; f=os.environ.get('AB_FILTER','')
print('variant[$v] round $round: %.2f ms | ' % r['ms_per_step'] + ' '.join('%s %.3f' % (n.replace('block_','b').replace('pair_','p'), v['ms_per_step']) for n, v in sorted(k.items()) if (f in n if f else v['ms_per_step'] > 0.6)))" || exit 1
  done
done
