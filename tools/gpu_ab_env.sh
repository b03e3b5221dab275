# GPU box: A/B of environment switches on the 512^3 bench (same box, same binary, interleaved runs).
# usage: AB_ENVS="MVTV_DCT_FASTDIV=1 MVTV_FOLD_OFF=1" bash tools/gpu_ab_env.sh   (results under AB_OUT, default out/ab)
set -o pipefail
R=$GRAFT_REPO_ROOT
cd $R
O=${AB_OUT:-out/ab}
mkdir -p $O
if [ -n "$AB_TESTS" ]; then
  env $AB_TEST_ENV timeout -k 10 300 python -u -m pytest $AB_TESTS -x -q -m gpu --timeout 120 --timeout-method thread > $O/tests.log 2>&1 || { tail -20 $O/tests.log; exit 1; }
  tail -2 $O/tests.log
fi
for rep in $(seq 1 ${AB_REPS:-2}); do
  for e in base $AB_ENVS; do
    if [ "$e" = base ]; then ev=""; else ev="$e"; fi
    env $ev timeout -k 10 200 python bench.py --full --no-cpu --pcg-steps 0 --steps ${AB_STEPS:-30} --warmup 3 > $O/$e.$rep.json 2> $O/$e.$rep.err || { echo "bench $e failed"; tail -5 $O/$e.$rep.err; exit 1; }
    python -c "import json,sys;d=json.load(open(sys.argv[1]));print(sys.argv[2],d['value'],{k:v['avg_ms'] for k,v in d['kernels'].items()})" $O/$e.$rep.json "$e.$rep"
  done
done
