set -o pipefail
# headline A/B over environment settings, 3 rounds: bash scripts/gpu_ab_env.sh "A=0 B=1" "A=1 B=1" ...
# (each argument: one configuration, space-separated VAR=value pairs)
mkdir -p gpurun_out
T=$(mktemp -d)  # the bench line of each run (read back at once)
for i in 1 2 3; do
  for cfg in "$@"; do
    env $cfg timeout -k 10 300 python bench.py --full --no-cpu-baseline --no-e2e > $T/b_env.json 2> $T/b_env.err || { tail -20 $T/b_env.err; exit 1; }
    echo "[$cfg] $(python -c "import json; d=json.load(open('$T/b_env.json')); print(d['value'], d['ms_per_step'], d['roofline']['avg_ms'])")"
  done
done
