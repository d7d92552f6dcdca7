#   bash tools/le_bench.sh [out dir]   layer engine on / off: decode bench per preset
set -o pipefail
OUT=${1:-le_bench_out}
mkdir -p "$OUT"
for p in llama3-8b-q4km tinyllama-q8_0; do
  for e in 1 0; do
    LLMI_ENGINE=$e timeout -k 10 240 python -u bench.py --full --preset $p --steps 128 --warmup 16 --no-cpu-baseline --batch-seqs '' --no-other-numerics > "$OUT/b_${p}_e$e.json" 2> "$OUT/b_${p}_e$e.log" || exit 1
    python -c "import json;d=json.load(open('$OUT/b_${p}_e$e.json'));print('$p e=$e', d['value'], d['c2_full'], {k:(v['us'],v['per_step']) for k,v in d['kernels'].items()})"
  done
done
