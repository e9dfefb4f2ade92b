set -o pipefail
O=${OUT:-measure_out}/rep; mkdir -p $O
for cfg in "--replicas 2 --chain-batches 4" "--replicas 3 --chain-batches 4" "--replicas 3 --chain-batches 2" "--replicas 4 --chain-batches 2"; do
  timeout -k 10 300 python -u bench.py --full --no-cpu-baseline --no-isolated $cfg > $O/b.json 2>$O/b.err || { tail $O/b.err; exit 1; }
  python -c "import json,sys; d=json.load(open('$O/b.json')); print('$cfg', round(d['value']), {k:v for k,v in d.items() if 'p50' in k})"
done
