# forced Fr-program forms at the driver's command
mkdir -p gpurun_out/r03_ab2
for t in "none" "frvm_streams=4,frvm_lds_kb=78" "frvm_streams=4,frvm_lds_kb=64" "frvm_streams=4,frvm_lds_kb=100" "frvm_streams=4,frvm_lds_kb=36"; do
  f=gpurun_out/r03_ab2/$(echo $t | tr '=,' '__').json
  case $t in none*) T="";; *) T="--tuning $t";; esac
  timeout -k 10 120 python bench.py --gpus 1 --steps 20 --warmup 5 --full --no-cpu-baseline --no-reupload-leg --no-extra-legs $T > $f 2> ${f%.json}.err || exit 1
done
python3 - <<'PY'
import json,glob
for f in sorted(glob.glob('gpurun_out/r03_ab2/*.json')):
    for l in open(f):
        if l.startswith('{'):
            j=json.loads(l); print(f.split('/')[-1], j.get('tuning'), round(j['value']/1e6,3), {k:round(v,3) for k,v in j['stages_ms'].items()})
PY
