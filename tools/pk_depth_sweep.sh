# persistent decode step: same-box sweep of the loaders' in-flight depth (MS_PK_DEPTH), bench lines
mkdir -p gpurun_out; O=gpurun_out/pk_depth.txt; : > $O
T=$(mktemp -d)
for d in ${DEPTHS:-12 20 28 36 44}; do
  MS_PERSIST=1 MS_PK_DEPTH=$d timeout -k 10 300 python3 bench.py --full --no-cpu-baseline --no-roofline --steps 2 --warmup 1 > $T/pkd.json 2> $T/pkd.err || { tail -20 $T/pkd.err; exit 1; }
  python3 -c "import json; d=json.load(open('$T/pkd.json')); b=d['breakdown']; print('depth $d', d['value'], b['decode_ms_per_decode_step'], d['check'])" | tee -a $O
done
