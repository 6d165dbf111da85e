# same-box A/B of the upsample fold: tools/upsample_fold_ab.sh path/to/parent/libsdxl_mi355.so   (the in-tree library is "this")
# bench line parent / this / parent / this, then kernel traces of a replayed step and of a decode per library, twice (profiles/upsample_fold_ab.txt)
set -o pipefail
P=$(realpath "$1"); O=${2:-/tmp/upsample_fold_ab}; mkdir -p $O
for round in 1 2; do for l in parent this; do
  if [ $l = parent ]; then export SDXL_LIB_PATH=$P; else unset SDXL_LIB_PATH; fi
  timeout -k 10 240 python bench.py --gpus 1 --steps 5 --warmup 2 --full --no-cpu-baseline --no-live-parity 2>/dev/null | tail -1 | python -c "import json,sys; d=json.loads(sys.stdin.read()); print('bench[$l $round] images/s', d['value'], 'ms per image', d['ms_per_step'], 'step p50 ms', d['unet_step_ms_p50'], 'decode ms', d['decode_ms'], 'finite', d['outputs_finite'])" || exit 1
done; done
for round in 1 2; do for l in parent this; do
  if [ $l = parent ]; then export SDXL_LIB_PATH=$P; else unset SDXL_LIB_PATH; fi
  timeout -k 10 240 rocprofv3 --kernel-trace --output-format csv -d $O/step_$l -o t -- python tools/step_trace.py > $O/step_$l.log 2>&1 || exit 1
  echo "== step trace [$l $round]"; python tools/trace_launch_rows.py step $O/step_$l || exit 1
  timeout -k 10 240 rocprofv3 --kernel-trace --output-format csv -d $O/dec_$l -o t -- python tools/profile_decode.py f32_split > $O/dec_$l.log 2>&1 || exit 1
  echo "== decode trace [$l $round]"; python tools/trace_launch_rows.py decode $O/dec_$l || exit 1
  rm -rf $O/step_$l $O/dec_$l
done; done
