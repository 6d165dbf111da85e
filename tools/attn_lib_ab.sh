# same-box A/B of library builds on the attention micro-benchmark: tools/attn_lib_ab.sh "B H N variants" a.so b.so ...
# (one process per library and round, each under its own time limit; the first failure ends the run)
SHAPES="$1"; shift
for round in 1 2 3; do
for l in "$@"; do
  export SDXL_LIB_PATH=$PWD/$l
  out=$(timeout -k 10 300 python tools/attn_variant_times.py $SHAPES 2>&1) || { echo "lib[$l] failed: $out"; exit 1; }
  echo "lib[$l] $(echo "$out" | grep -v amdgpu.ids | tail -1)"
done; done
