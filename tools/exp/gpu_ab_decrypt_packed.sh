#!/bin/bash
# same-box A/B of decrypt_packed between two checkouts (each with its own built library): PARENT=<path of the other checkout>.
# tools/bench_slots.py --only key_holder with each tree in turn, alternating, every process under its own time limit; stops at the
# first run that fails.  Output: $OUT/key_holder_<tree>_<k>.json (OUT=<output directory>)
cd "$(dirname "$0")/../.."
out=${OUT:?OUT=<output directory>}; mkdir -p $out
P=${PARENT:?PARENT=<checkout of the revision to compare with>}
k=0
for tree in $P . $P . $P .; do
  k=$((k + 1))
  name=$([ "$tree" = "." ] && echo this || echo parent)
  timeout -k 10 ${LIMIT:-150} python tools/bench_slots.py --only key_holder --tree $tree --repeats ${REPEATS:-5} > $out/key_holder_${name}_$k.json 2> $out/key_holder_${name}_$k.err \
    || { echo "$name run $k rc=$? - stopping"; tail -5 $out/key_holder_${name}_$k.err; exit 1; }
  echo "$name $k: $(cat $out/key_holder_${name}_$k.json)"
done
