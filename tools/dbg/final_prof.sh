out=$(realpath -m "${1:?usage: bash tools/dbg/final_prof.sh <output directory>}") && mkdir -p "$out" || exit 1
cd $GRAFT_REPO_ROOT
bash tools/profile_aux.sh r04 > $out/profile_aux_r04.log 2>&1
cd $GRAFT_REPO_ROOT
for w in pranet gald deeplab_bn; do python bench.py --full --workload $w > $out/r04_bench_$w.json 2> $out/r04_bench_$w.err; done
python bench.py --full > $out/r04_bench_builder.json 2> $out/r04_bench_builder.err
for f in $out/r04_bench_pranet.json $out/r04_bench_gald.json $out/r04_bench_deeplab_bn.json $out/r04_bench_builder.json; do cut -c1-260 $f; done
