set -e -o pipefail
export TMPDIR=/tmp
out=${1:?usage: bash tools/prof_train.sh OUT_DIR}
mkdir -p $out
rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/prof_kt -o kt -- python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-decode --no-roofline > $out/bench.json 2> $out/err.log
cp /tmp/prof_kt/*kernel_stats.csv $out/kernel_stats.csv
python tools/kstats.py $out 27 40
