# the round's final records in ONE box (boxes differ by 3-5 %): run from the repo root on the GPU box;  OUT=<folder> bash tools/final_records.sh TAG HEAD [bench-only]
# HEAD = `git rev-parse --short HEAD` of the tree sent to the box (the box has no .git): it goes into every summary (profiles/summarize.py provenance)
set -e
TAG=${1:-r05}; HEAD=${2:-unknown}
SUMMARY=${OUT:?set OUT to the folder the records go to}/${TAG}_summary
mkdir -p "$SUMMARY"
if [ "$3" != "bench-only" ]; then
  bash profiles/collect.sh $TAG 128 $HEAD > gpurun_out/${TAG}_collect.log 2>&1
  python3 profiles/summarize.py $TAG 128 > gpurun_out/${TAG}_summarize.log 2>&1
  cp profiles/${TAG}_* "$SUMMARY"/
  rm -rf gpurun_out/${TAG}_sq1 gpurun_out/${TAG}_sq2 gpurun_out/${TAG}_fetch gpurun_out/${TAG}_write gpurun_out/${TAG}_stats gpurun_out/${TAG}_stats1
fi
# the bench lines of the records carry every section (--full): the CPU baseline, parity, the strong-scaling configs, the SOR-only launches
python3 bench.py --full > "$SUMMARY/${TAG}_bench.json" 2> "$SUMMARY/${TAG}_bench.err"
python3 bench.py --full --gpus 1 --steps 20 --warmup 5 > "$SUMMARY/${TAG}_bench_steps20.json" 2>> "$SUMMARY/${TAG}_bench.err"
echo "$HEAD" > "$SUMMARY/${TAG}_bench_head.txt"
echo collected
