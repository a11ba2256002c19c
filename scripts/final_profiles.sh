# round-end evidence: bench line, rocprofv3 kernel stats of the same command, HBM traffic PMC passes
# usage: final_profiles.sh <output dir>
O=$1
cd /tmp && export TMPDIR=/tmp; cd $GRAFT_REPO_ROOT
mkdir -p $O
python3 bench.py --full > $O/bench.json 2> $O/bench.err
tail -c 600 $O/bench.json
rocprofv3 --kernel-trace --stats --output-format csv -d $O/stats -o runc -- python3 bench.py --full --no-cpu-baseline --no-extras > $O/stats.log 2>&1
rocprofv3 --kernel-trace --stats --output-format csv -d $O/stats_eager1 -o runc -- python3 bench.py --full --no-cpu-baseline --no-extras --no-h2d --reps 1 --no-graph --pipeline 1 --steps 20 --warmup 5 > $O/stats_eager1.log 2>&1
for set in FETCH_SIZE WRITE_SIZE; do
  rocprofv3 --pmc $set --kernel-trace --output-format csv -d $O/pmc_$set -o runc -- python3 scripts/fwd_only.py 3 > $O/pmc_$set.log 2>&1
done
python3 scripts/make_traffic_json.py $O $O/conv_hbm_traffic.json | tail -30
