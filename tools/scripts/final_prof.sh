set -o pipefail
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
O=gpurun_out/r2j; mkdir -p $O
python bench.py --full > $O/bench_default.json 2> $O/bench_default.err; tail -c 600 $O/bench_default.json
rocprofv3 --kernel-trace --stats -d $O/ks_default -o p --output-format csv -- python3 bench.py --full --no-cpu-baseline > $O/bench_default_prof.json 2> $O/ks_default.log
rocprofv3 --kernel-trace --stats -d $O/ks_seq -o p --output-format csv -- python3 bench.py --full --no-cpu-baseline --inflight 1 --no-graph --steps 3 --warmup 1 > $O/bench_seq_prof.json 2> $O/ks_seq.log
for c in FETCH_SIZE WRITE_SIZE; do rocprofv3 --pmc $c -d $O/pmc_$c -o p --output-format csv -- python3 bench.py --full --no-cpu-baseline --no-fp32-compare --inflight 1 --no-graph --steps 1 --warmup 0 > /dev/null 2> $O/pmc_$c.log; done
rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE SQ_WAVE_CYCLES SQ_WAIT_INST_ANY SQ_WAIT_ANY SQ_ACTIVE_INST_ANY -d $O/pmc_SQ -o p --output-format csv -- python3 bench.py --full --no-cpu-baseline --no-fp32-compare --inflight 1 --no-graph --steps 1 --warmup 0 > /dev/null 2> $O/pmc_SQ.log
find $O -name "*.csv" | head -20
for d in pmc_FETCH_SIZE pmc_WRITE_SIZE pmc_SQ; do f=$(find $O/$d -name "*counter_collection.csv" | head -1); [ -n "$f" ] && cp $f $O/$d/p_counter_collection.csv; done
python tools/summarize_pmc.py $O/pmc_FETCH_SIZE $O/pmc_WRITE_SIZE $O/pmc_SQ $O/pmc_traffic.json > $O/pmc_traffic.log 2>&1; tail -3 $O/pmc_traffic.log
python tools/pmc_summary.py $O/pmc_SQ > $O/pmc_sq.txt 2>&1
for f in $(find $O/ks_default $O/ks_seq -name "*kernel_stats.csv"); do echo $f; head -8 $f | cut -c1-150; done
python bench.py --full --no-cpu-baseline --fp32 > $O/bench_fp32.json 2> /dev/null
python bench.py --full --no-cpu-baseline --prior aia_complex_trans_ri > $O/bench_aia_ri.json 2> /dev/null
python bench.py --full --no-cpu-baseline --prior dual_aia_trans_merge_crm > $O/bench_aia_dual.json 2> /dev/null
python bench.py --full --no-cpu-baseline --seconds 10 --batch 16 > $O/bench_10s_b16.json 2> /dev/null
python bench.py --full --no-cpu-baseline --full-schedule > $O/bench_full50.json 2> /dev/null
python tools/time_eps.py > $O/eps_per_launch.txt 2>&1
python tools/time_gcrn.py > $O/gcrn_per_launch.txt 2>&1
for f in fp32 aia_ri aia_dual 10s_b16 full50; do python -c "import json; d=json.loads(open('$O/bench_$f.json').read().strip().splitlines()[-1]); print('$f', d['ms_per_step'], d.get('ms_per_step_sequential'), d['value'], d['dtype'])"; done
