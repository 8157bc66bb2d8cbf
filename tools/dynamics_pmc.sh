#!/bin/bash
# Issue / LDS counters of the dynamics and controller-solve kernels (one pass,
# 8 SQ slots): where a wave's cycles go at 1,048,576 fp64 states.
#   [OUT=dir] bash tools/dynamics_pmc.sh   -> $OUT/{sq/, sq.log, summary.json} (default build_pmc/dynamics)
ROOT=$(pwd); OUT=${OUT:-$ROOT/build_pmc/dynamics}; case $OUT in /*) ;; *) OUT=$ROOT/$OUT;; esac; mkdir -p $OUT; cd /tmp; export TMPDIR=/tmp
CNT="SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_WAIT_INST_LDS SQ_ACTIVE_INST_LDS"
timeout -k 10 240 rocprofv3 --kernel-trace --pmc $CNT --output-format csv -d $OUT/sq -o run -- \
  python3 $ROOT/tools/dynamics_bench.py --batches 1048576 --reps 2 --warmup 1 > $OUT/sq.log 2>&1
rc=$?; echo "sq rc=$rc"; [ $rc -eq 0 ] || { tail -5 $OUT/sq.log; exit $rc; }
python3 - "$OUT" <<'PY'
import csv, glob, json, sys
out = sys.argv[1]
agg = {}
for f in glob.glob(out + "/sq/**/*counter_collection.csv", recursive=True):
    for row in csv.DictReader(open(f)):
        k = row["Kernel_Name"].split("(")[0]
        if "dynamics" not in k and "control_solve" not in k and "frame_kin" not in k:
            continue
        d = agg.setdefault(k, {})
        d.setdefault(row["Counter_Name"], []).append(float(row["Counter_Value"]))
res = {k: {c: sum(v) / len(v) for c, v in d.items()} for k, d in agg.items()}
json.dump(res, open(out + "/summary.json", "w"), indent=1)
for k, d in res.items():
    wc = d.get("SQ_WAVE_CYCLES", 0) or 1
    print(k[:60], {c: round(v / wc, 3) for c, v in d.items() if c not in ("SQ_WAVES", "SQ_BUSY_CYCLES")}, "waves", d.get("SQ_WAVES"))
PY
