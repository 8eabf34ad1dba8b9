# SQ counters of the K12 kernels (sun depth pass, 2048^2, ~1M-triangle temple), a counter run of its own:
#   bash tools/k12_pmc.sh [output dir]      (prints one line per kernel; the raw CSV stays under the output dir)
set -e
export TMPDIR=/tmp
R=$PWD
OUT=${1:-/tmp/k12pmc}
rm -rf "$OUT/pmc"; mkdir -p "$OUT"
rocprofv3 --pmc SQ_WAVES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_VMEM_RD SQ_INSTS_LDS SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_INST_ANY --output-format csv -d "$OUT/pmc" \
    -- python3 "$R/tools/sun_depth_time.py" --out "$OUT/pmc_run.json" --timed 1 --walls 1 --passes 2 > /dev/null 2>&1
python3 - "$OUT" <<'PY'
import csv, glob, collections, re, sys
f = glob.glob(sys.argv[1] + "/pmc/**/*_counter_collection.csv", recursive=True)[0]
per = collections.defaultdict(lambda: collections.defaultdict(list))
for r in csv.DictReader(open(f)):
    m = re.search(r"(k_raster_[a-z]+)", r["Kernel_Name"])
    if not m: continue
    per[m.group(1)][r["Counter_Name"]].append(float(r["Counter_Value"]))
for k, c in sorted(per.items()):
    med = {n: sorted(v)[len(v) // 2] for n, v in c.items()}
    w = max(med.get("SQ_WAVES", 1.0), 1.0)
    print(f"{k:18s} waves {w:9.0f}  VALU/wave {med['SQ_INSTS_VALU']/w:8.0f}  SALU/wave {med['SQ_INSTS_SALU']/w:7.0f}  loads/wave {med['SQ_INSTS_VMEM_RD']/w:6.1f}  "
          f"LDS/wave {med['SQ_INSTS_LDS']/w:7.0f}  wave_cycles/wave {med['SQ_WAVE_CYCLES']/w:9.0f}  wait_inst/wave {med['SQ_WAIT_INST_ANY']/w:9.0f}  busy_cycles {med['SQ_BUSY_CYCLES']:11.0f}")
PY
