"""Summarise the ab_*.log bench lines of tools/ab_bench.sh (under $RJ_OUT, default bench_out)."""
import glob
import json
import os

for f in sorted(glob.glob(os.path.join(os.environ.get("RJ_OUT", "bench_out"), "ab_*.log"))):
    for line in open(f):
        if line.startswith("{"):
            d = json.loads(line)
            st = d["stages_ms_per_step"]
            print(f"{os.path.basename(f)[3:-4]:14s} {d['value']:10.1f} img/s {d['ms_per_step']:7.3f} ms | " +
                  " ".join(f"{k[:-3]}={v:.3f}" for k, v in st.items()))
