"""Launches per decode step and per-stage decode times of the multi-LoRA path, from the per-dispatch kernel trace of
``rocprofv3 --kernel-trace --output-format csv -- python tools/bench_multi_lora.py --profile N``.  Prints one JSON line.

The trace is cut into decode steps at each argmax launch (every step ends with md_argmax_advance, which lm_head feeds);
a step with a decode attention launch is a decode step, and it is a mixed step when it also launches a LoRA kernel.  Per
stage, the median time of the LoRA kernels inside decode steps, told apart by their grids.

  python tools/multi_lora_trace_split.py <kernel_trace.csv>
"""
import collections
import csv
import json
import statistics
import sys


def main():
    path = sys.argv[1]
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    steps, cur = [], []
    for r in rows:
        cur.append(r)
        if "argmax" in r["Kernel_Name"]:
            steps.append(cur)
            cur = []
    launches = {"mixed": [], "base": []}
    stage = collections.defaultdict(list)
    for st in steps:
        names = [r["Kernel_Name"] for r in st]
        if not any("attn_decode" in n for n in names):
            continue  # a prefill pass (or a torch-only segment)
        lora = [r for r in st if "lora_" in r["Kernel_Name"]]
        launches["mixed" if lora else "base"].append(len(st))
        for r in lora:
            kind = "shrink" if "lora_shrink" in r["Kernel_Name"] else "expand"
            key = f"{kind} grid {r['Grid_Size_X']}x{r['Grid_Size_Y']}x{r['Grid_Size_Z']}"
            stage[key].append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    res = {
        "decode_steps": {k: len(v) for k, v in launches.items()},
        "launches_per_step": {k: statistics.median(v) if v else None for k, v in launches.items()},
        "lora_stage_us_median": {k: round(statistics.median(v) / 1000, 2) for k, v in sorted(stage.items())},
        "lora_stage_launches": {k: len(v) for k, v in sorted(stage.items())},
    }
    print(json.dumps(res))


if __name__ == "__main__":
    main()
