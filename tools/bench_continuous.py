"""Continuous batching vs the lockstep path on ragged caption lengths (2B, bf16, compile()).  Prints one JSON line.

Workload "ragged": N seeded synthetic 378x378 images with the caption prompt, per-request lengths uniform in 4..64 tokens
from a fixed seed, ``ignore_eos`` (the synthetic checkpoint's EOS behaviour is not a property to rely on, so the lengths
come from per-request ``max_tokens``).  Workload "uniform32": every request 32 tokens, as in bench.py -- nothing to compact,
so it bounds the engine's own overhead.

  (A) today's best: ``batch_generate_ids`` over consecutive groups of 64, each at its group's longest length, truncated
  (B) ContinuousEngine, max_live = 64
  (C) ContinuousEngine, max_live = 128

images/s = median of ``--repeats`` timed runs after one warm-up run; decode-phase ms from one further instrumented run
(A: the lockstep loop's own phase marks; B / C: the decode chunks, each bracketed by a device sync); row-steps: padded =
rows launched x steps, live = rows doing useful work (a request of n tokens needs n - 1 decode steps after its prefill).

Sampling: ``--temperature T --top-p P`` builds the engines with those engine-wide settings; ``--mixed-sampling`` gives a
quarter of the requests each of four settings per request, (0, -) greedy, (0.5, 0.3), (1.0, 0.8) and (4.0, 0.999), in one
engine.  Request i is seeded with i.  Sampled ids are not the lockstep leg's, so with either switch choose the engine legs
(``--legs B_continuous64``); ``ids_equal_A`` then compares with the first leg run.

    python tools/bench_continuous.py [--n 256] [--repeats 5] [--model 2b] [--legs A_lockstep64,B_continuous64]
                                     [--workloads ragged] [--temperature 0.5 --top-p 0.3 | --mixed-sampling]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="2b")
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--len-seed", type=int, default=0)
    ap.add_argument("--group", type=int, default=64, help="lockstep group size of (A)")
    ap.add_argument("--chunk", type=int, default=16)
    ap.add_argument("--legs", default="A_lockstep64,B_continuous64,C_continuous128")
    ap.add_argument("--workloads", default="ragged,uniform32")
    ap.add_argument("--temperature", type=float, default=0.0, help="engine-wide sampling temperature of the engine legs")
    ap.add_argument("--top-p", type=float, default=0.3)
    ap.add_argument("--mixed-sampling", action="store_true", help="four per-request settings, one of them greedy")
    args = ap.parse_args()

    import torch

    from moondream_amd import synth
    from moondream_amd.config import get_config
    from moondream_amd.continuous import ContinuousEngine
    from moondream_amd.moondream import IdTokenizer, MoondreamModel

    cfg = get_config(args.model)
    sd = synth.synthetic_state_dict(cfg, seed=args.seed, device="cuda")
    model = MoondreamModel(cfg, sd, device="cuda", tokenizer=IdTokenizer(), max_batch=128)
    model.compile()
    images = [synth.synthetic_image(i, args.seed) for i in range(args.n)]
    prompt = cfg.tokenizer.templates["caption"]["normal"]
    prompts = [prompt] * args.n
    workloads = {
        "ragged": [int(x) for x in np.random.default_rng(args.len_seed).integers(4, 65, args.n)],
        "uniform32": [32] * args.n,
    }

    def run_lockstep(mt, instrument=False):
        out, decode_ms, padded = [], 0.0, 0
        model.collect_timing = instrument
        try:
            for i0 in range(0, args.n, args.group):
                part = slice(i0, i0 + args.group)
                top = max(mt[part])
                ids = model.batch_generate_ids(images[part], prompts[part], max_tokens=top, ignore_eos=True)
                out += [s[:n] for s, n in zip(ids, mt[part])]
                padded += len(ids) * top
                if instrument:
                    decode_ms += model.last_phase_ms.get("decode", 0.0)
        finally:
            model.collect_timing = False
        torch.cuda.synchronize()
        return out, {"decode_ms": decode_ms, "padded_row_steps": padded, "live_row_steps": sum(n - 1 for n in mt)}

    def run_engine(max_live, mt, instrument=False):
        eng = ContinuousEngine(model, max_live=max_live, chunk=args.chunk, temperature=args.temperature, top_p=args.top_p)
        decode_ms = [0.0]
        if instrument:
            step = eng._step

            def timed(plan):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r = step(plan)  # ends with the chunk's D2H copy (a sync)
                decode_ms[0] += (time.perf_counter() - t0) * 1e3
                return r

            eng._step = timed
        out = eng.generate(images, prompts, max_tokens=mt, ignore_eos=True, seeds=list(range(args.n)), **per_request)
        torch.cuda.synchronize()
        s = eng.stats
        return out, {"decode_ms": decode_ms[0], "padded_row_steps": s.padded_row_steps, "live_row_steps": s.live_row_steps,
                     "decode_steps": s.decode_steps, "admissions": s.admissions, "prefill_passes": s.prefill_passes,
                     "graph_captures": s.graph_captures}

    per_request = {}
    if args.mixed_sampling:
        four = [(0.0, 0.3), (0.5, 0.3), (1.0, 0.8), (4.0, 0.999)]
        per_request = {"temperature": [four[i % 4][0] for i in range(args.n)], "top_p": [four[i % 4][1] for i in range(args.n)]}
    legs = {"A_lockstep64": run_lockstep, "B_continuous64": lambda mt, instrument=False: run_engine(64, mt, instrument),
            "C_continuous128": lambda mt, instrument=False: run_engine(128, mt, instrument)}
    legs = {k: legs[k] for k in args.legs.split(",")}
    workloads = {k: workloads[k] for k in args.workloads.split(",")}
    sampling = "mixed per request" if args.mixed_sampling else (
        "greedy" if args.temperature == 0 else "engine-wide T=%g top_p=%g" % (args.temperature, args.top_p))
    result = {"metric": "continuous_batching_images_per_s", "model": args.model, "n": args.n, "repeats": args.repeats,
              "chunk": args.chunk, "lengths": "uniform 4..64 (seed %d)" % args.len_seed, "sampling": sampling}
    with torch.inference_mode():
        for wname, mt in workloads.items():
            res, ref_ids = {}, None
            for lname, fn in legs.items():
                ids, _ = fn(mt)  # warm-up (graph captures, arenas)
                times = []
                for _ in range(args.repeats):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    ids, _ = fn(mt)
                    times.append(time.perf_counter() - t0)
                _, info = fn(mt, instrument=True)
                if ref_ids is None:
                    ref_ids = ids
                med = statistics.median(times)
                res[lname] = {"images_per_s": round(args.n / med, 2), "run_s_median": round(med, 4),
                              "run_s_all": [round(t, 4) for t in times], "ids_equal_A": ids == ref_ids,
                              **{k: (round(v, 2) if isinstance(v, float) else v) for k, v in info.items()}}
            if "A_lockstep64" in res:
                a = res["A_lockstep64"]["images_per_s"]
                for lname in res:
                    if lname != "A_lockstep64":
                        res[lname]["speedup_vs_A"] = round(res[lname]["images_per_s"] / a, 4)
            result[wname] = res
    print(json.dumps(result))


if __name__ == "__main__":
    main()
