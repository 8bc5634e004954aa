"""What the batched reasoning query buys, and what its control flow costs per step (2B synthetic weights, bf16,
compile()).  Prints one JSON line.

B = 64 synthetic images, one question, greedy, ``max_tokens`` = 32 per phase, end to end (vision encoder included):
  (a) batch      answers/s of ``batch_query(images, questions, reasoning=True)``;
  (b) sequential the same 64 as ``query(image, question, reasoning=True)`` calls, one after the other (that path has one
                 host decision per token and is unchanged by the batched form: timed in the same build);
  (c) plain      ``batch_generate_ids`` over the same images and prompts (plus the thinking token) for exactly the number of
                 decode steps (a) ran, ``ignore_eos``: the same lockstep without the region head, the routing kernel and the
                 mask -- (a)/(c) isolates what those cost per step.
Each leg in ``--procs`` fresh processes that alternate (a, b, c, a, b, c, ..); per process the median of ``--repeats`` timed
calls after a warm-up ((b): one timed pass over the 64 calls after two warm-up calls); per leg the median and the span of
the process medians.

  python tools/bench_reasoning.py > profiles/reasoning_bench.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
import zlib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, TOKENS, QUESTION = 64, 32, "11 12 13"


def build_model(name, seed, max_batch):
    from moondream_amd import synth
    from moondream_amd.config import get_config
    from moondream_amd.moondream import IdTokenizer, MoondreamModel

    cfg = get_config(name)
    sd = synth.synthetic_state_dict(cfg, seed=seed, device="cuda")
    return cfg, synth, MoondreamModel(cfg, sd, device="cuda", tokenizer=IdTokenizer(), max_batch=max_batch)


def timed(fn):
    import torch

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def worker(args):
    cfg, synth, model = build_model(args.model, args.seed, B)
    model.compile()
    tk = cfg.tokenizer
    images = [synth.synthetic_image(i, args.seed) for i in range(B)]
    st = {"temperature": 0, "max_tokens": TOKENS}
    out = {"leg": args.leg}
    if args.leg == "batch":
        run = lambda: model.batch_query(images, [QUESTION] * B, settings=st, reasoning=True)
        res = run()  # warm-up: graph captures
        times = [timed(run)[1] for _ in range(args.repeats)]
        out["steps"] = int(model.last_reason_steps)
        out["reasoning_tokens"] = sum(len(r["reasoning"]["text"].split()) for r in res)
        out["answer_tokens"] = sum(len(r["answer"].split()) for r in res)
        out["answers_crc"] = zlib.crc32("|".join(r["answer"] for r in res).encode())
    elif args.leg == "sequential":
        one = lambda i: model.query(images[i], QUESTION, reasoning=True, settings=st)
        one(0), one(1)  # warm-up
        res, t = timed(lambda: [one(i) for i in range(B)])
        times = [t]
        out["answers_crc"] = zlib.crc32("|".join(r["answer"] for r in res).encode())
    else:
        tpl = tk.templates["query"]
        prompt = list(tpl["prefix"]) + [int(t) for t in QUESTION.split()] + list(tpl["suffix"]) + [tk.thinking_id]
        run = lambda: model.batch_generate_ids(images, [prompt] * B, max_tokens=args.steps, ignore_eos=True)
        run()
        times = [timed(run)[1] for _ in range(args.repeats)]
        out["steps"] = args.steps
    out.update(answers_per_s=round(B / statistics.median(times), 2), run_s_all=[round(t, 4) for t in times])
    print(json.dumps(out))


def child(argv, timeout=900):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), *argv], stdout=subprocess.PIPE, timeout=timeout)
    if r.returncode != 0:
        raise SystemExit(f"worker {argv} failed with status {r.returncode}")
    line = r.stdout.decode().strip().splitlines()[-1]
    print(f"[bench_reasoning] {' '.join(argv[:4])}: {line}", file=sys.stderr, flush=True)
    return json.loads(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="2b")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--leg", choices=("batch", "sequential", "plain"))
    ap.add_argument("--steps", type=int, default=2 * TOKENS + 1)
    args = ap.parse_args()
    sys.path.insert(0, REPO)
    if args.leg:
        import torch

        with torch.inference_mode():
            worker(args)
        return
    common = ["--model", args.model, "--seed", str(args.seed), "--repeats", str(args.repeats)]
    runs = {"batch": [], "sequential": [], "plain": []}
    for _ in range(args.procs):  # alternate the legs: drift of the machine lands on all of them
        runs["batch"].append(child(["--leg", "batch", *common]))
        runs["sequential"].append(child(["--leg", "sequential", *common]))
        runs["plain"].append(child(["--leg", "plain", "--steps", str(runs["batch"][-1]["steps"]), *common]))
    assert len({r["answers_crc"] for r in runs["batch"]}) == 1
    result = {"metric": "reasoning_bench", "model": args.model, "batch_size": B, "max_tokens_per_phase": TOKENS, "procs": args.procs,
              "repeats": args.repeats, "decode_steps": runs["batch"][0]["steps"],
              "reasoning_tokens": runs["batch"][0]["reasoning_tokens"], "answer_tokens": runs["batch"][0]["answer_tokens"]}
    for leg, v in runs.items():
        a = [r["answers_per_s"] for r in v]
        result[leg] = {"answers_per_s_median": statistics.median(a), "answers_per_s_span": [min(a), max(a)], "answers_per_s_all": a}
    med = lambda leg: result[leg]["answers_per_s_median"]
    result["batch_vs_sequential"] = round(med("batch") / med("sequential"), 2)
    result["batch_vs_plain"] = round(med("batch") / med("plain"), 4)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
