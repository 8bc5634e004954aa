"""Mixed LoRA variants in one batch against one call per variant (2B, bf16, compile()).  Prints one JSON line.

64 caption requests over 64 synthetic images, greedy, 32 tokens with ``ignore_eos``; four synthetic variants
(``synth.synthetic_lora`` seeds 1 .. 4, ranks 8, 64, 8, 64) and the base model take the rows in turn:
  mixed     ONE ``batch_generate_ids(..., variants=[...])`` call (the grouped kernels of csrc/lora_multi.hip);
  grouped   one ``batch_generate_ids(..., variant=v)`` call per variant plus one base call: the only option before;
  base      the same 64 requests on the base model alone.
Reported: answers/s per path (median of the interleaved repeats), and the decode time per step of the mixed and base
paths (the ``decode`` phase of ``collect_timing`` over 31 steps).  Mixed and grouped must give the same ids (asserted).

  python tools/bench_multi_lora.py [--repeats 3]
  python tools/bench_multi_lora.py --profile 4   # mixed then base only, N calls each, for a rocprofv3 --kernel-trace --stats run
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

TOKENS = 32
N = 64
VARIANTS = (("v1", 1, 8), ("v2", 2, 64), ("v3", 3, 8), ("v4", 4, 64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="2b")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--profile", type=int, default=0)
    args = ap.parse_args()

    import torch

    from moondream_amd import synth
    from moondream_amd.config import get_config
    from moondream_amd.moondream import IdTokenizer, MoondreamModel

    cfg = get_config(args.model)
    sd = synth.synthetic_state_dict(cfg, seed=args.seed, device="cuda")
    model = MoondreamModel(cfg, sd, device="cuda", tokenizer=IdTokenizer(), max_batch=N)
    model.compile()
    for name, seed, rank in VARIANTS:
        model.register_variant(name, synth.synthetic_lora(cfg, seed=seed, rank=rank, device="cuda"))
    images = [synth.synthetic_image(i, args.seed) for i in range(N)]
    prompt = cfg.tokenizer.templates["caption"]["normal"]
    names = [None] + [v[0] for v in VARIANTS]
    row_variant = [names[i % len(names)] for i in range(N)]
    kw = dict(max_tokens=TOKENS, ignore_eos=True)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, time.perf_counter() - t0

    def mixed():
        return model.batch_generate_ids(images, [prompt] * N, variants=row_variant, **kw)

    def grouped():
        out = [None] * N
        for v in names:
            rows = [i for i in range(N) if row_variant[i] == v]
            ids = model.batch_generate_ids([images[i] for i in rows], [prompt] * len(rows), variant=v, **kw)
            for i, r in zip(rows, ids):
                out[i] = r
        return out

    def base():
        return model.batch_generate_ids(images, [prompt] * N, **kw)

    if args.profile:
        for fn in (mixed, base):
            fn()
            for _ in range(args.profile):
                timed(fn)
        return

    for fn in (mixed, grouped, base):  # warm-up: graphs captured, bank filled
        fn()
    ids_mixed, ids_grouped = mixed(), grouped()
    assert ids_mixed == ids_grouped, [i for i in range(N) if ids_mixed[i] != ids_grouped[i]][:8]
    secs = {"mixed": [], "grouped": [], "base": []}
    step_ms = {"mixed": [], "base": []}
    model.collect_timing = True
    for _ in range(args.repeats):
        for name, fn in (("mixed", mixed), ("grouped", grouped), ("base", base)):
            _, dt = timed(fn)
            secs[name].append(dt)
            if name in step_ms:
                step_ms[name].append(model.last_phase_ms["decode"] / (TOKENS - 1))
    model.collect_timing = False
    med = {k: statistics.median(v) for k, v in secs.items()}
    res = {
        "metric": "multi_lora_answers_per_s", "model": args.model, "requests": N, "tokens": TOKENS,
        "variants": [{"name": n, "seed": s, "rank": r} for n, s, r in VARIANTS], "base_rows": row_variant.count(None),
        "answers_per_s": {k: round(N / v, 1) for k, v in med.items()},
        "mixed_over_grouped": round(med["grouped"] / med["mixed"], 2),
        "decode_ms_per_step": {k: round(statistics.median(v), 3) for k, v in step_ms.items()},
        "mixed_step_over_base_step": round(statistics.median(step_ms["mixed"]) / statistics.median(step_ms["base"]), 3),
        "repeats": args.repeats,
    }
    print(json.dumps(res))


if __name__ == "__main__":
    main()
