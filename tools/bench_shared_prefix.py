"""Many questions about few images: the shared image prefix against the copy path (2B, bf16, compile()).  Prints one JSON line.

For each (images, questions per image) in {(1, 64), (4, 16), (1, 128)}: synthetic 378x378 images, 32-id synthetic question
prompts, greedy, 32 tokens with ``ignore_eos``, answers/s on
  raw     ``batch_generate_ids`` over the images repeated per question (ViT + image prefill once per row);
  copy    ``batch_generate_ids`` over repeated ``EncodedImage``s (each row's slot gets a copy of the prefix);
  shared  ``batch_generate_ids(..., share_prefix=True)`` over the same ``EncodedImage``s (one prefix slot per image);
  shared_raw  ``share_prefix=True`` over the raw images, i.e. what ``query_many`` does (one ViT + prefill per image).
The paths are interleaved across repeats; the median is reported.  copy and shared must give the same ids (asserted).

  python tools/bench_shared_prefix.py [--repeats 5]
  python tools/bench_shared_prefix.py --profile 4   # (1, 64) copy / shared only, for a rocprofv3 --kernel-trace --stats run
  python tools/bench_shared_prefix.py --fp8 > profiles/shared_prefix_f8_bench.json
      # the same legs in the fp8 KV mode: enable_fp8(kv_cache=True) calibrated on the tool's own images, before they are encoded
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

CONFIGS = ((1, 64), (4, 16), (1, 128))
TOKENS = 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="2b")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--profile", type=int, default=0, help="only (1, 64) copy then shared, N timed calls each")
    ap.add_argument("--fp8", action="store_true", help="every leg in the fp8 mode with the e4m3 copy of the KV cache")
    args = ap.parse_args()

    import torch

    from moondream_amd import synth
    from moondream_amd.config import get_config
    from moondream_amd.moondream import IdTokenizer, MoondreamModel

    cfg = get_config(args.model)
    sd = synth.synthetic_state_dict(cfg, seed=args.seed, device="cuda")
    model = MoondreamModel(cfg, sd, device="cuda", tokenizer=IdTokenizer(), max_batch=132)
    model.compile()
    images = [synth.synthetic_image(i, args.seed) for i in range(4)]
    if args.fp8:
        info = model.enable_fp8(images, synth.synthetic_vqa_prompt(cfg, 0, args.seed), kv_cache=True)
        assert info["kv_cache_fp8"], "this model has no e4m3 KV mode (MHA, head_dim 64, context <= 2048)"
    encs = [model.encode_image(im) for im in images]
    prompts_all = [synth.synthetic_vqa_prompt(cfg, i, args.seed) for i in range(128)]

    def rows(n_img, per):
        idx = [k for k in range(n_img) for _ in range(per)]
        return idx, prompts_all[: n_img * per]

    def run(path, n_img, per):
        idx, prompts = rows(n_img, per)
        if path == "raw":
            return model.batch_generate_ids([images[k] for k in idx], prompts, max_tokens=TOKENS, ignore_eos=True)
        if path == "copy":
            return model.batch_generate_ids([encs[k] for k in idx], prompts, max_tokens=TOKENS, ignore_eos=True)
        if path == "shared":
            return model.batch_generate_ids([encs[k] for k in idx], prompts, max_tokens=TOKENS, ignore_eos=True, share_prefix=True)
        return model.batch_generate_ids([images[k] for k in idx], prompts, max_tokens=TOKENS, ignore_eos=True, share_prefix=True)

    def timed(path, n_img, per):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ids = run(path, n_img, per)
        torch.cuda.synchronize()
        return ids, time.perf_counter() - t0

    with torch.inference_mode():
        if args.profile:
            for path in ("copy", "shared"):
                run(path, 1, 64)  # warm-up: graph captures
                for _ in range(args.profile):
                    timed(path, 1, 64)
            print(json.dumps({"profile_calls": args.profile, "decode_steps_per_call": TOKENS - 1, "rows": 64, "fp8_kv": args.fp8}))
            return
        paths = ("raw", "copy", "shared", "shared_raw")
        result = {"metric": "shared_prefix_answers_per_s", "model": args.model, "tokens": TOKENS, "repeats": args.repeats,
                  "prompt_len": len(prompts_all[0]), "fp8_kv": args.fp8}
        for n_img, per in CONFIGS:
            n = n_img * per
            ids = {p: run(p, n_img, per) for p in paths}  # warm-up
            assert ids["copy"] == ids["shared"], "shared-prefix ids differ from the copy path's"
            times = {p: [] for p in paths}
            for _ in range(args.repeats):
                for p in paths:
                    out, t = timed(p, n_img, per)
                    times[p].append(t)
                    if p == "shared":
                        assert out == ids["copy"]
            res = {}
            for p in paths:
                med = statistics.median(times[p])
                res[p] = {"answers_per_s": round(n / med, 2), "run_s_median": round(med, 4), "run_s_all": [round(t, 4) for t in times[p]]}
            res["shared_vs_copy"] = round(res["shared"]["answers_per_s"] / res["copy"]["answers_per_s"], 3)
            res["shared_raw_vs_raw"] = round(res["shared_raw"]["answers_per_s"] / res["raw"]["answers_per_s"], 3)
            res["ids_shared_equal_copy"] = True
            res["ids_raw_equal_copy"] = sum(a == b for a, b in zip(ids["raw"], ids["copy"]))
            result[f"{n_img}x{per}"] = res
    print(json.dumps(result))


if __name__ == "__main__":
    main()
