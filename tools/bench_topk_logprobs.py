"""What the top-k alternatives (``top_logprobs=k``) cost (2B, bf16, compile()).  Prints one JSON line and writes it to
profiles/topk_logprobs_bench.json.

  generation   B = 64 synthetic images, the caption prompt, greedy, 32 tokens with ``ignore_eos``: images/s of
               ``batch_generate_ids`` in the legs logprobs off, ``return_logprobs`` only, ``top_logprobs=5`` and
               ``top_logprobs=20`` and, with ``--parent-repo DIR`` (a built checkout of the parent commit), that tree's
               ``return_logprobs``, off and ``top_logprobs=5`` legs -- each in ``--procs`` fresh processes that alternate (off,
               lp, top5, top20, parent, parent_off, parent_top5, off, ..); per process the median of ``--repeats`` timed calls
               after a warm-up (graph captures), per leg the median and the span of the process medians.  ``top5_vs_lp`` /
               ``top20_vs_lp``: the flag's cost against the ``return_logprobs`` leg of the same run; ``off_within_parent_span``
               / ``lp_within_parent_span`` / ``top5_within_parent_span``: whether this tree's median lies inside the span of
               the parent's same leg.
  score        one ``score_ids(..., top_logprobs=5)`` call over 64 eight-token continuations after one encoded image, in
               continuations per second, against the only route to these numbers without it: the same decisions as forced
               decode steps through ``teacher_forced_logits`` gathering the whole vocabulary, then ``log_softmax`` and
               ``topk`` on the host.

  python tools/bench_topk_logprobs.py [--parent-repo DIR]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_logprobs import B, CHOICE_IDS, N_CHOICES, TOKENS, build_model, timed  # noqa: E402

LEGS = {"off": {}, "lp": {"return_logprobs": True}, "top5": {"return_logprobs": True, "top_logprobs": 5},
        "top20": {"return_logprobs": True, "top_logprobs": 20}, "parent": {"return_logprobs": True}, "parent_off": {},
        "parent_top5": {"return_logprobs": True, "top_logprobs": 5}}
SCORE_K = 5


def worker_generation(args):
    """One process, one leg."""
    cfg, synth, model = build_model(args.model, args.seed, B)
    model.compile()
    images = [synth.synthetic_image(i, args.seed) for i in range(B)]
    prompts = [cfg.tokenizer.templates["caption"]["normal"]] * B
    run = lambda: model.batch_generate_ids(images, prompts, max_tokens=TOKENS, ignore_eos=True, **LEGS[args.leg])
    out = run()  # warm-up: graph captures
    ids = out[0] if LEGS[args.leg] else out
    times = [timed(run)[1] for _ in range(args.repeats)]
    med = statistics.median(times)
    print(json.dumps({"leg": args.leg, "images_per_s": round(B / med, 2), "run_s_all": [round(t, 4) for t in times],
                      "ids_crc": hash(tuple(map(tuple, ids))) & 0xFFFFFFFF}))


def worker_score(args):
    import numpy as np
    import torch

    cfg, synth, model = build_model(args.model, args.seed, N_CHOICES + 4)
    model.compile()
    tk = cfg.tokenizer
    enc = model.encode_image(synth.synthetic_image(0, args.seed))
    prompt = list(synth.synthetic_vqa_prompt(cfg, 0, args.seed))
    rng = np.random.default_rng(args.seed)
    choice_ids = rng.integers(100, cfg.text.vocab_size, size=(N_CHOICES, CHOICE_IDS)).tolist()
    conts = [c + [tk.eos_id] for c in choice_ids]

    def forced():
        """The 8 decisions of every continuation as one prompt pass and 7 forced decode steps; full-vocabulary gather."""
        idx = np.broadcast_to(np.arange(cfg.text.vocab_size), (N_CHOICES, CHOICE_IDS + 1, cfg.text.vocab_size))
        lg = model.teacher_forced_logits([enc] * N_CHOICES, [prompt] * N_CHOICES, choice_ids, idx)  # fp32 [64, 8, V] on the host
        lp = torch.log_softmax(lg, dim=-1)
        return torch.topk(lp, SCORE_K, dim=-1)

    scored = lambda: model.score_ids([enc] * N_CHOICES, [prompt] * N_CHOICES, conts, share_prefix=True, top_logprobs=SCORE_K)
    a, b = scored(), forced()  # warm-up
    got = torch.tensor([[[x for _, x in dec] for dec in seq] for seq in a[2]])
    diff = float((got - b.values).abs().max())
    same_top1 = float((torch.tensor([[dec[0][0] for dec in seq] for seq in a[2]]) == b.indices[..., 0]).float().mean())
    t_new, t_old = [], []
    for _ in range(args.repeats):
        t_new.append(timed(scored)[1])
        t_old.append(timed(forced)[1])
    new, old = N_CHOICES / statistics.median(t_new), N_CHOICES / statistics.median(t_old)
    print(json.dumps({"continuations": N_CHOICES, "tokens_per_continuation": CHOICE_IDS + 1, "k": SCORE_K, "prompt_len": len(prompt),
                      "score_ids_continuations_per_s": round(new, 2), "forced_decode_host_topk_continuations_per_s": round(old, 2),
                      "ratio": round(new / old, 2), "run_s_score_ids": [round(t, 4) for t in t_new],
                      "run_s_forced_decode": [round(t, 4) for t in t_old],
                      "max_abs_logprob_diff_between_the_two": round(diff, 4), "top1_agreement": round(same_top1, 4)}))


def child(argv, repo=None, timeout=900):
    """A fresh process of this file (``repo``: the tree its moondream_amd comes from); its last stdout line as JSON."""
    env = dict(os.environ, MD_BENCH_LOGPROBS_REPO=repo or REPO)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), *argv], env=env, stdout=subprocess.PIPE, timeout=timeout)
    if r.returncode != 0:
        raise SystemExit(f"worker {argv} failed with status {r.returncode}")
    line = r.stdout.decode().strip().splitlines()[-1]
    print(f"[bench_topk_logprobs] {' '.join(argv[:4])}: {line}", file=sys.stderr, flush=True)
    return json.loads(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="2b")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parent-repo", default=None, help="a built checkout of the parent commit (its legs)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "topk_logprobs_bench.json"))
    ap.add_argument("--worker", choices=("generation", "score"))
    ap.add_argument("--leg", choices=tuple(LEGS), default="off")
    args = ap.parse_args()
    sys.path.insert(0, os.environ.get("MD_BENCH_LOGPROBS_REPO", REPO))
    if args.worker:
        import torch

        with torch.inference_mode():
            {"generation": worker_generation, "score": worker_score}[args.worker](args)
        return

    common = ["--model", args.model, "--seed", str(args.seed), "--repeats", str(args.repeats)]
    legs = [leg for leg in LEGS if not leg.startswith("parent") or args.parent_repo]
    runs = {leg: [] for leg in legs}
    for _ in range(args.procs):  # alternate the legs: drift of the machine lands on all of them
        for leg in legs:
            runs[leg].append(child(["--worker", "generation", "--leg", leg, *common],
                                   args.parent_repo if leg.startswith("parent") else None))
    result = {"metric": "topk_logprobs_bench", "model": args.model, "batch": B, "tokens": TOKENS, "procs": args.procs,
              "repeats": args.repeats}
    gen = {}
    for leg in legs:
        v = [r["images_per_s"] for r in runs[leg]]
        gen[leg] = {"images_per_s_median": statistics.median(v), "images_per_s_span": [min(v), max(v)], "images_per_s_all": v}
    assert len({r["ids_crc"] for leg in legs for r in runs[leg]}) == 1, "a flag changed an id"
    for leg in ("top5", "top20"):
        gen[f"{leg}_vs_lp"] = round(gen[leg]["images_per_s_median"] / gen["lp"]["images_per_s_median"], 4)
    gen["lp_vs_off"] = round(gen["lp"]["images_per_s_median"] / gen["off"]["images_per_s_median"], 4)
    if args.parent_repo:
        for leg, parent in (("lp", "parent"), ("off", "parent_off"), ("top5", "parent_top5")):
            lo, hi = gen[parent]["images_per_s_span"]
            gen[f"{leg}_within_parent_span"] = lo <= gen[leg]["images_per_s_median"] <= hi
    result["generation"] = gen
    result["score"] = child(["--worker", "score", *common])
    line = json.dumps(result)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
