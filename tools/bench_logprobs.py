"""What token log-probabilities cost, and what the prefill-based scorer buys (2B, bf16, compile()).  Prints one JSON line.

  generation   B = 64 synthetic images, the caption prompt, greedy, 32 tokens with ``ignore_eos``: images/s of
               ``batch_generate_ids`` with ``return_logprobs`` off and on, each in ``--procs`` fresh processes that alternate
               (off, on, off, on, ..); per process the median of ``--repeats`` timed calls after a warm-up (graph captures), per
               leg the median and the span of the process medians.  With ``--parent-repo DIR`` (a built checkout of the parent
               commit) a third leg runs that tree's ``batch_generate_ids``, which has no such flag, the same way: the yardstick
               of "off costs nothing" -- ``off_within_parent_span`` says whether the off median lies inside the parent's span.
  choices      ``query_choices`` with 64 choices of 8 tokens (7 ids and the EOS) about one encoded image, in answers scored per
               second, against the only way to get these numbers without it: the same 64 continuations as forced decode steps
               through ``teacher_forced_logits`` gathering the whole vocabulary, then torch ``log_softmax`` on the host.
  parity       the tiny model on tests/golden/tiny_seed1.npz: the largest |logprob - float64 log-softmax of the reference's
               step logits| over the three golden captions, generated and scored (the tests bound it by 1.0).

  python tools/bench_logprobs.py [--parent-repo DIR] > profiles/logprobs_bench.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, TOKENS, N_CHOICES, CHOICE_IDS = 64, 32, 64, 7


def build_model(name, seed, max_batch):
    import torch  # noqa: F401

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


def worker_generation(args):
    """One process, one leg: ``flag`` off / on, or absent (a tree without the argument)."""
    cfg, synth, model = build_model(args.model, args.seed, B)
    model.compile()
    images = [synth.synthetic_image(i, args.seed) for i in range(B)]
    prompts = [cfg.tokenizer.templates["caption"]["normal"]] * B
    kw = {} if args.flag == "absent" else {"return_logprobs": args.flag == "on"}
    run = lambda: model.batch_generate_ids(images, prompts, max_tokens=TOKENS, ignore_eos=True, **kw)
    out = run()  # warm-up: graph captures
    ids = out[0] if args.flag == "on" else out
    times = [timed(run)[1] for _ in range(args.repeats)]
    med = statistics.median(times)
    print(json.dumps({"flag": args.flag, "images_per_s": round(B / med, 2), "run_s_all": [round(t, 4) for t in times],
                      "ids_crc": hash(tuple(map(tuple, ids))) & 0xFFFFFFFF}))


def worker_choices(args):
    import numpy as np
    import torch

    cfg, synth, model = build_model(args.model, args.seed, N_CHOICES + 4)
    model.compile()
    tk = cfg.tokenizer
    enc = model.encode_image(synth.synthetic_image(0, args.seed))
    prompt = synth.synthetic_vqa_prompt(cfg, 0, args.seed)
    pre, suf = len(tk.templates["query"]["prefix"]), len(tk.templates["query"]["suffix"])
    question = " ".join(str(t) for t in prompt[pre : len(prompt) - 2 * suf])
    assert model._query_prompts([question])[0] == list(prompt)
    rng = np.random.default_rng(args.seed)
    choice_ids = rng.integers(100, cfg.text.vocab_size, size=(N_CHOICES, CHOICE_IDS)).tolist()
    choices = [" ".join(map(str, c)) for c in choice_ids]
    conts = [c + [tk.eos_id] for c in choice_ids]

    def forced():
        """The 8 decisions of every continuation as one prompt pass and 7 forced decode steps; full-vocabulary gather."""
        idx = np.broadcast_to(np.arange(cfg.text.vocab_size), (N_CHOICES, CHOICE_IDS + 1, cfg.text.vocab_size))
        lg = model.teacher_forced_logits([enc] * N_CHOICES, [prompt] * N_CHOICES, choice_ids, idx)  # fp32 [64, 8, V] on the host
        lp = torch.log_softmax(lg, dim=-1)
        return torch.gather(lp, 2, torch.tensor(conts).unsqueeze(-1)).squeeze(-1)

    scored = lambda: model.query_choices(enc, question, choices)
    a, b = scored(), forced()  # warm-up
    diff = float((torch.tensor(a["per_token"]) - b).abs().max())
    t_new, t_old = [], []
    for _ in range(args.repeats):
        t_new.append(timed(scored)[1])
        t_old.append(timed(forced)[1])
    new, old = N_CHOICES / statistics.median(t_new), N_CHOICES / statistics.median(t_old)
    print(json.dumps({"choices": N_CHOICES, "tokens_per_choice": CHOICE_IDS + 1, "prompt_len": len(prompt),
                      "query_choices_answers_per_s": round(new, 2), "forced_decode_answers_per_s": round(old, 2),
                      "ratio": round(new / old, 2), "run_s_query_choices": [round(t, 4) for t in t_new],
                      "run_s_forced_decode": [round(t, 4) for t in t_old],
                      "max_abs_logprob_diff_between_the_two": round(diff, 4)}))


def worker_parity(args):
    import numpy as np
    import torch
    from PIL import Image

    sys.path.insert(0, os.path.join(REPO, "tests"))
    from util import bits_to_bf16

    g = np.load(os.path.join(REPO, "tests", "golden", "tiny_seed1.npz"))
    cfg, synth, model = build_model("tiny", int(g["seed"]), 4)
    images, prompts, tokens, refs = [], [], [], []
    for i in range(3):
        arr = synth.synthetic_image_array(int(g["image_index"][i]), int(g["seed"]), tuple(g[f"img{i}.cap.size"]))
        images.append(Image.fromarray(arr, "RGB"))
        prompts.append(g[f"img{i}.cap.prompt"].tolist())
        tokens.append(g[f"img{i}.cap.tokens"].tolist())
        lg = bits_to_bf16(g[f"img{i}.cap.step_logits"]).double()[: len(tokens[i])].clone()
        lg[1:, cfg.tokenizer.answer_id] = float("-inf")
        refs.append(torch.log_softmax(lg, 1)[torch.arange(len(tokens[i])), torch.tensor(tokens[i])])
    ids, lp, rk = model.batch_generate_ids(images, prompts, max_tokens=len(tokens[0]), return_logprobs=True)
    slp, srk = model.score_ids(images, prompts, tokens)
    err = lambda got: max(float((torch.tensor(got[i], dtype=torch.float64) - refs[i]).abs().max()) for i in range(3))
    print(json.dumps({"ids_equal_reference": ids == tokens, "generated_max_abs_err": round(err(lp), 5),
                      "scored_max_abs_err": round(err(slp), 5), "all_ranks_zero": not any(r for s in rk + srk for r in s),
                      "bound": 1.0}))


def child(argv, repo=None, timeout=900):
    """A fresh process of this file (``repo``: the tree its moondream_amd comes from); its last stdout line as JSON."""
    env = dict(os.environ, MD_BENCH_LOGPROBS_REPO=repo or REPO)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), *argv], env=env, stdout=subprocess.PIPE, timeout=timeout)
    if r.returncode != 0:
        raise SystemExit(f"worker {argv} failed with status {r.returncode}")
    line = r.stdout.decode().strip().splitlines()[-1]
    print(f"[bench_logprobs] {' '.join(argv[:4])}: {line}", file=sys.stderr, flush=True)
    return json.loads(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="2b")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parent-repo", default=None, help="a built checkout of the parent commit (the flag-absent leg)")
    ap.add_argument("--worker", choices=("generation", "choices", "parity"))
    ap.add_argument("--flag", choices=("off", "on", "absent"), default="off")
    args = ap.parse_args()
    sys.path.insert(0, os.environ.get("MD_BENCH_LOGPROBS_REPO", REPO))
    if args.worker:
        import torch

        with torch.inference_mode():
            {"generation": worker_generation, "choices": worker_choices, "parity": worker_parity}[args.worker](args)
        return

    common = ["--model", args.model, "--seed", str(args.seed), "--repeats", str(args.repeats)]
    legs = ["off", "on"] + (["absent"] if args.parent_repo else [])
    runs = {leg: [] for leg in legs}
    for _ in range(args.procs):  # alternate the legs: drift of the machine lands on all of them
        for leg in legs:
            runs[leg].append(child(["--worker", "generation", "--flag", leg, *common], args.parent_repo if leg == "absent" else None))
    result = {"metric": "logprobs_bench", "model": args.model, "batch": B, "tokens": TOKENS, "procs": args.procs, "repeats": args.repeats}
    gen = {}
    for leg in legs:
        v = [r["images_per_s"] for r in runs[leg]]
        gen["parent" if leg == "absent" else leg] = {"images_per_s_median": statistics.median(v), "images_per_s_span": [min(v), max(v)],
                                                     "images_per_s_all": v}
    assert len({r["ids_crc"] for r in runs["off"] + runs["on"]}) == 1, "the flag changed an id"
    gen["on_vs_off"] = round(gen["on"]["images_per_s_median"] / gen["off"]["images_per_s_median"], 4)
    if args.parent_repo:
        lo, hi = gen["parent"]["images_per_s_span"]
        gen["off_within_parent_span"] = lo <= gen["off"]["images_per_s_median"] <= hi
    result["generation"] = gen
    result["choices"] = child(["--worker", "choices", *common])
    result["parity_tiny"] = child(["--worker", "parity", *common])
    print(json.dumps(result))


if __name__ == "__main__":
    main()
