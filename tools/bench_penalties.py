"""What the repetition / presence / frequency penalties cost (2B, bf16, compile()).  Prints one JSON line, also written to
profiles/penalties_bench.json.

  generation   B = 64 synthetic images, the caption prompt, greedy, 32 tokens with ``ignore_eos``: ``batch_generate_ids`` with
               the penalties off (neutral: the call without the arguments), on for all rows and on for half of them, each
               in ``--procs`` fresh processes that alternate (off, all, half, [parent,] off, ..); per process the median of
               ``--repeats`` timed calls after a warm-up (graph captures), per leg the median and the span of the process
               medians.  Beside images/s each call's decode phase is timed with device events (``collect_timing``): ms per
               decode step, and for the on legs what a step gained over the off leg and that as a share of the step.
               With ``--parent-repo DIR`` (a built checkout of the parent commit) a fourth leg runs that tree's
               ``batch_generate_ids``, which has no such arguments: ``off_within_parent_span`` says whether the off median
               lies inside the parent's span.
  kernel       md_penalize_rows alone over 64 rows of 51200 logits, every row penalised, histories of 32 and of 1024 random
               tokens (hist_cap 2048; the token of each launch is no id, so the lengths stay): microseconds per launch from
               device events around ``--launches`` back-to-back launches, the median of ``--repeats`` such windows.

  python tools/bench_penalties.py [--parent-repo DIR]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, TOKENS, VOCAB, HIST_CAP = 64, 32, 51200, 2048
SETTINGS = dict(repetition_penalty=1.2, presence_penalty=0.5, frequency_penalty=0.25)


def worker_generation(args):
    """One process, one leg: off / all / half, or absent (a tree without the arguments)."""
    import torch

    from moondream_amd import synth
    from moondream_amd.config import get_config
    from moondream_amd.moondream import IdTokenizer, MoondreamModel

    cfg = get_config(args.model)
    sd = synth.synthetic_state_dict(cfg, seed=args.seed, device="cuda")
    model = MoondreamModel(cfg, sd, device="cuda", tokenizer=IdTokenizer(), max_batch=B)
    model.compile()
    model.collect_timing = True
    images = [synth.synthetic_image(i, args.seed) for i in range(B)]
    prompts = [cfg.tokenizer.templates["caption"]["normal"]] * B
    on = {"all": [True] * B, "half": [i % 2 == 0 for i in range(B)]}.get(args.leg)
    neutral = dict(repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0)
    kw = {} if args.leg in ("off", "absent") else {k: [v if o else neutral[k] for o in on] for k, v in SETTINGS.items()}
    run = lambda: model.batch_generate_ids(images, prompts, max_tokens=TOKENS, ignore_eos=True, **kw)
    ids = run()  # warm-up: graph captures
    times, decode = [], []
    for _ in range(args.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
        decode.append(model.last_phase_ms["decode"])
    print(json.dumps({"leg": args.leg, "images_per_s": round(B / statistics.median(times), 2),
                      "decode_ms_per_step": round(statistics.median(decode) / (TOKENS - 1), 4),
                      "run_s_all": [round(t, 4) for t in times], "ids_crc": hash(tuple(map(tuple, ids))) & 0xFFFFFFFF}))


def worker_kernel(args):
    import torch

    from moondream_amd import _lib

    lib = _lib.load()
    gen = torch.Generator().manual_seed(args.seed)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = {}
    for length in (32, 1024):
        logits = (torch.randn(B, VOCAB, generator=gen) * 8.0).to(torch.bfloat16).cuda()
        hist = torch.randint(0, VOCAB, (B, HIST_CAP), generator=gen, dtype=torch.int32).cuda()
        lens = torch.full((B,), length, dtype=torch.int32, device="cuda")
        tok = torch.full((B,), -1, dtype=torch.int32, device="cuda")  # no id: nothing is appended, the lengths stay
        st = torch.tensor([[SETTINGS["repetition_penalty"]] * B, [SETTINGS["presence_penalty"]] * B,
                           [SETTINGS["frequency_penalty"]] * B], dtype=torch.float32, device="cuda")

        def window(n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                _lib.check(lib.md_penalize_rows(logits.data_ptr(), logits.stride(0), B, VOCAB, tok.data_ptr(), None, 0, hist.data_ptr(),
                                                HIST_CAP, lens.data_ptr(), st[0].data_ptr(), st[1].data_ptr(), st[2].data_ptr(), stream),
                           "md_penalize_rows")
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e3 / n

        window(50)  # warm-up
        us = [window(args.launches) for _ in range(args.repeats)]
        out[f"history_{length}"] = {"us_per_launch_median": round(statistics.median(us), 2), "us_per_launch_all": [round(u, 2) for u in us],
                                    "distinct_tokens_per_row": int(torch.unique(hist[0, :length]).numel())}
    out.update(rows=B, vocab=VOCAB, hist_cap=HIST_CAP, launches_per_window=args.launches)
    print(json.dumps(out))


def child(argv, repo=None, timeout=900):
    """A fresh process of this file (``repo``: the tree its moondream_amd comes from); its last stdout line as JSON."""
    env = dict(os.environ, MD_BENCH_PENALTIES_REPO=repo or REPO)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), *argv], env=env, stdout=subprocess.PIPE, timeout=timeout)
    if r.returncode != 0:
        raise SystemExit(f"worker {argv} failed with status {r.returncode}")
    line = r.stdout.decode().strip().splitlines()[-1]
    print(f"[bench_penalties] {' '.join(argv[:4])}: {line}", file=sys.stderr, flush=True)
    return json.loads(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="2b")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--launches", type=int, default=500)
    ap.add_argument("--parent-repo", default=None, help="a built checkout of the parent commit (the arguments-absent leg)")
    ap.add_argument("--worker", choices=("generation", "kernel"))
    ap.add_argument("--leg", choices=("off", "all", "half", "absent"), default="off")
    args = ap.parse_args()
    sys.path.insert(0, os.environ.get("MD_BENCH_PENALTIES_REPO", REPO))
    if args.worker:
        import torch

        with torch.inference_mode():
            {"generation": worker_generation, "kernel": worker_kernel}[args.worker](args)
        return

    common = ["--model", args.model, "--seed", str(args.seed), "--repeats", str(args.repeats)]
    legs = ["off", "all", "half"] + (["absent"] if args.parent_repo else [])
    runs = {leg: [] for leg in legs}
    for _ in range(args.procs):  # alternate the legs: drift of the machine lands on all of them
        for leg in legs:
            runs[leg].append(child(["--worker", "generation", "--leg", leg, *common], args.parent_repo if leg == "absent" else None))
    result = {"metric": "penalties_bench", "model": args.model, "batch": B, "tokens": TOKENS, "procs": args.procs,
              "repeats": args.repeats, "settings": SETTINGS}
    gen = {}
    for leg in legs:
        v, d = [r["images_per_s"] for r in runs[leg]], [r["decode_ms_per_step"] for r in runs[leg]]
        gen["parent" if leg == "absent" else leg] = {
            "images_per_s_median": statistics.median(v), "images_per_s_span": [min(v), max(v)], "images_per_s_all": v,
            "decode_ms_per_step_median": statistics.median(d), "decode_ms_per_step_all": d}
    assert len({r["ids_crc"] for r in runs["off"] + runs.get("absent", [])}) == 1, "the neutral call's ids differ from the parent's"
    off = gen["off"]["decode_ms_per_step_median"]
    for leg in ("all", "half"):
        extra = gen[leg]["decode_ms_per_step_median"] - off
        gen[leg]["added_us_per_step"] = round(extra * 1e3, 1)
        gen[leg]["share_of_its_step"] = round(extra / gen[leg]["decode_ms_per_step_median"], 4)
        gen[leg]["images_per_s_vs_off"] = round(gen[leg]["images_per_s_median"] / gen["off"]["images_per_s_median"], 4)
    if args.parent_repo:
        lo, hi = gen["parent"]["images_per_s_span"]
        gen["off_within_parent_span"] = lo <= gen["off"]["images_per_s_median"] <= hi
        gen["off_vs_parent"] = round(gen["off"]["images_per_s_median"] / gen["parent"]["images_per_s_median"], 4)
    result["generation"] = gen
    result["kernel"] = child(["--worker", "kernel", "--seed", str(args.seed), "--repeats", str(args.repeats), "--launches", str(args.launches)])
    line = json.dumps(result)
    with open(os.path.join(REPO, "profiles", "penalties_bench.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
