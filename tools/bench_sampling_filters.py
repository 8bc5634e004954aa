"""What per-request top-k / min-p sampling costs (2B, bf16, compile()).  Prints one JSON line, also written to
profiles/sampling_filters_bench.json.

  generation   B = 64 synthetic images, the caption prompt, temperature 0.5 / top-p 0.3 (the reference's defaults), 32 tokens
               with ``ignore_eos``: ``batch_generate_ids`` with the filters off (neutral: the call without the arguments),
               ``top_k=40`` on all rows, ``min_p=0.1`` on all rows, and both on half the rows, each in ``--procs`` fresh
               processes that alternate (off, [parent,] top_k, min_p, half, off, ..); per process the median of ``--repeats``
               timed calls after a warm-up (graph captures), per leg the median and the span of the process medians.
               Beside images/s each call's decode phase is timed with device events (``collect_timing``): ms per decode
               step, and for the filtered legs what a step gained over the off leg.  With ``--parent-repo DIR`` (a built
               checkout of the parent commit) one more leg runs that tree's ``batch_generate_ids``, which has no such
               arguments: ``off_within_parent_span`` says whether the off median lies inside the parent's span.
               ``--skip-generation`` leaves this part out.
  kernel       md_sample_rows against md_sample_rows_filtered over 64 rows of 51200 logits (temperature 0.5, top-p 0.3;
               the filtered launch with every row neutral, with top_k = 40, with min_p = 0.1 and with both): microseconds
               per launch from device events around ``--launches`` back-to-back launches, the median of ``--repeats`` such
               windows, all from the same process.

  python tools/bench_sampling_filters.py [--parent-repo DIR] [--skip-generation]
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
B, TOKENS, VOCAB = 64, 32, 51200
TEMPERATURE, TOP_P, TOP_K, MIN_P = 0.5, 0.3, 40, 0.1
LEGS = ("off", "top_k", "min_p", "half")


def worker_generation(args):
    """One process, one leg: off / top_k / min_p / half, or absent (a tree without the arguments)."""
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
    half = [i % 2 == 0 for i in range(B)]
    kw = {"off": dict(top_k=0, min_p=0.0), "absent": {}, "top_k": dict(top_k=TOP_K), "min_p": dict(min_p=MIN_P),
          "half": dict(top_k=[TOP_K if o else 0 for o in half], min_p=[MIN_P if o else 0.0 for o in half])}[args.leg]

    def run():
        gen = torch.Generator(device="cuda").manual_seed(args.seed)
        return model.batch_generate_ids(images, prompts, max_tokens=TOKENS, ignore_eos=True, temperature=TEMPERATURE, top_p=TOP_P,
                                        generator=gen, **kw)

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
    logits = (torch.randn(B, VOCAB, generator=gen) * 3.0).to(torch.bfloat16).cuda()
    f32 = lambda v: torch.full((B,), v, dtype=torch.float32, device="cuda")
    t, p, u = f32(TEMPERATURE), f32(TOP_P), torch.rand(B, generator=gen).cuda()
    nxt = torch.zeros(B, dtype=torch.int32, device="cuda")

    def plain():
        return lib.md_sample_rows(logits.data_ptr(), VOCAB, B, VOCAB, -1, t.data_ptr(), p.data_ptr(), u.data_ptr(), nxt.data_ptr(),
                                  None, 0, stream)

    def filtered(k, m):
        kd, md = torch.full((B,), k, dtype=torch.int32, device="cuda"), f32(m)
        return lambda: lib.md_sample_rows_filtered(logits.data_ptr(), VOCAB, B, VOCAB, -1, t.data_ptr(), p.data_ptr(), kd.data_ptr(),
                                                   md.data_ptr(), u.data_ptr(), nxt.data_ptr(), None, 0, stream)

    def window(launch, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            _lib.check(launch(), "launch")
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / n

    out = {}
    cases = {"md_sample_rows": plain, "filtered_neutral": filtered(0, 0.0), "filtered_top_k": filtered(TOP_K, 0.0),
             "filtered_min_p": filtered(0, MIN_P), "filtered_both": filtered(TOP_K, MIN_P)}
    for launch in cases.values():
        window(launch, 50)  # warm-up
    per = {name: [] for name in cases}
    for _ in range(args.repeats):  # the cases alternate window by window
        for name, launch in cases.items():
            per[name].append(window(launch, args.launches))
    for name, us in per.items():
        out[name] = {"us_per_launch_median": round(statistics.median(us), 2), "us_per_launch_all": [round(x, 2) for x in us]}
    out.update(rows=B, vocab=VOCAB, temperature=TEMPERATURE, top_p=TOP_P, launches_per_window=args.launches)
    print(json.dumps(out))


def child(argv, repo=None, timeout=900):
    """A fresh process of this file (``repo``: the tree its moondream_amd comes from); its last stdout line as JSON."""
    env = dict(os.environ, MD_BENCH_FILTERS_REPO=repo or REPO)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), *argv], env=env, stdout=subprocess.PIPE, timeout=timeout)
    if r.returncode != 0:
        raise SystemExit(f"worker {argv} failed with status {r.returncode}")
    line = r.stdout.decode().strip().splitlines()[-1]
    print(f"[bench_sampling_filters] {' '.join(argv[:4])}: {line}", file=sys.stderr, flush=True)
    return json.loads(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="2b")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--launches", type=int, default=500)
    ap.add_argument("--parent-repo", default=None, help="a built checkout of the parent commit (the arguments-absent leg)")
    ap.add_argument("--skip-generation", action="store_true", help="the kernel part only")
    ap.add_argument("--worker", choices=("generation", "kernel"))
    ap.add_argument("--leg", choices=LEGS + ("absent",), default="off")
    args = ap.parse_args()
    sys.path.insert(0, os.environ.get("MD_BENCH_FILTERS_REPO", REPO))
    if args.worker:
        import torch

        with torch.inference_mode():
            {"generation": worker_generation, "kernel": worker_kernel}[args.worker](args)
        return

    result = {"metric": "sampling_filters_bench", "model": args.model, "batch": B, "tokens": TOKENS, "procs": args.procs,
              "repeats": args.repeats, "settings": dict(temperature=TEMPERATURE, top_p=TOP_P, top_k=TOP_K, min_p=MIN_P)}
    if not args.skip_generation:
        common = ["--model", args.model, "--seed", str(args.seed), "--repeats", str(args.repeats)]
        legs = ["off"] + (["absent"] if args.parent_repo else []) + list(LEGS[1:])
        runs = {leg: [] for leg in legs}
        for _ in range(args.procs):  # alternate the legs: drift of the machine lands on all of them
            for leg in legs:
                runs[leg].append(child(["--worker", "generation", "--leg", leg, *common], args.parent_repo if leg == "absent" else None))
        gen = {}
        for leg in legs:
            v, d = [r["images_per_s"] for r in runs[leg]], [r["decode_ms_per_step"] for r in runs[leg]]
            gen["parent" if leg == "absent" else leg] = {
                "images_per_s_median": statistics.median(v), "images_per_s_span": [min(v), max(v)], "images_per_s_all": v,
                "decode_ms_per_step_median": statistics.median(d), "decode_ms_per_step_all": d}
        assert len({r["ids_crc"] for r in runs["off"] + runs.get("absent", [])}) == 1, "the neutral call's ids differ from the parent's"
        off = gen["off"]["decode_ms_per_step_median"]
        for leg in LEGS[1:]:
            extra = gen[leg]["decode_ms_per_step_median"] - off
            gen[leg]["added_us_per_step"] = round(extra * 1e3, 1)
            gen[leg]["images_per_s_vs_off"] = round(gen[leg]["images_per_s_median"] / gen["off"]["images_per_s_median"], 4)
        if args.parent_repo:
            lo, hi = gen["parent"]["images_per_s_span"]
            gen["off_within_parent_span"] = lo <= gen["off"]["images_per_s_median"] <= hi
            gen["off_vs_parent"] = round(gen["off"]["images_per_s_median"] / gen["parent"]["images_per_s_median"], 4)
        result["generation"] = gen
    result["kernel"] = child(["--worker", "kernel", "--seed", str(args.seed), "--repeats", str(args.repeats), "--launches", str(args.launches)])
    line = json.dumps(result)
    with open(os.path.join(REPO, "profiles", "sampling_filters_bench.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
