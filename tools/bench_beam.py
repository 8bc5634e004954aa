"""What beam search costs (2B, bf16, compile()).  Prints one JSON line, also written to profiles/beam_bench.json.

  generation   16 synthetic images, the caption prompt, ``num_beams=4`` (64 beam rows), 32 tokens with ``ignore_eos``:
               ``batch_beam_search_ids`` against plain greedy ``batch_generate_ids`` over B = 64 run to the same number
               of decode steps -- the step cost without select and copy -- each in ``--procs`` fresh processes that
               alternate (beam, greedy, [parent,] beam, ..); per process the median of ``--repeats`` timed calls after a
               warm-up (graph captures), per leg the median and the span of the process medians.  Each call's decode
               phase is timed with device events (``collect_timing``): ms per decode step; the beam leg is reported as
               requests/s and as the microseconds a step gained over the greedy leg.  With ``--parent-repo DIR`` (a built
               checkout of the parent commit) one more leg runs that tree's greedy call: ``greedy_within_parent_span``
               says whether the greedy median lies inside the parent's span.  ``--skip-generation`` leaves this part out.
  kernel       per-launch medians at 64 rows of the 2B cache layout (24 layers, 32 heads, context 2048): md_beam_select
               (16 requests x 4 beams over 51200 logits) and md_kv_copy_tail with tails of 16 and 32 tokens, every row
               moving, every second row moving and one row moving (a child that continues its own beam is a skipped copy), from device
               events around ``--launches`` back-to-back launches, the median of ``--repeats`` such windows, all from the
               same process.

  python tools/bench_beam.py [--parent-repo DIR] [--skip-generation]
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
REQUESTS, BEAMS, TOKENS, VOCAB = 16, 4, 32, 51200
ROWS = REQUESTS * BEAMS
STEPS = TOKENS - 1  # decode steps of a beam call of TOKENS tokens: the first decision is the prompt pass's
LEGS = ("beam", "greedy")


def worker_generation(args):
    """One process, one leg: beam, greedy, or parent (the greedy call in a tree without beam search)."""
    import torch

    from moondream_amd import synth
    from moondream_amd.config import get_config
    from moondream_amd.moondream import IdTokenizer, MoondreamModel

    beam = args.leg == "beam"
    n = REQUESTS if beam else ROWS
    cfg = get_config(args.model)
    sd = synth.synthetic_state_dict(cfg, seed=args.seed, device="cuda")
    model = MoondreamModel(cfg, sd, device="cuda", tokenizer=IdTokenizer(), max_batch=REQUESTS * (1 + 2 * BEAMS) if beam else ROWS)
    model.compile()
    model.collect_timing = True
    images = [synth.synthetic_image(i, args.seed) for i in range(n)]
    prompts = [cfg.tokenizer.templates["caption"]["normal"]] * n

    def run():
        if beam:
            return [h[0].ids for h in model.batch_beam_search_ids(images, prompts, BEAMS, max_tokens=TOKENS, ignore_eos=True)]
        return model.batch_generate_ids(images, prompts, max_tokens=STEPS, ignore_eos=True)  # STEPS decode steps

    ids = run()  # warm-up: graph captures
    times, decode = [], []
    for _ in range(args.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
        decode.append(model.last_phase_ms["decode"])
    print(json.dumps({"leg": args.leg, "per_s": round(n / statistics.median(times), 2),
                      "decode_ms_per_step": round(statistics.median(decode) / STEPS, 4),
                      "run_s_all": [round(t, 4) for t in times], "ids_crc": hash(tuple(map(tuple, ids))) & 0xFFFFFFFF}))


def worker_kernel(args):
    import numpy as np
    import torch

    from moondream_amd import _lib

    lib = _lib.load()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def window(launch, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            _lib.check(launch(), "launch")
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / n

    # ---- md_beam_select: nothing ever finishes (eos -1), so every launch does the whole work on the state the last one left
    gen = torch.Generator().manual_seed(args.seed)
    logits = (torch.randn(ROWS, VOCAB, generator=gen) * 3.0).to(torch.bfloat16).cuda()
    own = (REQUESTS + 2 * np.arange(ROWS, dtype=np.int32)[:, None] + np.arange(2, dtype=np.int32)[None, :]).astype(np.int32)
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device="cuda")
    f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device="cuda")
    st_t = dict(cum=f32(ROWS), cur=dev(own[:, 0]), own=dev(own), len=i32(REQUESTS), done=i32(REQUESTS),
                prefix_len=i32(REQUESTS) + 735, pool_n=i32(REQUESTS), pool_score=f32(ROWS), pool_sum=f32(ROWS),
                pool_parent=i32(ROWS), pool_step=i32(ROWS), inv_norm=torch.ones(64, dtype=torch.float32, device="cuda"))
    cand_ids, cand_lp = i32(ROWS, 2 * BEAMS), f32(ROWS, 2 * BEAMS)
    st = _lib.MdBeamState(*(t.data_ptr() for t in st_t.values()), 64, cand_ids.data_ptr(), cand_lp.data_ptr())
    outs = [i32(ROWS) for _ in range(6)]

    def select():
        return lib.md_beam_select(logits.data_ptr(), VOCAB, REQUESTS, BEAMS, BEAMS, VOCAB, 3, None, -1, 0, C.byref(st),
                                  *(t.data_ptr() for t in outs), stream)

    # ---- md_kv_copy_tail over slabs of the 2B layout: row r moves slot 2r -> 2r + 1 (src and dst sets disjoint)
    layers, heads, ctx, n_slots = 24, 32, 2048, 2 * ROWS
    bs = heads * ctx * 64
    k = torch.empty(layers * n_slots * bs, dtype=torch.bfloat16, device="cuda")
    v = torch.empty_like(k)
    kv = _lib.MdKvCache(k.data_ptr(), v.data_ptr(), n_slots * bs, bs, ctx)

    def copy(tail, every):
        src = dev(2 * np.arange(ROWS, dtype=np.int32))
        dst = dev(np.where(np.arange(ROWS) % every == 0, 2 * np.arange(ROWS) + 1, 2 * np.arange(ROWS)).astype(np.int32))
        frm, to = i32(ROWS) + 735, i32(ROWS) + 735 + tail
        keep = (src, dst, frm, to)
        return lambda: lib.md_kv_copy_tail(C.byref(kv), layers, heads, n_slots, ROWS, *(t.data_ptr() for t in keep), stream)

    cases = {"md_beam_select": select, "kv_copy_tail16_all": copy(16, 1), "kv_copy_tail16_half": copy(16, 2),
             "kv_copy_tail32_all": copy(32, 1), "kv_copy_tail32_half": copy(32, 2), "kv_copy_tail16_one_row": copy(16, 10 ** 6)}
    for launch in cases.values():
        window(launch, 20)  # warm-up
    per = {name: [] for name in cases}
    for _ in range(args.repeats):  # the cases alternate window by window
        for name, launch in cases.items():
            per[name].append(window(launch, args.launches))
    out = {name: {"us_per_launch_median": round(statistics.median(us), 2), "us_per_launch_all": [round(x, 2) for x in us]}
           for name, us in per.items()}
    moved = lambda tail, rows: rows * tail * layers * 2 * heads * 64 * 2  # bytes read (and as many written)
    for name, tail, rows in (("kv_copy_tail16_all", 16, ROWS), ("kv_copy_tail32_all", 32, ROWS)):
        out[name]["gb_per_s_read_plus_write"] = round(2 * moved(tail, rows) / out[name]["us_per_launch_median"] / 1e3, 1)
    out.update(rows=ROWS, requests=REQUESTS, num_beams=BEAMS, vocab=VOCAB, layers=layers, heads=heads, ctx=ctx,
               launches_per_window=args.launches)
    print(json.dumps(out))


def child(argv, repo=None, timeout=1500):
    """A fresh process of this file (``repo``: the tree its moondream_amd comes from); its last stdout line as JSON."""
    env = dict(os.environ, MD_BENCH_BEAM_REPO=repo or REPO)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), *argv], env=env, stdout=subprocess.PIPE, timeout=timeout)
    if r.returncode != 0:
        raise SystemExit(f"worker {argv} failed with status {r.returncode}")
    line = r.stdout.decode().strip().splitlines()[-1]
    print(f"[bench_beam] {' '.join(argv[:4])}: {line}", file=sys.stderr, flush=True)
    return json.loads(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="2b")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--parent-repo", default=None, help="a built checkout of the parent commit (its greedy leg)")
    ap.add_argument("--skip-generation", action="store_true", help="the kernel part only")
    ap.add_argument("--worker", choices=("generation", "kernel"))
    ap.add_argument("--leg", choices=LEGS + ("parent",), default="beam")
    args = ap.parse_args()
    sys.path.insert(0, os.environ.get("MD_BENCH_BEAM_REPO", REPO))
    if args.worker:
        import torch

        with torch.inference_mode():
            {"generation": worker_generation, "kernel": worker_kernel}[args.worker](args)
        return

    result = {"metric": "beam_bench", "model": args.model, "requests": REQUESTS, "num_beams": BEAMS, "tokens": TOKENS,
              "decode_steps": STEPS, "procs": args.procs, "repeats": args.repeats}
    if not args.skip_generation:
        common = ["--model", args.model, "--seed", str(args.seed), "--repeats", str(args.repeats)]
        legs = list(LEGS) + (["parent"] if args.parent_repo else [])
        runs = {leg: [] for leg in legs}
        for _ in range(args.procs):  # alternate the legs: drift of the machine lands on all of them
            for leg in legs:
                runs[leg].append(child(["--worker", "generation", "--leg", leg, *common], args.parent_repo if leg == "parent" else None))
        gen = {}
        for leg in legs:
            v, d = [r["per_s"] for r in runs[leg]], [r["decode_ms_per_step"] for r in runs[leg]]
            unit = "requests_per_s" if leg == "beam" else "images_per_s"
            gen[leg] = {unit + "_median": statistics.median(v), unit + "_span": [min(v), max(v)], unit + "_all": v,
                        "decode_ms_per_step_median": statistics.median(d), "decode_ms_per_step_all": d}
        assert len({r["ids_crc"] for r in runs["greedy"] + runs.get("parent", [])}) == 1, "the greedy ids differ from the parent's"
        gen["beam"]["added_us_per_step"] = round((gen["beam"]["decode_ms_per_step_median"] - gen["greedy"]["decode_ms_per_step_median"]) * 1e3, 1)
        if args.parent_repo:
            lo, hi = gen["parent"]["images_per_s_span"]
            gen["greedy_within_parent_span"] = lo <= gen["greedy"]["images_per_s_median"] <= hi
            gen["greedy_vs_parent"] = round(gen["greedy"]["images_per_s_median"] / gen["parent"]["images_per_s_median"], 4)
        result["generation"] = gen
    result["kernel"] = child(["--worker", "kernel", "--seed", str(args.seed), "--repeats", str(args.repeats), "--launches", str(args.launches)])
    line = json.dumps(result)
    with open(os.path.join(REPO, "profiles", "beam_bench.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
