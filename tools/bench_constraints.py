"""What constrained decoding costs (2B, bf16, compile()).  Prints one JSON line, also written to
profiles/constraints_bench.json.

  generation   B = 64 synthetic images, the caption prompt, greedy, 32 tokens with ``ignore_eos``: ``batch_generate_ids`` with
               constraints off (the call without the argument), all 64 rows under a 16-way ``choices`` trie (default-forbid
               states: the bitmap sweep), all 64 rows under ``banned_tokens`` of 8 ids (a default-allow state) and half the
               rows under the trie, each in ``--procs`` fresh processes that alternate (off, choices, banned, half,
               [parent,] off, ..); per process the median of ``--repeats`` timed calls after a warm-up (graph captures), per
               leg the median and the span of the process medians.  Beside images/s each call's decode phase is timed with
               device events (``collect_timing``): ms per decode step, and for the constrained legs what a step gained
               over the off leg and that as a share of the step.  A trie row is FREE once its choice and eos are out (at
               most 5 tokens), so the trie legs also run with every choice 32 tokens long (``choices_long``): every step masks.
               With ``--parent-repo DIR`` (a built checkout of the parent commit) one more leg runs that tree's
               ``batch_generate_ids``, which has no such argument: ``off_within_parent_span`` says whether the off median
               lies inside the parent's span.  No ratio is fixed in advance.
  kernel       md_constrain_rows alone over 64 rows of 51200 logits, every row in a default-forbid state of 16 allowed
               tokens, then every row in a default-allow state of 8 forbidden ones (tokens_in NULL: the states stay):
               microseconds per launch from device events around ``--launches`` back-to-back launches, the median of
               ``--repeats`` such windows.

  python tools/bench_constraints.py [--parent-repo DIR]
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
LEGS = ("off", "choices", "choices_long", "banned", "half")


def automaton(leg):
    """The leg's automaton (ids chosen away from the special tokens)."""
    from moondream_amd.constraint import TokenAutomaton

    if leg == "banned":
        return TokenAutomaton.banned_tokens(range(1000, 1008))
    n = TOKENS if leg == "choices_long" else 4
    return TokenAutomaton.choices([[2000 + 37 * c + 16 * j for j in range(n)] for c in range(16)], eos_id=0)


def worker_generation(args):
    """One process, one leg: off / choices / choices_long / banned / half, or absent (a tree without the argument)."""
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
    kw = {}
    if args.leg not in ("off", "absent"):
        a = automaton("choices_long" if args.leg == "half" else args.leg)
        kw = {"constraints": [a if args.leg != "half" or i % 2 == 0 else None for i in range(B)]}
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
    import numpy as np
    import torch

    from moondream_amd import _lib
    from moondream_amd.constraint import TokenAutomaton, pack

    lib = _lib.load()
    gen = torch.Generator().manual_seed(args.seed)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = {}
    kinds = {"default_forbid_16_allowed": TokenAutomaton.allowed_tokens(range(2000, 2000 + 16 * 37, 37)),
             "default_allow_8_forbidden": TokenAutomaton.banned_tokens(range(1000, 1008))}
    for name, a in kinds.items():
        t = pack([a])
        logits = (torch.randn(B, VOCAB, generator=gen) * 8.0).to(torch.bfloat16).cuda()
        table = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (t.row_ptr, t.default_next, t.edge_tok, t.edge_next)]
        state = torch.zeros(B, dtype=torch.int32, device="cuda")

        def window(n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                _lib.check(lib.md_constrain_rows(logits.data_ptr(), logits.stride(0), B, VOCAB, None, None, 0, state.data_ptr(),
                                                 *(x.data_ptr() for x in table), t.n_states, stream), "md_constrain_rows")
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e3 / n

        window(50)  # warm-up
        us = [window(args.launches) for _ in range(args.repeats)]
        out[name] = {"us_per_launch_median": round(statistics.median(us), 2), "us_per_launch_all": [round(u, 2) for u in us]}
    out.update(rows=B, vocab=VOCAB, launches_per_window=args.launches)
    print(json.dumps(out))


def child(argv, repo=None, timeout=900):
    """A fresh process of this file (``repo``: the tree its moondream_amd comes from); its last stdout line as JSON."""
    env = dict(os.environ, MD_BENCH_CONSTRAINTS_REPO=repo or REPO)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), *argv], env=env, stdout=subprocess.PIPE, timeout=timeout)
    if r.returncode != 0:
        raise SystemExit(f"worker {argv} failed with status {r.returncode}")
    line = r.stdout.decode().strip().splitlines()[-1]
    print(f"[bench_constraints] {' '.join(argv[:4])}: {line}", file=sys.stderr, flush=True)
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
    ap.add_argument("--leg", choices=LEGS + ("absent",), default="off")
    args = ap.parse_args()
    sys.path.insert(0, os.environ.get("MD_BENCH_CONSTRAINTS_REPO", REPO))
    if args.worker:
        import torch

        with torch.inference_mode():
            {"generation": worker_generation, "kernel": worker_kernel}[args.worker](args)
        return

    common = ["--model", args.model, "--seed", str(args.seed), "--repeats", str(args.repeats)]
    legs = list(LEGS) + (["absent"] if args.parent_repo else [])
    runs = {leg: [] for leg in legs}
    for _ in range(args.procs):  # alternate the legs: drift of the machine lands on all of them
        for leg in legs:
            runs[leg].append(child(["--worker", "generation", "--leg", leg, *common], args.parent_repo if leg == "absent" else None))
    result = {"metric": "constraints_bench", "model": args.model, "batch": B, "tokens": TOKENS, "procs": args.procs,
              "repeats": args.repeats}
    gen = {}
    for leg in legs:
        v, d = [r["images_per_s"] for r in runs[leg]], [r["decode_ms_per_step"] for r in runs[leg]]
        gen["parent" if leg == "absent" else leg] = {
            "images_per_s_median": statistics.median(v), "images_per_s_span": [min(v), max(v)], "images_per_s_all": v,
            "decode_ms_per_step_median": statistics.median(d), "decode_ms_per_step_all": d}
    assert len({r["ids_crc"] for r in runs["off"] + runs.get("absent", [])}) == 1, "the free call's ids differ from the parent's"
    off = gen["off"]["decode_ms_per_step_median"]
    for leg in LEGS[1:]:
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
    with open(os.path.join(REPO, "profiles", "constraints_bench.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
