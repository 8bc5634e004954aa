"""What stop strings / stop token ids cost and save (2B, bf16, compile()).  Prints one JSON line, also written to
profiles/stop_bench.json.

  kernel       md_stop_rows alone over 64 rows and a synthetic vocabulary of 51200 tokens, every row with a stop set that
               never matches (so every launch walks its whole token): stop sets of 1 and of 16 strings at tokens of 4 bytes,
               and 16 strings at the vocabulary's longest token (48 bytes) -- microseconds per launch from device events
               around ``--launches`` back-to-back launches, the median of ``--repeats`` such windows.  This is the figure
               for the kernel's mapping (one thread per row, one wave per 64 rows): measured here, not assumed.
  generation   B = 64 synthetic images, the caption prompt, greedy, 32 tokens with ``ignore_eos``: ``batch_generate_ids``
               with stops off (the call without the arguments) and with a never-matching stop set on all rows -- what the
               feature costs per step -- each in ``--procs`` fresh processes that alternate; per process the median of
               ``--repeats`` timed calls after a warm-up (graph captures), per leg the median and the span of the process
               medians; ms per decode step from device events (``collect_timing``).  With ``--parent-repo DIR`` (a built
               checkout of the parent commit) a third leg runs that tree's ``batch_generate_ids``, which has no such
               arguments: ``off_within_parent_span`` says whether the off median lies inside the parent's span.
  engine       ``ContinuousEngine`` (max_live 16) over 64 requests of 4 .. 64 tokens with ``ignore_eos``, without stops and
               with a stop id per request taken from its own free output (its 3rd token, so every request ends early):
               requests/s and ``stats.decode_steps`` of both.

  python tools/bench_stop.py [--parent-repo DIR] [--skip-generation] [--skip-engine]
A leg that is skipped is absent from the JSON: no figure is claimed for it.
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
B, TOKENS, VOCAB, LONGEST = 64, 32, 51200, 48
NEVER = ["\x01never\x02%d" % i for i in range(16)]  # bytes no synthetic token spells


def synthetic_vocab(seed):
    """VOCAB tokens over lower-case letters: id v < 1024 spells 4 bytes, id 1024 the longest token, the rest 1 .. 12 bytes."""
    import numpy as np

    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 13, size=VOCAB)
    lens[:1024], lens[1024] = 4, LONGEST
    return [bytes(rng.integers(97, 123, size=int(n)).astype(np.uint8)) for n in lens]


def worker_generation(args):
    """One process, one leg: off / never (a never-matching stop set on all rows), or absent (a tree without the arguments)."""
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
    if args.leg == "never":
        vocab = [b"t%d" % v for v in range(cfg.text.vocab_size)]
        kw = dict(stop=NEVER[:4], vocab_bytes=vocab)
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

    from moondream_amd import _lib, grammar
    from moondream_amd.stop import StopSet, pack, padded

    lib = _lib.load()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    vocab = synthetic_vocab(args.seed)
    off, data = grammar.vocab_arrays(vocab)
    d_off, d_bytes = dev(off), dev(data.copy())
    rng = np.random.default_rng(args.seed)
    out = {}
    for name, n_strings, tokens in (("strings_1_token_4_bytes", 1, rng.integers(0, 1024, size=B)),
                                    ("strings_16_token_4_bytes", 16, rng.integers(0, 1024, size=B)),
                                    (f"strings_16_token_{LONGEST}_bytes", 16, np.full(B, 1024))):
        trans, match_len, match_id, cap = padded(pack([StopSet(NEVER[:n_strings])]))
        d_table = dev(trans.view(np.int16)), dev(match_len.view(np.int16)), dev(match_id)
        d_ptr, d_ids, d_base = dev(np.zeros(B + 1, dtype=np.int32)), dev(np.full(1, -1, dtype=np.int32)), dev(np.full(B, n_strings, dtype=np.int32))
        words = np.zeros((6, B), dtype=np.int32)
        words[3], words[5] = -1, -1
        d_words, d_tok = dev(words), dev(tokens.astype(np.int32))

        def window(n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            d_words[1:3].zero_()  # the counters start over: they never overflow however many windows run
            e0.record()
            for _ in range(n):
                _lib.check(lib.md_stop_rows(d_tok.data_ptr(), B, None, 0, *(t.data_ptr() for t in d_table), cap, d_ptr.data_ptr(),
                                            d_ids.data_ptr(), d_base.data_ptr(), d_off.data_ptr(), d_bytes.data_ptr(), VOCAB,
                                            int(off[-1]), *(d_words[i].data_ptr() for i in range(6)), stream), "md_stop_rows")
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e3 / n

        window(50)  # warm-up
        us = [window(args.launches) for _ in range(args.repeats)]
        assert int((d_words[3] >= 0).sum()) == 0, "a never-matching stop set matched"
        out[name] = {"us_per_launch_median": round(statistics.median(us), 2), "us_per_launch_all": [round(u, 2) for u in us],
                     "dfa_states": int(cap)}
    out.update(rows=B, vocab=VOCAB, launches_per_window=args.launches, rows_per_workgroup=64)
    print(json.dumps(out))


def worker_engine(args):
    import numpy as np
    import torch

    from moondream_amd import synth
    from moondream_amd.config import get_config
    from moondream_amd.continuous import ContinuousEngine
    from moondream_amd.moondream import IdTokenizer, MoondreamModel

    cfg = get_config(args.model)
    sd = synth.synthetic_state_dict(cfg, seed=args.seed, device="cuda")
    model = MoondreamModel(cfg, sd, device="cuda", tokenizer=IdTokenizer(), max_batch=16)
    model.compile()
    n = 64
    images = [synth.synthetic_image(i, args.seed) for i in range(n)]
    prompts = [cfg.tokenizer.templates["caption"]["normal"]] * n
    mt = np.random.default_rng(args.seed).integers(4, 65, size=n).tolist()
    eng = ContinuousEngine(model, max_live=16)
    free = eng.generate(images, prompts, max_tokens=mt, ignore_eos=True)  # warm-up: graph captures; and the stop ids' source
    stop_ids = [[r[2]] for r in free]
    out = {}
    for leg, kw in (("none", {}), ("stops", dict(stop_token_ids=stop_ids))):
        eng.generate(images, prompts, max_tokens=mt, ignore_eos=True, **kw)  # this leg's captures
        times = []
        for _ in range(args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ids = eng.generate(images, prompts, max_tokens=mt, ignore_eos=True, **kw)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        out[leg] = {"requests_per_s": round(n / statistics.median(times), 2), "run_s_all": [round(t, 4) for t in times],
                    "decode_steps": eng.stats.decode_steps, "tokens": sum(len(r) for r in ids)}
    out.update(requests=n, max_live=16, max_tokens="4..64")
    print(json.dumps(out))


def child(argv, repo=None, timeout=900):
    """A fresh process of this file (``repo``: the tree its moondream_amd comes from); its last stdout line as JSON."""
    env = dict(os.environ, MD_BENCH_STOP_REPO=repo or REPO)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), *argv], env=env, stdout=subprocess.PIPE, timeout=timeout)
    if r.returncode != 0:
        raise SystemExit(f"worker {argv} failed with status {r.returncode}")
    line = r.stdout.decode().strip().splitlines()[-1]
    print(f"[bench_stop] {' '.join(argv[:4])}: {line}", file=sys.stderr, flush=True)
    return json.loads(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="2b")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--launches", type=int, default=500)
    ap.add_argument("--parent-repo", default=None, help="a built checkout of the parent commit (the arguments-absent leg)")
    ap.add_argument("--skip-generation", action="store_true")
    ap.add_argument("--skip-engine", action="store_true")
    ap.add_argument("--worker", choices=("generation", "kernel", "engine"))
    ap.add_argument("--leg", choices=("off", "never", "absent"), default="off")
    args = ap.parse_args()
    sys.path.insert(0, os.environ.get("MD_BENCH_STOP_REPO", REPO))
    if args.worker:
        import torch

        with torch.inference_mode():
            {"generation": worker_generation, "kernel": worker_kernel, "engine": worker_engine}[args.worker](args)
        return

    common = ["--model", args.model, "--seed", str(args.seed), "--repeats", str(args.repeats)]
    result = {"metric": "stop_bench", "model": args.model, "batch": B, "tokens": TOKENS, "procs": args.procs, "repeats": args.repeats}
    result["kernel"] = child(["--worker", "kernel", "--seed", str(args.seed), "--repeats", str(args.repeats), "--launches", str(args.launches)])
    if not args.skip_generation:
        legs = ["off", "never"] + (["absent"] if args.parent_repo else [])
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
        assert len({r["ids_crc"] for r in runs["off"] + runs["never"] + runs.get("absent", [])}) == 1, "a leg's ids differ"
        extra = gen["never"]["decode_ms_per_step_median"] - gen["off"]["decode_ms_per_step_median"]
        gen["never"]["added_us_per_step"] = round(extra * 1e3, 1)
        gen["never"]["images_per_s_vs_off"] = round(gen["never"]["images_per_s_median"] / gen["off"]["images_per_s_median"], 4)
        if args.parent_repo:
            lo, hi = gen["parent"]["images_per_s_span"]
            gen["off_within_parent_span"] = lo <= gen["off"]["images_per_s_median"] <= hi
            gen["off_vs_parent"] = round(gen["off"]["images_per_s_median"] / gen["parent"]["images_per_s_median"], 4)
        result["generation"] = gen
    if not args.skip_engine:
        result["engine"] = child(["--worker", "engine", *common])
    line = json.dumps(result)
    os.makedirs(os.path.join(REPO, "profiles"), exist_ok=True)
    with open(os.path.join(REPO, "profiles", "stop_bench.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
