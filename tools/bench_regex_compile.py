"""What compiling a regex or a JSON schema to a token automaton costs, and what serving it costs (2B, bf16, compile()).
Prints one JSON line, also written to profiles/regex_compile_bench.json.

  compile      three patterns over a synthetic vocabulary of 51200 tokens (the 256 single bytes and seeded strings over the
               characters of numbers and JSON): the integer regex ``-?[0-9]{1,3}(\\.[0-9]{1,2})?``, a 6-property JSON schema, and
               the largest schema of a family (an object of k bounded strings) whose DFA stays under 4096 states.  Per
               pattern: the host DFA construction (wall clock), then in one process ``--repeats`` compiles, each timed in its
               parts -- md_automaton_count (lift + histogram + scan) and md_automaton_fill (lift + compaction) with device
               events, the copy back and the host finish (pruning, ``from_arrays``) with the wall clock -- medians and spans;
               and tests/grammar_ref.py's numpy lift + compaction of the same DFA on the host, ``--host-repeats`` times
               (it is what a host implementation pays; the largest schema's may take minutes: ``--skip-host-largest``).
  generation   B = 64 synthetic images, the caption prompt, greedy, 32 tokens with ``ignore_eos``: ``batch_generate_ids`` with
               no constraint and with the 6-property schema's automaton on every row, in ``--procs`` fresh processes that
               alternate (off, schema, [parent,] off, ..); per process the median of ``--repeats`` timed calls after a
               warm-up.  With ``--parent-repo DIR`` (a built checkout of the parent commit) one more leg runs that tree's
               unconstrained call: ``off_within_parent_span`` says whether the off median lies inside the parent's span.
               No ratio is fixed in advance.

  python tools/bench_regex_compile.py [--parent-repo DIR]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, TOKENS, VOCAB, EOS = 64, 32, 51200, 0
INTEGER = r"-?[0-9]{1,3}(\.[0-9]{1,2})?"
SIX = {"type": "object", "required": ["label", "count", "score", "visible", "color", "box"], "properties": {
    "label": {"type": "string", "maxLength": 16}, "count": {"type": "integer"}, "score": {"type": "number"},
    "visible": {"type": "boolean"}, "color": {"enum": ["red", "green", "blue", None]},
    "box": {"type": "array", "items": {"type": "number"}, "minItems": 4, "maxItems": 4}}}


def strings_schema(k, length=24):
    return {"type": "object", "required": [f"f{i}" for i in range(k)],
            "properties": {f"f{i}": {"type": "string", "maxLength": length} for i in range(k)}}


def patterns():
    """name -> (pattern, DFA, seconds the host took for the DFA)."""
    from moondream_amd.grammar import MAX_STATES, json_schema_to_regex, regex_to_dfa

    def timed(p):
        t0 = time.perf_counter()
        d = regex_to_dfa(p)
        return p, d, time.perf_counter() - t0

    out = {"integer": timed(INTEGER), "schema6": timed(json_schema_to_regex(SIX))}
    best = None
    for k in range(1, 400):  # states grow by a constant per property: stop at the first k past the cap
        try:
            best = (k,) + timed(json_schema_to_regex(strings_schema(k)))
        except ValueError:
            break
        if best[2].n_states > MAX_STATES - 60:
            break
    out[f"largest_strings{best[0]}"] = best[1:]
    return out


def vocabulary(seed):
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import grammar_ref

    return grammar_ref, [b""] * 10 + grammar_ref.synthetic_vocab(VOCAB - 10, seed, longest=8)


def med(xs, nd=3):
    return {"median": round(statistics.median(xs), nd), "span": [round(min(xs), nd), round(max(xs), nd)], "n": len(xs)}


def worker_compile(args):
    import numpy as np
    import torch

    from moondream_amd import _lib
    from moondream_amd import grammar as G

    ref, vocab = vocabulary(args.seed)
    lib = _lib.load()
    tok_off, tok_bytes = G.vocab_arrays(vocab)
    forbidden = np.zeros(VOCAB, dtype=np.uint8)
    forbidden[1:10] = 1
    stream = torch.cuda.current_stream().cuda_stream
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    result = {}
    for name, (pattern, dfa, dfa_s) in patterns().items():
        s = dfa.n_states
        d = [up(dfa.trans), up(dfa.accept.astype(np.uint8)), up(tok_off), up(tok_bytes), up(forbidden)]
        common = (d[0].data_ptr(), d[1].data_ptr(), s, d[2].data_ptr(), d[3].data_ptr(), int(tok_bytes.shape[0]), VOCAB, EOS, d[4].data_ptr())
        ws_bytes = lib.md_automaton_workspace_bytes(s, VOCAB)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
        head = torch.empty(2 * s + 1, dtype=torch.int32, device="cuda")
        parts = {"count_ms": [], "fill_ms": [], "copy_back_ms": [], "host_finish_ms": [], "whole_compile_ms": []}
        for i in range(args.repeats + 1):  # the first pass is a warm-up
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            ev[0].record()
            _lib.check(lib.md_automaton_count(*common, head.data_ptr(), head[s:].data_ptr(), ws.data_ptr(), ws_bytes, stream))
            ev[1].record()
            n = int(head[2 * s].item())
            edges = torch.empty(2 * max(n, 1), dtype=torch.int32, device="cuda")
            ev[2].record()
            _lib.check(lib.md_automaton_fill(*common, head.data_ptr(), head[s:].data_ptr(), edges.data_ptr(), edges[max(n, 1):].data_ptr(), n,
                                             ws.data_ptr(), ws_bytes, stream))
            ev[3].record()
            ev[3].synchronize()
            t0 = time.perf_counter()
            host = torch.cat([head, edges]).cpu().numpy()
            t1 = time.perf_counter()
            arrays = (host[s : 2 * s + 1], host[:s], host[2 * s + 1 : 2 * s + 1 + n], host[2 * s + 1 + max(n, 1) : 2 * s + 1 + max(n, 1) + n])
            a = G.finish_automaton(dfa, arrays)
            t2 = time.perf_counter()
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            whole = G.compile_dfa(dfa, vocab, EOS, range(1, 10))
            t4 = time.perf_counter()
            assert whole.n_edges == a.n_edges
            if i:
                for k, x in zip(parts, (ev[0].elapsed_time(ev[1]), ev[2].elapsed_time(ev[3]), (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t4 - t3) * 1e3)):
                    parts[k].append(x)
        entry = {"dfa_states": s, "host_dfa_s": round(dfa_s, 3), "lift_edges": n, "automaton_states": a.n_states, "automaton_edges": a.n_edges}
        entry.update({k: med(v) for k, v in parts.items()})
        if not (args.skip_host_largest and name.startswith("largest")):
            host_s = []
            for _ in range(args.host_repeats):
                t0 = time.perf_counter()
                want = ref.compact(ref.lift(dfa.trans, dfa.accept, vocab, EOS, forbidden))
                host_s.append(time.perf_counter() - t0)
            assert all(np.array_equal(x, y) for x, y in zip(want, arrays)), "the device table differs from the host reference"
            entry["host_numpy_lift_s"] = med(host_s)
            entry["host_over_device"] = round(statistics.median(host_s) * 1e3 / (entry["count_ms"]["median"] + entry["fill_ms"]["median"]
                                                                                + entry["copy_back_ms"]["median"]), 1)
        result[name] = entry
    print(json.dumps(result))


def worker_generation(args):
    import torch

    from moondream_amd import synth
    from moondream_amd.config import get_config
    from moondream_amd.moondream import IdTokenizer, MoondreamModel

    cfg = get_config(args.model)
    sd = synth.synthetic_state_dict(cfg, seed=args.seed, device="cuda")
    model = MoondreamModel(cfg, sd, device="cuda", tokenizer=IdTokenizer(), max_batch=B)
    model.compile()
    images = [synth.synthetic_image(i, args.seed) for i in range(B)]
    prompts = [cfg.tokenizer.templates["caption"]["normal"]] * B
    kw = {}
    if args.leg == "schema":
        kw = {"constraints": model.json_constraint(SIX, vocabulary(args.seed)[1])}
    run = lambda: model.batch_generate_ids(images, prompts, max_tokens=TOKENS, ignore_eos=True, **kw)
    ids = run()  # warm-up: graph captures
    times = []
    for _ in range(args.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    print(json.dumps({"leg": args.leg, "images_per_s": round(B / statistics.median(times), 2), "run_s_all": [round(t, 4) for t in times],
                      "ids_crc": hash(tuple(map(tuple, ids))) & 0xFFFFFFFF}))


def child(argv, repo=None, timeout=1500):
    """A fresh process of this file (``repo``: the tree its moondream_amd comes from); its last stdout line as JSON."""
    env = dict(os.environ, MD_BENCH_REGEX_REPO=repo or REPO)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), *argv], env=env, stdout=subprocess.PIPE, timeout=timeout)
    if r.returncode != 0:
        raise SystemExit(f"worker {argv} failed with status {r.returncode}")
    line = r.stdout.decode().strip().splitlines()[-1]
    print(f"[bench_regex_compile] {' '.join(argv[:4])}: {line[:400]}", file=sys.stderr, flush=True)
    return json.loads(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="2b")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--skip-host-largest", action="store_true")
    ap.add_argument("--skip-generation", action="store_true")
    ap.add_argument("--parent-repo", default=None, help="a built checkout of the parent commit (the unconstrained leg)")
    ap.add_argument("--worker", choices=("compile", "generation"))
    ap.add_argument("--leg", choices=("off", "schema", "absent"), default="off")
    args = ap.parse_args()
    sys.path.insert(0, os.environ.get("MD_BENCH_REGEX_REPO", REPO))
    if args.worker:
        import torch

        with torch.inference_mode():
            {"compile": worker_compile, "generation": worker_generation}[args.worker](args)
        return

    common = ["--model", args.model, "--seed", str(args.seed), "--repeats", str(args.repeats)]
    result = {"metric": "regex_compile_bench", "model": args.model, "vocab": VOCAB, "repeats": args.repeats}
    result["compile"] = child(["--worker", "compile", *common, "--host-repeats", str(args.host_repeats)]
                              + (["--skip-host-largest"] if args.skip_host_largest else []))
    if not args.skip_generation:
        legs = ["off", "schema"] + (["absent"] if args.parent_repo else [])
        runs = {leg: [] for leg in legs}
        for _ in range(args.procs):  # alternate the legs: drift of the machine lands on all of them
            for leg in legs:
                runs[leg].append(child(["--worker", "generation", "--leg", "off" if leg == "absent" else leg, *common],
                                       args.parent_repo if leg == "absent" else None))
        gen = {}
        for leg in legs:
            v = [r["images_per_s"] for r in runs[leg]]
            gen["parent" if leg == "absent" else leg] = {"images_per_s_median": statistics.median(v), "images_per_s_span": [min(v), max(v)],
                                                         "images_per_s_all": v}
        assert len({r["ids_crc"] for r in runs["off"] + runs.get("absent", [])}) == 1, "the free call's ids differ from the parent's"
        gen["schema_vs_off"] = round(gen["schema"]["images_per_s_median"] / gen["off"]["images_per_s_median"], 4)
        if args.parent_repo:
            lo, hi = gen["parent"]["images_per_s_span"]
            gen["off_within_parent_span"] = lo <= gen["off"]["images_per_s_median"] <= hi
            gen["off_vs_parent"] = round(gen["off"]["images_per_s_median"] / gen["parent"]["images_per_s_median"], 4)
        result["generation"] = dict(gen, batch=B, tokens=TOKENS, procs=args.procs)
    line = json.dumps(result)
    with open(os.path.join(REPO, "profiles", "regex_compile_bench.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
