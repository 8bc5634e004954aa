"""What spatial references in the batched queries cost and save (2B, bf16, compile()).  Prints one JSON line, also written to
profiles/spatial_refs_bench.json.

  queries      ONE synthetic image, 64 boxes, one question about each, greedy, 16 tokens:
                 many        ``query_many(image, questions, settings={"spatial_refs": boxes})``: one batch over one copy of
                             the image's prefix, every reference token encoded by one md_spatial_ref_embed launch;
                 sequential  the same 64 as ``query(image, question, spatial_refs=[box])`` calls on the image's EncodedImage;
                 norefs      ``batch_query`` over 64 images without refs, and with ``--parent-repo DIR`` (a built checkout of
                             the parent commit) the same call on that tree (``parent``): ``norefs_within_parent_span`` says
                             whether the no-refs median lies inside the parent's own span.
               Each leg in ``--procs`` fresh processes that alternate; per process the median of ``--repeats`` timed calls
               after a warm-up, per leg the median and the span of the process medians.  ``--skip-queries`` leaves this out.
  kernel       md_spatial_ref_embed over 192 tokens (64 boxes: 128 coordinates, 64 sizes) at 2B's dimensions, beside the
               launches it replaces (md_fourier_features and md_gemm_bf16, once per kind): microseconds per launch from
               device events around ``--launches`` back-to-back launches, the median of ``--repeats`` windows.

  python tools/bench_spatial_refs.py [--parent-repo DIR] [--skip-queries]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time
import zlib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, TOKENS = 64, 16
LEGS = ("many", "sequential", "norefs")


def boxes(n):
    return [[((i % 8) / 10, (i // 8) / 10, (i % 8) / 10 + 0.2, (i // 8) / 10 + 0.25)] for i in range(n)]


def worker_queries(args):
    import torch

    from moondream_amd import synth
    from moondream_amd.config import get_config
    from moondream_amd.moondream import IdTokenizer, MoondreamModel

    cfg = get_config(args.model)
    sd = synth.synthetic_state_dict(cfg, seed=args.seed, device="cuda")
    model = MoondreamModel(cfg, sd, device="cuda", tokenizer=IdTokenizer(), max_batch=B)
    model.compile()
    st = {"temperature": 0, "max_tokens": TOKENS}
    questions = [f"{11 + i % 5} 12 13" for i in range(B)]
    refs = boxes(B)
    if args.leg == "many":
        image = synth.synthetic_image(0, args.seed)
        run = lambda: model.query_many(image, questions, settings={**st, "spatial_refs": refs})
    elif args.leg == "sequential":
        enc = model.encode_image(synth.synthetic_image(0, args.seed))
        run = lambda: [model.query(enc, q, spatial_refs=r, settings=st) for q, r in zip(questions, refs)]
    else:  # norefs / absent: the call every tree has
        images = [synth.synthetic_image(i, args.seed) for i in range(B)]
        run = lambda: model.batch_query(images, questions, settings=st)
    out = run()  # warm-up: graph captures
    times = []
    for _ in range(args.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    print(json.dumps({"leg": args.leg, "queries_per_s": round(B / statistics.median(times), 2),
                      "run_s_all": [round(t, 4) for t in times], "out_crc": zlib.crc32(repr(out).encode())}))


def worker_kernel(args):
    import torch

    from moondream_amd import _lib
    from moondream_amd.weights import PackedLinear

    lib = _lib.load()
    gen = torch.Generator().manual_seed(args.seed)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    bf = torch.bfloat16
    dim, cf, sf, n_box = 2048, 256, 512, B
    r = lambda *s, scale=1.0: (torch.randn(*s, generator=gen) * scale).to(bf)
    cfw, sfw = r(1, cf // 2, scale=10.0).cuda(), r(2, sf // 2, scale=10.0).cuda()
    ce, se = PackedLinear(r(dim, cf, scale=cf ** -0.5), r(dim, scale=0.1), "cuda"), PackedLinear(r(dim, sf, scale=sf ** -0.5), r(dim, scale=0.1), "cuda")
    cv, sv = torch.rand(2 * n_box, 1, generator=gen).to(bf).cuda(), torch.rand(n_box, 2, generator=gen).to(bf).cuda()
    # the table of 64 boxes: [coord, coord, size] each, at rows 3 .. 5 of 64 prompts of 12 positions
    t_len, rows = 12, []
    cb, sb = cv.cpu().view(torch.int16).int() & 0xFFFF, sv.cpu().view(torch.int16).int() & 0xFFFF
    for i in range(n_box):
        rows += [[i * t_len + 3, 0, int(cb[2 * i]), 0], [i * t_len + 4, 0, int(cb[2 * i + 1]), 0], [i * t_len + 5, 1, int(sb[i, 0]), int(sb[i, 1])]]
    desc = torch.tensor(rows, dtype=torch.int32).cuda()
    emb = torch.zeros(n_box * t_len, dim, dtype=bf, device="cuda")

    def fused():
        return lib.md_spatial_ref_embed(desc.data_ptr(), desc.shape[0], cfw.data_ptr(), cf, ce.w.data_ptr(), ce.k_pad, ce.b.data_ptr(),
                                        sfw.data_ptr(), sf, se.w.data_ptr(), se.k_pad, se.b.data_ptr(), dim, emb.data_ptr(), dim, 0,
                                        emb.shape[0], stream)

    cfeat, sfeat = torch.empty(2 * n_box, cf, dtype=bf, device="cuda"), torch.empty(n_box, sf, dtype=bf, device="cuda")
    cout, sout = torch.empty(2 * n_box, dim, dtype=bf, device="cuda"), torch.empty(n_box, dim, dtype=bf, device="cuda")
    need = max(lib.md_gemm_workspace_bytes(C.byref(lin.struct()), 64, 1) for lin in (ce, se))
    ws = torch.zeros(max(need, 16), dtype=torch.uint8, device="cuda")

    def gemm(a, lin, out):
        g = _lib.MdGemmArgs(a.data_ptr(), lin.k_pad, lin.struct(), out.data_ptr(), lin.n_pad, None, 0, 0, a.shape[0], _lib.MD_EPI_BIAS,
                            1, 0, ws.data_ptr(), ws.numel(), _lib.MD_TILE_BY_SHAPE)
        return lib.md_gemm_bf16(C.byref(g), stream)

    def replaced():  # what _prefill_prompt launches for the same tokens (without its mask assignments)
        st = lib.md_fourier_features(cv.data_ptr(), 1, 2 * n_box, 1, cfw.data_ptr(), cf // 2, cfeat.data_ptr(), cf, stream)
        st |= gemm(cfeat, ce, cout)
        st |= lib.md_fourier_features(sv.data_ptr(), 2, n_box, 2, sfw.data_ptr(), sf // 2, sfeat.data_ptr(), sf, stream)
        return st | gemm(sfeat, se, sout)

    def window(launch, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            _lib.check(launch(), "launch")
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / n

    cases = {"md_spatial_ref_embed": fused, "fourier_and_gemm_x2": replaced}
    for launch in cases.values():
        window(launch, 50)  # warm-up
    per = {name: [] for name in cases}
    for _ in range(args.repeats):  # the cases alternate window by window
        for name, launch in cases.items():
            per[name].append(window(launch, args.launches))
    out = {name: {"us_median": round(statistics.median(us), 2), "us_all": [round(x, 2) for x in us]} for name, us in per.items()}
    same = bool(((emb.view(n_box, t_len, dim)[:, 3:5].reshape(-1, dim).float() - cout.float()).abs().max() < 0.1).item())
    out.update(tokens=desc.shape[0], dim=dim, launches_per_window=args.launches, launches_replaced=4, agree_with_gemm_path=same)
    print(json.dumps(out))


def child(argv, repo=None, timeout=1200):
    """A fresh process of this file (``repo``: the tree its moondream_amd comes from); its last stdout line as JSON."""
    env = dict(os.environ, MD_BENCH_SPATIAL_REPO=repo or REPO)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), *argv], env=env, stdout=subprocess.PIPE, timeout=timeout)
    if r.returncode != 0:
        raise SystemExit(f"worker {argv} failed with status {r.returncode}")
    line = r.stdout.decode().strip().splitlines()[-1]
    print(f"[bench_spatial_refs] {' '.join(argv[:4])}: {line}", file=sys.stderr, flush=True)
    return json.loads(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="2b")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--launches", type=int, default=500)
    ap.add_argument("--parent-repo", default=None, help="a built checkout of the parent commit (the no-refs call on that tree)")
    ap.add_argument("--skip-queries", action="store_true", help="the kernel part only")
    ap.add_argument("--worker", choices=("queries", "kernel"))
    ap.add_argument("--leg", choices=LEGS + ("absent",), default="many")
    args = ap.parse_args()
    sys.path.insert(0, os.environ.get("MD_BENCH_SPATIAL_REPO", REPO))
    if args.worker:
        import torch

        with torch.inference_mode():
            {"queries": worker_queries, "kernel": worker_kernel}[args.worker](args)
        return

    result = {"metric": "spatial_refs_bench", "model": args.model, "batch": B, "tokens": TOKENS, "procs": args.procs,
              "repeats": args.repeats}
    if not args.skip_queries:
        common = ["--model", args.model, "--seed", str(args.seed), "--repeats", str(args.repeats)]
        legs = list(LEGS) + (["absent"] if args.parent_repo else [])
        runs = {leg: [] for leg in legs}
        for _ in range(args.procs):  # alternate the legs: drift of the machine lands on all of them
            for leg in legs:
                runs[leg].append(child(["--worker", "queries", "--leg", leg, *common], args.parent_repo if leg == "absent" else None))
        q = {}
        for leg in legs:
            v = [r["queries_per_s"] for r in runs[leg]]
            q["parent" if leg == "absent" else leg] = {"queries_per_s_median": statistics.median(v), "queries_per_s_span": [min(v), max(v)],
                                                       "queries_per_s_all": v}
        q["many_vs_sequential"] = round(q["many"]["queries_per_s_median"] / q["sequential"]["queries_per_s_median"], 3)
        if args.parent_repo:
            assert len({r["out_crc"] for r in runs["norefs"] + runs["absent"]}) == 1, "the no-refs call's answers differ from the parent's"
            lo, hi = q["parent"]["queries_per_s_span"]
            q["norefs_within_parent_span"] = lo <= q["norefs"]["queries_per_s_median"] <= hi
            q["norefs_vs_parent"] = round(q["norefs"]["queries_per_s_median"] / q["parent"]["queries_per_s_median"], 4)
        result["queries"] = q
    result["kernel"] = child(["--worker", "kernel", "--seed", str(args.seed), "--repeats", str(args.repeats), "--launches", str(args.launches)])
    line = json.dumps(result)
    with open(os.path.join(REPO, "profiles", "spatial_refs_bench.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
