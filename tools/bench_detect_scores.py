"""What detection confidence costs (2B, bf16, compile()).  Prints one JSON line, also written to
profiles/detect_scores_bench.json.

  The ``detect13`` workload of bench.py's leg: B = 32 seeded 768 x 1024 images (13 crops each), ``batch_detect`` with the
  golden's ``max_objects`` and ``_run_all_objects`` (every row runs every round: the work is fixed), host tiling included.
  Legs: scores off (the call without the setting), ``return_scores`` at ``score_window`` 0 and at 8, and with
  ``--parent-repo DIR`` (a built checkout of the parent commit) that tree's call, which has no such setting.  Each leg runs in
  ``--procs`` fresh processes that alternate (off, w0, w8, [parent,] off, ..); per process the median of ``--repeats`` timed
  calls after a warm-up, per leg the median and the span of the process medians.  ``off_within_parent_span`` says whether
  the off median lies inside the parent's span.  The boxes of every leg must be the same (a CRC of the first call's).

  python tools/bench_detect_scores.py [--parent-repo DIR]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
import zlib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 32
LEGS = {"off": {}, "w0": {"return_scores": True}, "w8": {"return_scores": True, "score_window": 8}, "parent": {}}


def worker(args):
    import numpy as np
    import torch

    from moondream_amd import synth
    from moondream_amd.config import get_config
    from moondream_amd.moondream import IdTokenizer, MoondreamModel

    cfg = get_config(args.model)
    sd = synth.synthetic_state_dict(cfg, seed=args.seed, device="cuda")
    model = MoondreamModel(cfg, sd, device="cuda", tokenizer=IdTokenizer(), max_batch=B)
    model.compile()
    gpath = os.path.join(REPO, "tests", "golden", "md2b_detect13.npz")
    g = np.load(gpath) if os.path.exists(gpath) and args.model == "2b" and args.seed == 1 else None
    size = tuple(int(x) for x in g["size"]) if g is not None else (768, 1024)
    max_objects = int(g["max_objects"]) if g is not None else 4
    obj = " ".join(str(t) for t in (g["object_ids"].tolist() if g is not None else [7, 8]))
    imgs = [synth.synthetic_image(i, args.seed, size) for i in range(B)]
    st = {"max_objects": max_objects, "_run_all_objects": True, **LEGS[args.leg]}
    run = lambda: model.batch_detect(imgs, [obj] * B, st)
    res = run()  # warm-up
    boxes = [[[o[k] for k in ("x_min", "y_min", "x_max", "y_max")] for o in r["objects"]] for r in res]
    times = []
    for _ in range(args.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    out = {"leg": args.leg, "images_per_s": round(B / statistics.median(times), 2), "run_s_all": [round(t, 4) for t in times],
           "max_objects": max_objects, "objects": sum(len(b) for b in boxes), "boxes_crc": zlib.crc32(repr(boxes).encode())}
    if "return_scores" in st:
        scores = [o["score"] for r in res for o in r["objects"]]
        out["score_min_max"] = [min(scores), max(scores)] if scores else None
    print(json.dumps(out))


def child(argv, repo=None, timeout=900):
    """A fresh process of this file (``repo``: the tree its moondream_amd comes from); its last stdout line as JSON."""
    env = dict(os.environ, MD_BENCH_DETECT_SCORES_REPO=repo or REPO)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), *argv], env=env, stdout=subprocess.PIPE, timeout=timeout)
    if r.returncode != 0:
        raise SystemExit(f"worker {argv} failed with status {r.returncode}")
    line = r.stdout.decode().strip().splitlines()[-1]
    print(f"[bench_detect_scores] {' '.join(argv[:4])}: {line}", file=sys.stderr, flush=True)
    return json.loads(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="2b")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parent-repo", default=None, help="a built checkout of the parent commit (the setting-absent leg)")
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--leg", choices=tuple(LEGS), default="off")
    args = ap.parse_args()
    sys.path.insert(0, os.environ.get("MD_BENCH_DETECT_SCORES_REPO", REPO))
    if args.worker:
        import torch

        with torch.inference_mode():
            worker(args)
        return

    common = ["--model", args.model, "--seed", str(args.seed), "--repeats", str(args.repeats)]
    legs = ["off", "w0", "w8"] + (["parent"] if args.parent_repo else [])
    runs = {leg: [] for leg in legs}
    for _ in range(args.procs):  # alternate the legs: drift of the machine lands on all of them
        for leg in legs:
            runs[leg].append(child(["--worker", "--leg", leg, *common], args.parent_repo if leg == "parent" else None))
    assert len({r["boxes_crc"] for rs in runs.values() for r in rs}) == 1, "the legs' boxes differ"
    result = {"metric": "detect_scores_bench", "model": args.model, "batch": B, "crops_per_image": 13, "procs": args.procs,
              "repeats": args.repeats, "max_objects": runs["off"][0]["max_objects"], "objects_per_call": runs["off"][0]["objects"]}
    for leg in legs:
        v = [r["images_per_s"] for r in runs[leg]]
        result[leg] = {"images_per_s_median": statistics.median(v), "images_per_s_span": [min(v), max(v)], "images_per_s_all": v}
    for leg in ("w0", "w8"):
        result[leg]["images_per_s_vs_off"] = round(result[leg]["images_per_s_median"] / result["off"]["images_per_s_median"], 4)
        result[leg]["score_min_max"] = runs[leg][0]["score_min_max"]
    if args.parent_repo:
        lo, hi = result["parent"]["images_per_s_span"]
        result["off_within_parent_span"] = lo <= result["off"]["images_per_s_median"] <= hi
        result["off_vs_parent"] = round(result["off"]["images_per_s_median"] / result["parent"]["images_per_s_median"], 4)
    line = json.dumps(result)
    with open(os.path.join(REPO, "profiles", "detect_scores_bench.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
