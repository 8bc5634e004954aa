"""What device-side image preprocessing costs and saves (``model.device_preprocess``; 2B, bf16, compile()).  Prints one JSON
line, also written to profiles/device_preprocess_bench.json.

  latency   ``encode_image`` of one seeded image at 378 x 378, 1024 x 768 and 4000 x 3000 (W x H), host path against device
            path: ``--procs`` fresh processes per leg that alternate (host, device, host, ..); per process and size the median
            of ``--repeats`` timed calls after a warm-up, per leg the median and the span of the process medians.
  batch     ``batch_detect`` at B = 32 over 768 x 1024 images (13 crops each: bench.py's detect13 workload) and
            ``batch_generate_ids`` at B = 64 over 378 x 378 images (2 crops each): switch off, switch on and, with
            ``--parent-repo DIR`` (a built checkout of the parent commit), that tree's call.  ``off_within_parent_span`` says
            whether the switch-off median lies inside the parent's own span: nothing on that path changed.
            ``--skip-batch`` leaves this part out.
  kernel    the two launches of md_image_resample_crops alone over 32 images of 1000 x 1400 (H x W; 10 crops each), from device
            events around ``--launches`` back-to-back calls, the median of ``--repeats`` such windows; next to it the
            host-to-device copy of the same packed bytes from pinned memory, timed the same way.

  python tools/bench_device_preprocess.py [--parent-repo DIR] [--skip-batch] [--skip-latency]
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
LATENCY_SIZES = ((378, 378), (768, 1024), (3000, 4000))  # (H, W)
BATCH = {"detect13_b32": (32, (768, 1024)), "caption2_b64": (64, (378, 378))}
KERNEL_IMAGES, KERNEL_SIZE = 32, (1000, 1400)


def make_model(args, max_batch):
    from moondream_amd import synth
    from moondream_amd.config import get_config
    from moondream_amd.moondream import IdTokenizer, MoondreamModel

    cfg = get_config(args.model)
    model = MoondreamModel(cfg, synth.synthetic_state_dict(cfg, seed=args.seed, device="cuda"), device="cuda", tokenizer=IdTokenizer(),
                           max_batch=max_batch)
    model.compile()
    if args.leg == "device":
        model.device_preprocess = True  # (the parent leg runs a tree without the attribute: never set there)
    return cfg, model


def timed(fn, repeats):
    import torch

    fn()  # warm-up: graph captures, coefficient tables, pinned buffers
    times = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return times


def worker_latency(args):
    from moondream_amd import synth

    cfg, model = make_model(args, 1)
    out = {"leg": args.leg}
    for h, w in LATENCY_SIZES:
        img = synth.synthetic_image(3, args.seed, (h, w))
        ms = [t * 1e3 for t in timed(lambda: model.encode_image(img), args.repeats)]
        out[f"{w}x{h}"] = {"ms_median": round(statistics.median(ms), 3), "ms_all": [round(x, 3) for x in ms]}
    print(json.dumps(out))


def worker_batch(args):
    from moondream_amd import synth

    out = {"leg": args.leg}
    cfg, model = make_model(args, 64)
    for name, (b, size) in BATCH.items():
        images = [synth.synthetic_image(i, args.seed, size) for i in range(b)]
        if name.startswith("detect"):
            run = lambda: model.batch_detect(images, ["7 8"] * b, {"max_objects": 4})
        else:
            prompts = [cfg.tokenizer.templates["caption"]["normal"]] * b
            run = lambda: model.batch_generate_ids(images, prompts, max_tokens=32, ignore_eos=True)
        res = run()
        t = timed(run, args.repeats)
        out[name] = {"images_per_s": round(b / statistics.median(t), 2), "run_s_all": [round(x, 4) for x in t],
                     "result_crc": zlib.crc32(json.dumps(res, sort_keys=True).encode())}
    print(json.dumps(out))


def worker_kernel(args):
    import numpy as np
    import torch

    from moondream_amd import _lib, resample
    from moondream_amd.config import get_config
    from moondream_amd.crop_staging import PinnedRing

    lib, v = _lib.load(), get_config(args.model).vision
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    records = resample.plan([KERNEL_SIZE] * KERNEL_IMAGES, v)
    lay = resample.layout(records, v)
    rng = np.random.default_rng(args.seed)
    lease = PinnedRing().take(lay.nbytes)
    host = lease.array((lay.nbytes,))
    lay.write(host, [rng.integers(0, 256, size=KERNEL_SIZE + (3,), dtype=np.uint8) for _ in range(KERNEL_IMAGES)])
    pinned = torch.from_numpy(host)
    packed = torch.empty(lay.nbytes, dtype=torch.uint8, device="cuda")
    packed.copy_(pinned, non_blocking=True)
    crop, window, margin_px = resample.geometry(v)
    crops = torch.empty(lay.out_crops, crop, crop, 3, dtype=torch.uint8, device="cuda")
    ws = torch.empty(lay.ws_bytes, dtype=torch.uint8, device="cuda")

    def launch():
        _lib.check(lib.md_image_resample_crops(packed.data_ptr(), packed.numel(), lay.desc.ctypes.data, KERNEL_IMAGES, crop, window,
                                               margin_px, crops.data_ptr(), lay.out_crops, ws.data_ptr(), ws.numel(), stream), "resample")

    def window_us(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / n

    cases = {"resample_two_launches": launch, "h2d_copy_pinned": lambda: packed.copy_(pinned, non_blocking=True)}
    for fn in cases.values():
        window_us(fn, 5)
    per = {name: [] for name in cases}
    for _ in range(args.repeats):  # the cases alternate window by window
        for name, fn in cases.items():
            per[name].append(window_us(fn, args.launches))
    out = {name: {"us_median": round(statistics.median(us), 1), "us_all": [round(x, 1) for x in us]} for name, us in per.items()}
    # bytes the algorithm needs: the source once, the intermediates written and read once, the crops written once
    moved = lay.nbytes + 2 * lay.ws_bytes + crops.numel()
    out["resample_two_launches"]["gb_per_s_needed_bytes"] = round(moved / out["resample_two_launches"]["us_median"] / 1e3, 1)
    out["h2d_copy_pinned"]["gb_per_s"] = round(lay.nbytes / out["h2d_copy_pinned"]["us_median"] / 1e3, 1)
    out.update(images=KERNEL_IMAGES, size_hw=list(KERNEL_SIZE), packed_bytes=lay.nbytes, workspace_bytes=lay.ws_bytes,
               crops=lay.out_crops, launches_per_window=args.launches,
               bound_by="h2d_copy" if out["h2d_copy_pinned"]["us_median"] > out["resample_two_launches"]["us_median"] else "kernels")
    print(json.dumps(out))


def child(argv, repo=None, timeout=1500):
    """A fresh process of this file (``repo``: the tree its moondream_amd comes from); its last stdout line as JSON."""
    env = dict(os.environ, MD_BENCH_PREPROCESS_REPO=repo or REPO)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), *argv], env=env, stdout=subprocess.PIPE, timeout=timeout)
    if r.returncode != 0:
        raise SystemExit(f"worker {argv} failed with status {r.returncode}")
    line = r.stdout.decode().strip().splitlines()[-1]
    print(f"[bench_device_preprocess] {' '.join(argv[:4])}: {line}", file=sys.stderr, flush=True)
    return json.loads(line)


def spans(values):
    return {"median": statistics.median(values), "span": [min(values), max(values)], "all": values}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="2b")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--parent-repo", default=None, help="a built checkout of the parent commit (its switch-off leg)")
    ap.add_argument("--skip-latency", action="store_true")
    ap.add_argument("--skip-batch", action="store_true")
    ap.add_argument("--worker", choices=("latency", "batch", "kernel"))
    ap.add_argument("--leg", choices=("host", "device", "parent"), default="host")
    args = ap.parse_args()
    sys.path.insert(0, os.environ.get("MD_BENCH_PREPROCESS_REPO", REPO))
    if args.worker:
        import torch

        with torch.inference_mode():
            {"latency": worker_latency, "batch": worker_batch, "kernel": worker_kernel}[args.worker](args)
        return

    common = ["--model", args.model, "--seed", str(args.seed), "--repeats", str(args.repeats)]
    result = {"metric": "device_preprocess_bench", "model": args.model, "procs": args.procs, "repeats": args.repeats}
    if not args.skip_latency:
        runs = {"host": [], "device": []}
        for _ in range(args.procs):  # alternate the legs: drift of the machine lands on both
            for leg in runs:
                runs[leg].append(child(["--worker", "latency", "--leg", leg, *common]))
        result["latency_ms"] = {f"{w}x{h}": {leg: spans([r[f"{w}x{h}"]["ms_median"] for r in runs[leg]]) for leg in runs}
                                for h, w in LATENCY_SIZES}
    if not args.skip_batch:
        legs = ["host", "device"] + (["parent"] if args.parent_repo else [])
        runs = {leg: [] for leg in legs}
        for _ in range(args.procs):
            for leg in legs:
                runs[leg].append(child(["--worker", "batch", "--leg", leg, *common], args.parent_repo if leg == "parent" else None))
        batch = {}
        for name in BATCH:
            batch[name] = {leg: spans([r[name]["images_per_s"] for r in runs[leg]]) for leg in legs}
            assert len({r[name]["result_crc"] for leg in legs for r in runs[leg]}) == 1, f"{name}: results differ between the legs"
            if args.parent_repo:
                lo, hi = batch[name]["parent"]["span"]
                batch[name]["off_within_parent_span"] = lo <= batch[name]["host"]["median"] <= hi
        result["batch_images_per_s"] = batch
    result["kernel"] = child(["--worker", "kernel", "--model", args.model, "--seed", str(args.seed), "--repeats", str(args.repeats),
                              "--launches", str(args.launches)])
    line = json.dumps(result)
    with open(os.path.join(REPO, "profiles", "device_preprocess_bench.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
