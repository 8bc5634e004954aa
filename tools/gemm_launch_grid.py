#!/usr/bin/env python
"""One call of md_gemm_bf16 / md_gemm_partial_f32 / md_gemm_partial_f32_pair per point of a grid of launch inputs, for
comparing two builds of the library launch by launch (MD_HIP_LIB selects the build):

    rocprofv3 --kernel-trace --output-format csv -d <dir> -- python tools/gemm_launch_grid.py <calls.jsonl>
    python tools/gemm_launch_grid.py --compare <calls_a.jsonl> <trace_a.csv> <calls_b.jsonl> <trace_b.csv>

Every call is followed by exactly one marker kernel (a torch fill), so the kernel trace splits into per-call lists of
(kernel, grid, workgroup, LDS bytes); the result goes to the host by a copy (no kernel) and its CRC32 into <calls.jsonl>."""
import csv
import ctypes as C
import json
import math
import sys
import zlib

LAYERS = [(2048, 14336), (2048, 2048), (8192, 2048), (2048, 51200), (704, 256), (1152, 1000), (256, 1024), (4352, 1152)]
MS = [1, 33, 64, 70, 128, 300]
DECODE_CFGS = [16, 17, 18, 19, 10, 3]
TILE_IDS = [1, 2, 3, 10, 11, 15, 16, 17, 18, 19, 20, 21]


def run(out_path):
    import torch

    from moondream_amd import _lib
    from moondream_amd.weights import PackedLinear

    lib = _lib.load()
    BF16 = torch.bfloat16
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    mark = torch.zeros(1, dtype=torch.float64, device="cuda")  # the only float64 tensor: its fill kernel is the marker

    def randn(*shape, scale=1.0, seed=0):
        g = torch.Generator(device="cpu").manual_seed(seed)
        return (torch.randn(*shape, generator=g) * scale).to(BF16).cuda()

    def finish(f, rec, status, out):
        torch.cuda.synchronize()
        rec["status"] = status
        rec["crc"] = zlib.crc32(out.cpu().contiguous().view(torch.uint8).numpy().tobytes()) if status == 0 else None
        mark.fill_(1.0)  # the one marker kernel of this call
        torch.cuda.synchronize()
        f.write(json.dumps(rec) + "\n")

    with open(out_path, "w") as f:
        for li, (k, n) in enumerate(LAYERS):
            w, b = randn(n, k, scale=1 / math.sqrt(k), seed=2), randn(n, scale=0.1, seed=3)
            lin = PackedLinear(w, b, "cuda")
            st = lin.struct()
            ms = [m for m in MS if m <= 128 or n < 51200]
            a_all = torch.zeros(max(ms), lin.k_pad, dtype=BF16, device="cuda")
            a_all[:, :k] = randn(max(ms), k, seed=1)
            r_all = randn(max(ms), n, seed=4)
            for knob, values in ((b"decode_cfg", DECODE_CFGS), (b"tile", TILE_IDS)):
                for v in values:
                    _lib.check(lib.md_gemm_set_tuning(knob, v))
                    # sized under the knob that is set NOW: the size depends on decode_cfg (the widest layer splits K only under 3)
                    ws_all = torch.zeros(max(16, max(lib.md_gemm_workspace_bytes(C.byref(st), m, 0) for m in ms)), dtype=torch.uint8, device="cuda")
                    for m in ms:
                        a, r = a_all[:m], r_all[:m]
                        for policy in (0, 1, 2, 3):
                            for epi in (0, 1, 2):
                                for use_ws in (1, 0):
                                    c = torch.zeros(m, n, dtype=BF16, device="cuda")
                                    need = lib.md_gemm_workspace_bytes(C.byref(st), m, 0)
                                    assert need <= ws_all.numel(), (need, ws_all.numel())  # never promise more than is allocated
                                    args = _lib.MdGemmArgs(a.data_ptr(), a.stride(0), st, c.data_ptr(), c.stride(0),
                                                           r.data_ptr() if epi == 2 else None, r.stride(0) if epi == 2 else 0, 0, m, epi, 0, 0,
                                                           ws_all.data_ptr() if use_ws else None, need if use_ws else 0, policy)
                                    status = lib.md_gemm_bf16(C.byref(args), stream())
                                    finish(f, dict(call="gemm", layer=li, knob=knob.decode(), value=v, m=m, policy=policy, epi=epi, ws=use_ws), status, c)
                        if knob == b"decode_cfg" and m <= 128:
                            s = lib.md_gemm_partial_slices(C.byref(st))
                            p0 = torch.zeros(s, m, n, dtype=torch.float32, device="cuda")
                            status = lib.md_gemm_partial_f32(a.data_ptr(), a.stride(0), C.byref(st), m, p0.data_ptr(), n, m * n, stream())
                            finish(f, dict(call="partial", layer=li, value=v, m=m), status, p0)
                            p0.zero_()
                            p1 = torch.zeros_like(p0)
                            status = lib.md_gemm_partial_f32_pair(a.data_ptr(), a.stride(0), C.byref(st), p0.data_ptr(), a.data_ptr(), a.stride(0),
                                                                  C.byref(st), p1.data_ptr(), m, n, m * n, stream())
                            finish(f, dict(call="pair", layer=li, value=v, m=m), status, torch.stack([p0, p1]))
                    _lib.check(lib.md_gemm_set_tuning(knob, 16 if knob == b"decode_cfg" else -1))


def per_call(trace_csv):
    rows = list(csv.DictReader(open(trace_csv)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    shape_cols = [c for c in rows[0] if c.lower().startswith(("grid_size", "workgroup_size", "lds_block_size"))]
    assert len(shape_cols) >= 3, list(rows[0])
    calls, cur = [], []
    for r in rows:
        name = r["Kernel_Name"]
        if "gemm_bf16_kernel" in name or "gemm_pair_kernel" in name or "gemm_w4_kernel" in name:
            cur.append((name,) + tuple(r[c] for c in shape_cols))
        elif "FillFunctor<double>" in name:  # the marker
            calls.append(cur)
            cur = []
    return calls


def compare(calls_a, trace_a, calls_b, trace_b):
    ra, rb = [json.loads(l) for l in open(calls_a)], [json.loads(l) for l in open(calls_b)]
    ka, kb = per_call(trace_a), per_call(trace_b)
    # (torch.zeros of the marker tensor itself may run the same fill kernel once, before the first call)
    ka, kb = ka[len(ka) - len(ra):], kb[len(kb) - len(rb):]
    assert len(ra) == len(rb) == len(ka) == len(kb), (len(ra), len(rb), len(ka), len(kb))
    bad_launch = bad_crc = bad_status = 0
    for x, y, la, lb in zip(ra, rb, ka, kb):
        assert {k: v for k, v in x.items() if k not in ("status", "crc")} == {k: v for k, v in y.items() if k not in ("status", "crc")}
        if la != lb:
            bad_launch += 1
            print("LAUNCHES DIFFER", x, la, lb)
        if x["crc"] != y["crc"]:
            bad_crc += 1
            print("CHECKSUMS DIFFER", x, y)
        if x["status"] != y["status"]:
            bad_status += 1
            print("STATUS DIFFERS", x, y)
    kernels = sorted({k[0].split("(")[0][:120] for c in ka for k in c})
    by_status = {}
    for x in ra:
        by_status[x["status"]] = by_status.get(x["status"], 0) + 1
    print(f"{len(ra)} calls ({sum(1 for x in ra if x['call'] == 'gemm')} md_gemm_bf16, {sum(1 for x in ra if x['call'] == 'partial')} md_gemm_partial_f32, "
          f"{sum(1 for x in ra if x['call'] == 'pair')} md_gemm_partial_f32_pair), statuses {by_status}, {sum(len(c) for c in ka)} GEMM kernel launches, "
          f"{len(kernels)} distinct kernels")
    print(f"calls whose (kernel, grid, workgroup, LDS) list differs: {bad_launch}; whose status differs: {bad_status}; whose checksum differs: {bad_crc}")
    print("RESULT:", "identical" if bad_launch == bad_crc == bad_status == 0 else "DIFFERENT")
    return 0 if bad_launch == bad_crc == bad_status == 0 else 1


if __name__ == "__main__":
    import os
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if sys.argv[1] == "--compare":
        sys.exit(compare(*sys.argv[2:6]))
    run(sys.argv[1])
