"""Retrieval ranks of get_clip_metrics: the fused fp32 kernel (ops.retrieval_ranks) vs a chunked torch-on-GPU yardstick.
    python tools/retrieval_bench.py [--shapes 5000x768,50000x1024] [--iters 3] [--no-torch] > retrieval.jsonl
One JSON line per shape: milliseconds (HIP events, median after warm-up), TF/s at 2 N^2 E FLOPs and its fraction of the
157.3 TF fp32 matrix peak, and the rise of torch's peak allocated memory during one call, for the kernel and for the
yardstick (fp32 matmul of 4096-row blocks, then compare with the positives and count).  The yardstick's counts are
checked against the kernel's where both exist (they may differ only at near ties)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clipa_amd import ops  # noqa: E402

DEV = "cuda"
PEAK_TF = 157.3
SHAPES = [(n, e) for n in (5000, 50000, 65536) for e in (768, 1024)]


def torch_ranks(img, txt, scale, block=4096):
    """Chunked yardstick: the same counts with fp32 torch.matmul on row blocks, O(block * N) memory."""
    N = img.shape[0]
    d = scale * (img * txt).sum(1)                       # positives (different rounding than a GEMM; fine for timing)
    i2t = torch.empty(N, device=DEV, dtype=torch.int32)
    t2i = torch.zeros(N, device=DEV, dtype=torch.int64)
    for r0 in range(0, N, block):
        v = scale * (img[r0:r0 + block] @ txt.t())        # [b, N]
        idx = torch.arange(r0, min(r0 + block, N), device=DEV)
        v[idx - r0, idx] = float("-inf")
        i2t[r0:r0 + block] = (v > d[r0:r0 + block, None]).sum(1).to(torch.int32)
        t2i += (v > d[None, :]).sum(0)
        del v
    return i2t, t2i.to(torch.int32)


def measure(fn, iters):
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.max_memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2], rise, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=None, help="comma-separated NxE list (default: the 6 standard shapes)")
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true", help="skip the torch yardstick")
    args = ap.parse_args()
    shapes = SHAPES if not args.shapes else [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]
    for N, E in shapes:
        g = torch.Generator(device=DEV).manual_seed(N + E)
        base = torch.randn(N, E, device=DEV, generator=g)
        img = torch.nn.functional.normalize(base + 2.0 * torch.randn(N, E, device=DEV, generator=g), dim=-1)
        txt = torch.nn.functional.normalize(base + 2.0 * torch.randn(N, E, device=DEV, generator=g), dim=-1)
        del base
        scale = torch.tensor([1.0 / 0.07], device=DEV)
        flops = 2.0 * N * N * E
        ms, rise, (i2t, _, t2i, _) = measure(lambda: ops.retrieval_ranks(img, txt, scale), args.iters)
        rec = {"N": N, "E": E, "kernel_ms": round(ms, 3), "kernel_tflops": round(flops / ms / 1e9, 1),
               "kernel_frac_of_peak": round(flops / ms / 1e9 / PEAK_TF, 3), "kernel_mem_rise_mb": round(rise / 2 ** 20, 2)}
        if not args.no_torch:
            tms, trise, (ti2t, tt2i) = measure(lambda: torch_ranks(img, txt, scale), max(1, args.iters // 2))
            rec.update({"torch_ms": round(tms, 3), "torch_tflops": round(flops / tms / 1e9, 1),
                        "torch_mem_rise_mb": round(trise / 2 ** 20, 2), "speedup_vs_torch": round(tms / ms, 2),
                        "i2t_disagree": int((ti2t != i2t).sum()), "t2i_disagree": int((tt2i != t2i).sum())})
        print(json.dumps(rec), flush=True)
        del img, txt
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
