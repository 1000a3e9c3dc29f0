"""Multi-caption retrieval ranks (ops.retrieval_ranks_multi, csrc/retrieval_multi.hip) vs a chunked torch-on-GPU yardstick.
    python tools/retrieval_multi_bench.py [--shapes 1000x5000x768,5000x25000x1024] [--iters 3] [--no-torch] > out.jsonl
One JSON line per Ni x Nt x E shape (5 captions per image, in image order as COCO and Flickr30k store them):
milliseconds (HIP events, median after warm-up) and TF/s at 2 Ni Nt E FLOPs, its fraction of the 157.3 TF fp32 matrix
peak, and the rise of torch's peak allocated memory during one call, for the kernel and for the yardstick (fp32 matmul
of image-row blocks of at most 1 GiB of scores, own entries masked, then compare with the positives and count).  The
yardstick's gt counts are checked against the kernel's (they may differ only at near ties: its positives are rounded
differently)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clipa_amd import ops  # noqa: E402

DEV = "cuda"
PEAK_TF = 157.3
SHAPES = [(1000, 5000, 768), (5000, 25000, 768), (5000, 25000, 1024), (100000, 500000, 768)]


def torch_ranks(img, txt, c):
    """Chunked yardstick: i2t_gt and t2i_gt with fp32 torch.matmul on image-row blocks, O(block * Nt) memory."""
    Ni, Nt = img.shape[0], txt.shape[0]
    p = (img[c] * txt).sum(1)                                              # text positives
    m = torch.full((Ni,), float("-inf"), device=DEV).scatter_reduce(0, c, p, "amax")
    block = max(1, min(Ni, (1 << 28) // Nt))
    i2t = torch.empty(Ni, device=DEV, dtype=torch.int32)
    t2i = torch.zeros(Nt, device=DEV, dtype=torch.int64)
    for r0 in range(0, Ni, block):
        v = img[r0:r0 + block] @ txt.t()                                    # [b, Nt]
        v[c[None, :] == torch.arange(r0, r0 + v.shape[0], device=DEV)[:, None]] = float("-inf")   # own entries never count
        i2t[r0:r0 + block] = (v > m[r0:r0 + block, None]).sum(1).to(torch.int32)
        t2i += (v > p[None, :]).sum(0)
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
    ap.add_argument("--shapes", default=None, help="comma-separated NixNtxE list (default: the 4 standard shapes)")
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true", help="skip the torch yardstick")
    args = ap.parse_args()
    shapes = SHAPES if not args.shapes else [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]
    for Ni, Nt, E in shapes:
        g = torch.Generator(device=DEV).manual_seed(Ni + Nt + E)
        c = torch.arange(Ni, device=DEV).repeat_interleave((Nt + Ni - 1) // Ni)[:Nt]
        base = torch.randn(Ni, E, device=DEV, generator=g)
        img = torch.nn.functional.normalize(base + 4.0 * torch.randn(Ni, E, device=DEV, generator=g), dim=-1)
        txt = torch.nn.functional.normalize(base[c] + 4.0 * torch.randn(Nt, E, device=DEV, generator=g), dim=-1)
        del base
        flops = 2.0 * Ni * Nt * E
        ms, rise, (i2t, _, t2i, _) = measure(lambda: ops.retrieval_ranks_multi(img, txt, c), args.iters)
        rec = {"Ni": Ni, "Nt": Nt, "E": E, "kernel_ms": round(ms, 3), "kernel_tflops": round(flops / ms / 1e9, 1),
               "kernel_frac_of_peak": round(flops / ms / 1e9 / PEAK_TF, 3), "kernel_mem_rise_mb": round(rise / 2 ** 20, 2),
               "img2txt_r1": round(float((i2t == 0).float().mean()), 4), "txt2img_r1": round(float((t2i == 0).float().mean()), 4)}
        if not args.no_torch:
            tms, trise, (ti2t, tt2i) = measure(lambda: torch_ranks(img, txt, c), max(1, args.iters // 2))
            rec.update({"torch_ms": round(tms, 3), "torch_tflops": round(flops / tms / 1e9, 1),
                        "torch_mem_rise_mb": round(trise / 2 ** 20, 2), "speedup_vs_torch": round(tms / ms, 2),
                        "i2t_disagree": int((ti2t != i2t).sum()), "t2i_disagree": int((tt2i != t2i).sum())})
        print(json.dumps(rec), flush=True)
        del img, txt
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
