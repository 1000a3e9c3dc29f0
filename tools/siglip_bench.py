"""Forward + backward of SigLipLoss vs ClipLoss on the same embeddings.
    python tools/siglip_bench.py [--shapes 4096x4096x768,4096x32768x768] [--iters 20] [--warmup 5] > siglip.jsonl
One JSON line per shape B x N x E (B local rows, N gathered columns): milliseconds (HIP events, median after warm-up) of one
forward + backward for each loss, their ratio, and the per-kernel times of one further step (`ops.profile_start`).  N == B
runs the loss modules themselves at one rank (casts, autograd nodes, gradient GEMMs and all).  N > B is the per-rank work of an N / B-rank run on one GPU: the kernel sequence rank 0's
autograd node issues against N gathered columns (local_loss + gather_with_grad for ClipLoss), without the collectives -
ClipLoss exchanges both embeddings and both gradients there, SigLipLoss the text side only, so the omission favours ClipLoss.
ClipLoss is the yardstick: it is the loss the engine trains with today."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import clipa_amd  # noqa: E402
from clipa_amd import ops  # noqa: E402

DEV = "cuda"
SHAPES = [(4096, 4096, 768), (4096, 32768, 768)]
f32 = torch.float32


def measure(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def module_step(loss_fn, img, txt, scalars):
    def step():
        for t in (img, txt) + scalars:
            t.grad = None
        loss_fn(img, txt, *scalars).backward()
    return step


def siglip_rank_step(i_rows, t_all, s, b):
    """SigLipLossFn's kernels for B local images against N gathered texts."""
    B, N = i_rows.shape[0], t_all.shape[0]

    def step():
        lr, dl, dsr, dbr = ops.simsig(i_rows, t_all, N, 0, 1.0 / B, s, b)
        ops.sum_scale(lr, 1.0 / B)
        ops.gemm_nt(dl, ops.transpose_bf16(t_all), out_f32=True)
        ops.gemm_tn(dl, i_rows, f32)
        ops.sum_scale(dsr, 1.0)
        ops.sum_scale(dbr, 1.0)
    return step


def clip_rank_step(i_rows, t_rows, i_all, t_all, s):
    """ClipLossFn's kernels (local_loss, gather_with_grad) for B local pairs against N gathered embeddings."""
    B, N = i_rows.shape[0], t_all.shape[0]

    def step():
        li, dli, dsi = ops.simce(i_rows, t_all, N, 0, 0.5 / B, scale=s)
        lt, dlt, dst = ops.simce(t_rows, i_all, N, 0, 0.5 / B, scale=s)
        loss = ops.sum_scale(li, 0.5 / B)
        ops.sum_scale(lt, 0.5 / B, out=loss, accumulate=True)
        ops.gemm_nt(dli, ops.transpose_bf16(t_all), out_f32=True)
        ops.gemm_nt(dlt, ops.transpose_bf16(i_all), out_f32=True)
        d_t_all = ops.gemm_tn(dli, i_rows, f32)
        d_i_all = ops.gemm_tn(dlt, t_rows, f32)
        torch.cat([d_i_all, d_t_all], dim=1)              # the reduce-scatter's operand
        d_s = ops.sum_scale(dsi, 1.0)
        ops.sum_scale(dst, 1.0, out=d_s, accumulate=True)
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=None, help="comma-separated BxNxE list (default: 4096x4096x768,4096x32768x768)")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    shapes = SHAPES if not args.shapes else [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]
    for B, N, E in shapes:
        g = torch.Generator(device=DEV).manual_seed(B + N + E)
        base = torch.randn(N, E, device=DEV, generator=g)
        img = torch.nn.functional.normalize(base + 2.0 * torch.randn(N, E, device=DEV, generator=g), dim=-1)
        txt = torch.nn.functional.normalize(base + 2.0 * torch.randn(N, E, device=DEV, generator=g), dim=-1)
        del base
        if N == B:
            mode = "modules, one rank"
            img.requires_grad_(True)
            txt.requires_grad_(True)
            s10, b10 = (torch.tensor(v, device=DEV, requires_grad=True) for v in (10.0, -10.0))
            s14 = torch.tensor(1.0 / 0.07, device=DEV, requires_grad=True)
            sig = module_step(clipa_amd.SigLipLoss(), img, txt, (s10, b10))
            clip = module_step(clipa_amd.ClipLoss(), img, txt, (s14,))
        else:
            mode = f"kernel sequence of one of {N // B} ranks, no collectives"
            ib, tb = ops.to_bf16(img), ops.to_bf16(txt)
            s10, b10, s14 = (torch.tensor([v], device=DEV) for v in (10.0, -10.0, 1.0 / 0.07))
            sig = siglip_rank_step(ib[:B], tb, s10, b10)
            clip = clip_rank_step(ib[:B], tb[:B], ib, tb, s14)
        sig_ms, sig_lo, sig_hi = measure(sig, args.iters, args.warmup)
        clip_ms, clip_lo, clip_hi = measure(clip, args.iters, args.warmup)
        per_kernel = {}
        for name, step in (("siglip", sig), ("cliploss", clip)):      # one more step each with the per-launch event timers on
            ops.profile_start()
            step()
            per_kernel[name] = {k: round(v["ms"], 3) for k, v in ops.profile_stop().items()}
        print(json.dumps({"B": B, "N": N, "E": E, "mode": mode, "iters": args.iters, "warmup": args.warmup,
                          "siglip_ms": round(sig_ms, 3), "siglip_min_max_ms": [round(sig_lo, 3), round(sig_hi, 3)],
                          "cliploss_ms": round(clip_ms, 3), "cliploss_min_max_ms": [round(clip_lo, 3), round(clip_hi, 3)],
                          "siglip_over_cliploss": round(sig_ms / clip_ms, 3), "kernel_ms": per_kernel}), flush=True)
        del img, txt
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
