"""What the fine-tuning launches cost next to the tower, from one run.
    python tools/finetune_bench.py [--batch 1024] [--classes 1000] [--iters 20] [--models ViT-B-16 ViT-L-16] [--out profiles/finetune_bench.md]
uint8 channels_last images at 224 px (what DeviceAugment returns).  HIP events, median of --iters calls after 3 warm-up calls:
  mixcut mixup / cutmix      ops.mixcut_u8 in place; bytes = 2 reads + 2 writes per byte pair of the batch for mixup, and for
                             cutmix (boxes of sqrt(0.5) S, the mean of Beta(1, 1)) only the 16-byte chunks a box touches are
                             moved: its GB/s is given against the same 4 bytes per pair, as if every chunk moved
  head fwd / fwd+bwd         finetune.HeadLinearFn on fp32 features [B, E]: the bf16 cast, the GEMM, and in backward the cast of
                             dlogits, the feature-gradient GEMM and the weight-gradient GEMM (operand cache warm)
  loss fwd+bwd               SoftTargetCrossEntropy with mixed targets and smoothing 0.1: softce (loss + dlogits), the mean, and
                             in backward the cast / scale of dlogits
  tower fwd+bwd              model.visual forward + backward with a random feature gradient, grad checkpointing on
No time is gated.  Every number is a measurement of the run that printed it, on the device named in the record."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import clipa_amd  # noqa: E402
from clipa_amd import finetune, ops  # noqa: E402

DEV = "cuda"


def timed(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2]


def model_record(name, img, C, iters):
    torch.manual_seed(0)
    clip = clipa_amd.create_model(name, device=DEV)
    clip.set_grad_checkpointing(True)
    m = clipa_amd.ImageClassifier(clip.visual, C).train()
    B, E = img.shape[0], clip.visual.output_dim
    g = torch.Generator(device=DEV).manual_seed(1)
    feat = torch.randn(B, E, device=DEV, generator=g).requires_grad_(True)
    dfeat = torch.randn(B, E, device=DEV, generator=g) * 1e-3
    dlog = torch.randn(B, C, device=DEV, generator=g) * 1e-3
    ya = torch.randint(0, C, (B,), device=DEV, generator=g, dtype=torch.int32)
    lam = torch.rand(B, device=DEV, generator=g)
    target = (ya, ya.flip(0), lam)
    crit = clipa_amd.SoftTargetCrossEntropy(0.1)
    logits = m.head_logits(feat).detach().requires_grad_(True)
    params = [p for p in clip.visual.parameters() if p.requires_grad]

    def head_fb():
        torch.autograd.grad(m.head_logits(feat), (feat, m.head.weight), dlog)

    def loss_fb():
        torch.autograd.grad(crit(logits, target), logits)

    def tower_fb():
        torch.autograd.grad(m.visual(img), params, dfeat, allow_unused=True)

    with torch.no_grad():
        t_head_f = timed(lambda: m.head_logits(feat), iters)
    rec = {"model": name, "embed_dim": E, "head_fwd_ms": round(t_head_f, 4), "head_fwd_bwd_ms": round(timed(head_fb, iters), 4),
           "loss_fwd_bwd_ms": round(timed(loss_fb, iters), 4), "tower_fwd_bwd_ms": round(timed(tower_fb, max(3, iters // 4)), 3)}
    ops.check_token_ids(wait=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--classes", type=int, default=1000)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--models", nargs="+", default=["ViT-B-16", "ViT-L-16"])
    ap.add_argument("--out", default=None, help="also write the record as a markdown file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("finetune_bench: no GPU visible; nothing is measured without one")
    B, S, C = args.batch, 224, args.classes
    g = torch.Generator(device=DEV).manual_seed(B)
    img = torch.randint(0, 256, (B, 3, S, S), device=DEV, dtype=torch.uint8, generator=g).contiguous(memory_format=torch.channels_last)
    lam = torch.rand(B, device=DEV, generator=g) * 0.98 + 0.01
    side = int(0.5 ** 0.5 * S)
    y0 = torch.randint(0, S - side, (B,), device=DEV, generator=g, dtype=torch.int32)
    x0 = torch.randint(0, S - side, (B,), device=DEV, generator=g, dtype=torch.int32)
    box = torch.stack([y0, y0 + side, x0, x0 + side], 1).contiguous()
    work = img.clone(memory_format=torch.preserve_format)
    nbytes = 4.0 * (B // 2) * 3 * S * S
    t_mix = timed(lambda: ops.mixcut_u8(work, lam=lam), args.iters)
    t_cut = timed(lambda: ops.mixcut_u8(work, box=box), args.iters)
    ops.check_token_ids(wait=True)
    gbs = lambda ms: round(nbytes / ms / 1e6, 1)      # noqa: E731
    rec = {"device": torch.cuda.get_device_name(0), "batch": B, "classes": C, "image": "uint8 channels_last 224 px",
           "iters": args.iters, "mixcut_bytes": nbytes, "mixup_ms": round(t_mix, 4), "mixup_gbs": gbs(t_mix),
           "cutmix_ms": round(t_cut, 4), "cutmix_gbs_nominal": gbs(t_cut), "models": []}
    for name in args.models:
        r = model_record(name, img, C, args.iters)
        new = max(t_mix, t_cut) + r["head_fwd_bwd_ms"] + r["loss_fwd_bwd_ms"]
        r["new_launches_ms"] = round(new, 4)
        r["share_of_tower_step_pct"] = round(100.0 * new / r["tower_fwd_bwd_ms"], 3)
        rec["models"].append(r)
    print(json.dumps(rec), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("# Fine-tuning launches against the tower: tools/finetune_bench.py\n\n")
            f.write(f"Batch {B}, {C} classes, {rec['image']} images, {rec['device']}; HIP events, median of {args.iters} calls after 3 "
                    "warm-up calls (the tower: a quarter as many).  No gate: a record of one run.\n\n")
            f.write("| measurement | ms | GB/s |\n|---|---|---|\n")
            f.write(f"| `ops.mixcut_u8` mixup ({nbytes / 1e6:.0f} MB moved) | {rec['mixup_ms']} | {rec['mixup_gbs']} |\n")
            f.write(f"| `ops.mixcut_u8` cutmix (boxes of {side} px; GB/s as if every chunk moved) | {rec['cutmix_ms']} | {rec['cutmix_gbs_nominal']} |\n")
            for r in rec["models"]:
                f.write(f"| {r['model']}: head forward (E = {r['embed_dim']}) | {r['head_fwd_ms']} | |\n")
                f.write(f"| {r['model']}: head forward + backward | {r['head_fwd_bwd_ms']} | |\n")
                f.write(f"| {r['model']}: loss forward + backward | {r['loss_fwd_bwd_ms']} | |\n")
                f.write(f"| {r['model']}: tower forward + backward | {r['tower_fwd_bwd_ms']} | |\n")
                f.write(f"| {r['model']}: mixcut + head + loss = {r['share_of_tower_step_pct']} % of the tower | {r['new_launches_ms']} | |\n")
            f.write("\n```json\n" + json.dumps(rec) + "\n```\n")


if __name__ == "__main__":
    main()
