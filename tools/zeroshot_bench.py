"""Fused fp32 zero-shot evaluation (clipa_amd.zero_shot.build_classifier / evaluate_zero_shot, csrc/zeroshot.hip) vs the path a
user had before it (zero_shot_classifier + run of the same module: one encode_text per class, bf16 logits, torch.topk).
    python tools/zeroshot_bench.py [--shape 50000x1000x768] [--templates 80] [--batch 1000] [--iters 3] >> profiles/zeroshot_bench.jsonl
One JSON line per B x C x E shape.  The towers are a stand-in that returns planted unit-norm features (prototypes plus noise), so
what is timed is everything around the towers: for the classifier the per-class loop (C small launches chains) against
ceil(C T / 1024) chunks and one class-mean kernel, for the evaluation the bf16 casts, the [b, C] logit GEMM and topk per batch
against one rank kernel per batch.  A real text tower adds its own time to both sides, and C launch-bound runs of T prompts to
the old one only.
  classifier_old_ms / classifier_new_ms   wall clock of one call (median after a warm-up, ending in a device synchronise)
  eval_old_ms / eval_new_ms               the same for `run` / `evaluate_zero_shot` over B / batch batches
  new_kernels_ms                          HIP-event time per kernel family inside one new classifier + evaluation (ops.profile_start)
  top-1 / top-5 of both, and pred_disagree: images whose bf16-logit argmax differs from the fp32 rank kernel's.
There is no pass / fail threshold.  Every number is a measurement of the run that printed it, on the device named in the record."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clipa_amd import ops, zero_shot  # noqa: E402

DEV = "cuda"
SHAPE = (50000, 1000, 768)


class Planted(torch.nn.Module):
    """encode_text: column 0 of a token row is the prompt's row in prompt_emb; encode_image: an "image" is its row in feat."""

    def __init__(self, prompt_emb, feat):
        super().__init__()
        self.prompt_emb, self.feat = prompt_emb, feat

    def encode_text(self, tokens, normalize=False):
        return self.prompt_emb[tokens[:, 0]]

    def encode_image(self, images, normalize=False):
        return self.feat[images]


def wall(fn, iters):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="x".join(str(v) for v in SHAPE), help="BxCxE")
    ap.add_argument("--templates", type=int, default=80)
    ap.add_argument("--batch", type=int, default=1000)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--noise", type=float, default=8.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("zeroshot_bench: no GPU visible; nothing is measured without one")
    B, C, E = (int(v) for v in args.shape.split("x"))
    T = args.templates
    g = torch.Generator(device=DEV).manual_seed(B + C + E)
    norm = torch.nn.functional.normalize
    proto = torch.randn(C, E, device=DEV, generator=g)
    prompt_emb = norm(proto.repeat_interleave(T, 0) + 0.5 * torch.randn(C * T, E, device=DEV, generator=g), dim=1)
    y = torch.randint(0, C, (B,), device=DEV, generator=g)
    feat = norm(proto[y] + args.noise * torch.randn(B, E, device=DEV, generator=g), dim=1)
    model = Planted(prompt_emb, feat).eval()
    tokens = torch.zeros((C * T, 8), device=DEV, dtype=torch.int64)
    tokens[:, 0] = torch.arange(C * T, device=DEV)
    prompt_class = torch.arange(C).repeat_interleave(T).numpy()
    idx = torch.arange(B, device=DEV)
    batches = [(idx[i:i + args.batch], y[i:i + args.batch]) for i in range(0, B, args.batch)]

    old_clf_ms, (clf_old, n) = wall(lambda: zero_shot.zero_shot_classifier(model, tokens.view(C, T, -1)), args.iters)
    new_clf_ms, clf_new = wall(lambda: zero_shot.build_classifier(model, tokens, prompt_class, C), args.iters)
    old_eval_ms, old_acc = wall(lambda: zero_shot.run(model, clf_old, n, batches), args.iters)
    new_eval_ms, new_acc = wall(lambda: zero_shot.evaluate_zero_shot(model, clf_new, {"bench": batches}), args.iters)
    ops.profile_start()
    zero_shot.evaluate_zero_shot(model, zero_shot.build_classifier(model, tokens, prompt_class, C), {"bench": batches})
    prof = ops.profile_stop()
    disagree = 0
    for images, _ in batches:
        old_pred = zero_shot.zero_shot_logits(model, clf_old, n, images).argmax(1)
        disagree += int((old_pred != zero_shot.zero_shot_ranks(feat[images], clf_new, y[images])["pred"]).sum())
    rec = {"B": B, "C": C, "E": E, "templates": T, "batch": args.batch, "iters": args.iters, "device": torch.cuda.get_device_name(0),
           "classifier_old_ms": round(old_clf_ms, 2), "classifier_new_ms": round(new_clf_ms, 2),
           "eval_old_ms": round(old_eval_ms, 2), "eval_new_ms": round(new_eval_ms, 2),
           "new_kernels_ms": {k: round(v["ms"], 3) for k, v in sorted(prof.items())},
           "kernel_tflops": {k: round(v["work"] / v["ms"] / 1e9, 1) for k, v in sorted(prof.items()) if v["work"] and v["ms"]},
           "old_top1": old_acc[0], "old_top5": old_acc[1], "new_top1": float(new_acc["bench-top1"]),
           "new_top5": float(new_acc["bench-top5"]), "pred_disagree": disagree}
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
