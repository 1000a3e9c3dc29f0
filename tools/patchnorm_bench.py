"""What dual PatchNorm (input_patchnorm) costs in the image stem, and ops.patchify_ln against ops.patchify, from one run.
    python tools/patchnorm_bench.py [--batch 256] [--iters 20] [--out profiles/patchnorm_bench.md]
ViT-B/16 at 224 px, uint8 channels_last images (the loader's format).  Measured with HIP events, median of --iters calls after 3
warm-up calls:
  patchify / patchify_ln     one call each on the same images; GB/s = (image bytes + 2 * rows * Kp output bytes) / time
  stem fwd+bwd               engine.VisionStemFn forward + backward (every stem parameter trainable) of `ViT-B-16` and of
                             `ViT-B-16-patchnorm`, with a random gradient of the stem's output; the weight cache is warm (the fold
                             runs once per optimizer step, not per call) ...
  patchnorm_fold / _unfold   ... so the two glue launches are timed on their own: fold is paid once per optimizer step, unfold
                             once per backward (it is inside the stem time above)
No time is gated.  Every number is a measurement of the run that printed it, on the device named in the record."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import clipa_amd  # noqa: E402
from clipa_amd import engine, ops  # noqa: E402

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


def stem_step(name, img, iters):
    """Median ms of the stem's forward + backward of the built-in config `name`."""
    torch.manual_seed(0)
    v = clipa_amd.create_model(name, device=DEV).visual
    B, S, P = img.shape[0], img.shape[2], v.patch_size[0]
    L = (S // P) ** 2 + 1
    cfg = engine.StemCfg(B=B, L=L, P=P, Kp=(3 * P * P + 7) // 8 * 8, eps=1e-5, ln_pre=True, mean=v.image_mean, std=v.image_std,
                         patchnorm=v.input_patchnorm)
    pn = (v.conv1.bias, v.patchnorm_pre_ln.weight, v.patchnorm_pre_ln.bias) if v.input_patchnorm else ()
    params = (v.conv1.weight, v.class_embedding, v.positional_embedding, v.ln_pre.weight, v.ln_pre.bias) + pn
    dy = torch.randn(B * L, v.conv1.weight.shape[0], device=DEV).to(torch.bfloat16)

    def step():
        x0 = engine.VisionStemFn.apply(img, cfg, v._cache, *params)
        torch.autograd.grad(x0, params, dy)
    return timed(step, iters)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the record as a markdown file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("patchnorm_bench: no GPU visible; nothing is measured without one")
    B, S, P, D = args.batch, 224, 16, 768
    K = Kp = 3 * P * P
    g = torch.Generator(device=DEV).manual_seed(B)
    img = torch.randint(0, 256, (B, 3, S, S), device=DEV, dtype=torch.uint8, generator=g).contiguous(memory_format=torch.channels_last)
    mean, std = clipa_amd.model.OPENAI_DATASET_MEAN, clipa_amd.model.OPENAI_DATASET_STD
    rows = B * (S // P) ** 2
    nbytes = float(img.numel()) + 2.0 * rows * Kp
    t_p = timed(lambda: ops.patchify(img, P, Kp, mean, std), args.iters)
    t_pl = timed(lambda: ops.patchify_ln(img, P, Kp, mean, std), args.iters)
    w, b = torch.randn(D, K, device=DEV, generator=g) * 0.03, torch.randn(D, device=DEV, generator=g) * 0.1
    gamma, beta = torch.randn(K, device=DEV, generator=g), torch.randn(K, device=DEV, generator=g) * 0.3
    G, s = torch.randn(D, Kp, device=DEV, generator=g), torch.randn(D, device=DEV, generator=g)
    t_fold = timed(lambda: ops.patchnorm_fold(w, b, gamma, beta, P, Kp), args.iters)
    t_unfold = timed(lambda: ops.patchnorm_unfold(G, s, w, gamma, beta, P), args.iters)
    t_plain = stem_step("ViT-B-16", img, args.iters)
    t_pn = stem_step("ViT-B-16-patchnorm", img, args.iters)
    gbs = lambda ms: round(nbytes / ms / 1e6, 1)      # noqa: E731
    rec = {"device": torch.cuda.get_device_name(0), "model": "ViT-B/16 @ 224", "batch": B, "input": "uint8 channels_last",
           "iters": args.iters, "patch_rows": rows, "Kp": Kp, "patchify_bytes": nbytes,
           "patchify_ms": round(t_p, 4), "patchify_gbs": gbs(t_p), "patchify_ln_ms": round(t_pl, 4), "patchify_ln_gbs": gbs(t_pl),
           "patchnorm_fold_ms": round(t_fold, 4), "patchnorm_unfold_ms": round(t_unfold, 4),
           "stem_fwd_bwd_ms": round(t_plain, 4), "stem_fwd_bwd_patchnorm_ms": round(t_pn, 4),
           "stem_delta_ms": round(t_pn - t_plain, 4)}
    print(json.dumps(rec), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("# Dual PatchNorm stem: tools/patchnorm_bench.py\n\n")
            f.write(f"{rec['model']}, batch {B}, {rec['input']} images, {rec['device']}; HIP events, median of {args.iters} calls "
                    "after 3 warm-up calls.  No gate: a record of one run.\n\n")
            f.write("| measurement | ms | GB/s |\n|---|---|---|\n")
            f.write(f"| `ops.patchify` ({rows} x {Kp} bf16 out) | {rec['patchify_ms']} | {rec['patchify_gbs']} |\n")
            f.write(f"| `ops.patchify_ln` (same bytes) | {rec['patchify_ln_ms']} | {rec['patchify_ln_gbs']} |\n")
            f.write(f"| `ops.patchnorm_fold` ({D} x {K}, once per optimizer step) | {rec['patchnorm_fold_ms']} | |\n")
            f.write(f"| `ops.patchnorm_unfold` ({D} x {K}, once per backward) | {rec['patchnorm_unfold_ms']} | |\n")
            f.write(f"| stem forward + backward, `ViT-B-16` | {rec['stem_fwd_bwd_ms']} | |\n")
            f.write(f"| stem forward + backward, `ViT-B-16-patchnorm` | {rec['stem_fwd_bwd_patchnorm_ms']} | |\n")
            f.write(f"| difference | {rec['stem_delta_ms']} | |\n\n")
            f.write("```json\n" + json.dumps(rec) + "\n```\n")


if __name__ == "__main__":
    main()
