"""Few-shot linear probe (clipa_amd.fewshot.fewshot_lsr, csrc/fewshot.hip) vs the path a user had before it: copy the
features to the host and run the reference's regression in numpy fp32.
    python tools/fewshot_bench.py [--shape 10000x1024x1000x50000] [--iters 3] [--no-host] >> profiles/fewshot_bench.jsonl
One JSON line per N x D x C x Nt shape (N train rows in class order, N / C shots per class; prototypes plus noise):
  engine_ms          wall clock of one fewshot_lsr call, host ridge solve and its transfers included (median after a warm-up;
                     the call ends in a device synchronise)
  engine_kernels_ms  HIP-event time per kernel family inside one such call (ops.profile_start), and kernel_tflops for the two
                     products at their algorithmic FLOPs (gram: M^2 E, predict: 2 Nt C dim)
  host_copy_ms       features device -> host
  host_numpy_ms      whitening, z^T z or z z^T, eigh, weights, test logits and argmax in numpy fp32 (the reference's order);
                     median of the same number of runs after a warm-up, as engine_ms
  accuracies of both and the number of test rows on which the two predictions differ (near ties only: the host path
  rounds differently).
Every number is a measurement of the run that printed it, on the device named in the record."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clipa_amd import fewshot, ops  # noqa: E402

DEV = "cuda"
SHAPE = (10000, 1024, 1000, 50000)


def host_lsr(x, y, xt, num_classes, l2):
    """The reference's steps in numpy fp32 -> predictions [Nt]."""
    f = np.float32
    mean = x.mean(0, keepdims=True, dtype=f)
    std = np.sqrt(np.mean((x - mean) ** 2, axis=0, keepdims=True, dtype=f)) + f(1e-5)
    z = np.pad((x - mean) / std, ((0, 0), (0, 1)), constant_values=f(100.0))
    t = -np.ones((len(y), num_classes), dtype=f)
    t[np.arange(len(y)), y] = 1
    if z.shape[0] >= z.shape[1]:
        eigs, q = np.linalg.eigh(z.T @ z)
        rhs, lhs = q.T @ (z.T @ t), q
    else:
        eigs, q = np.linalg.eigh(z @ z.T)
        rhs, lhs = q.T @ t, z.T @ q
    w = (lhs * (f(1.0) / (eigs + f(l2))).reshape(1, -1)) @ rhs
    zt = np.pad((xt - mean) / std, ((0, 0), (0, 1)), constant_values=f(100.0))
    return np.argmax(zt @ w, axis=1)


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
    ap.add_argument("--shape", default="x".join(str(v) for v in SHAPE), help="NxDxCxNt")
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--l2", type=float, default=2.0 ** 10)
    ap.add_argument("--noise", type=float, default=3.0)
    ap.add_argument("--no-host", action="store_true", help="skip the host numpy path")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fewshot_bench: no GPU visible; nothing is measured without one")
    N, D, C, Nt = (int(v) for v in args.shape.split("x"))
    g = torch.Generator(device=DEV).manual_seed(N + D + C + Nt)
    proto = torch.randn(C, D, device=DEV, generator=g)
    y = torch.arange(C, device=DEV).repeat_interleave((N + C - 1) // C)[:N]
    yt = torch.randint(0, C, (Nt,), device=DEV, generator=g)
    x = proto[y] + args.noise * torch.randn(N, D, device=DEV, generator=g)
    xt = proto[yt] + args.noise * torch.randn(Nt, D, device=DEV, generator=g)
    y_h, yt_h = y.cpu().numpy(), yt.cpu().numpy()

    run = lambda: fewshot.fewshot_lsr(x, y_h, xt, yt_h, C, args.l2, return_predictions=True)      # noqa: E731
    ms, out = wall(run, args.iters)
    ops.profile_start()
    run()
    prof = ops.profile_stop()
    dim = D + 1
    rec = {"N": N, "D": D, "C": C, "Nt": Nt, "l2": args.l2, "route": out["route"], "device": torch.cuda.get_device_name(0),
           "engine_ms": round(ms, 2), "engine_accuracy": float(out["accuracy"]),
           "engine_kernels_ms": {k: round(v["ms"], 3) for k, v in sorted(prof.items())},
           "kernel_tflops": {k: round(v["work"] / v["ms"] / 1e9, 1) for k, v in sorted(prof.items()) if v["work"] and v["ms"]},
           "gram_shape": [dim, N] if out["route"] == "A" else [N, dim]}
    if not args.no_host:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        x_h, xt_h = x.cpu().numpy(), xt.cpu().numpy()
        copy_ms = (time.perf_counter() - t0) * 1e3
        host_lsr(x_h, y_h, xt_h, C, args.l2)      # warm-up, as the engine's
        ts = []
        for _ in range(args.iters):
            t0 = time.perf_counter()
            pred_h = host_lsr(x_h, y_h, xt_h, C, args.l2)
            ts.append((time.perf_counter() - t0) * 1e3)
        ts.sort()
        host_ms = ts[len(ts) // 2]
        rec.update({"host_copy_ms": round(copy_ms, 2), "host_numpy_ms": round(host_ms, 2), "iters": args.iters,
                    "host_threads": int(os.environ.get("OMP_NUM_THREADS", 0)) or None,
                    "host_accuracy": float(np.mean(pred_h == yt_h)),
                    "pred_disagree": int((pred_h != out["pred"].cpu().numpy()).sum()),
                    "speedup_vs_host": round((copy_ms + host_ms) / ms, 2)})
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
