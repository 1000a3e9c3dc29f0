"""One objective-and-gradient evaluation of the logistic-regression linear probe (clipa_amd.linear_probe, csrc/logreg.hip) vs
the same evaluation written with stock PyTorch fp32 (TF32 off) on the same GPU.
    python tools/linear_probe_bench.py --shape 1281167x1024x1000 [--iters 3] [--no-torch] >> profiles/linear_probe_bench.jsonl
    python tools/linear_probe_bench.py --shape 50000x768x100 >> profiles/linear_probe_bench.jsonl
One JSON line per N x D x C shape (random features and weights: the arithmetic does not depend on the values):
  prepare_ms         X~ and X~^T, once per fit
  engine_ms          wall clock of one logreg_objective call, transfers of theta and g and the host's fp64 included (median after
                     a warm-up; the call ends in a device synchronise)
  engine_kernels_ms  HIP-event time per kernel inside one such call (ops.profile_start), and kernel_tflops for the two
                     products at their algorithmic FLOPs (2 N C (D + 1) each)
  torch_ms           logits = X~ theta^T, logsumexp, cross entropy, softmax - onehot, its product with X~: device time by HIP
                     events (median after a warm-up), torch_tflops for the two matmuls alone timed the same way
  the largest differences between the two paths' f and g.
Every number is a measurement of the run that printed it, on the device named in the record.  Run each shape as its own
process under its own time limit, the steps chained with &&."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clipa_amd import linear_probe as P, ops  # noqa: E402

DEV = "cuda"


def device_ms(fn, iters):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2], out


def wall_ms(fn, iters):
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
    ap.add_argument("--shape", required=True, help="NxDxC")
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--l2", type=float, default=1e-3)
    ap.add_argument("--no-torch", action="store_true", help="skip the stock PyTorch path")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("linear_probe_bench: no GPU visible; nothing is measured without one")
    N, D, C = (int(v) for v in args.shape.split("x"))
    dim = D + 1
    g = torch.Generator(device=DEV).manual_seed(N + D + C)
    x = torch.randn(N, D, device=DEV, generator=g)
    y = torch.randint(0, C, (N,), device=DEV, generator=g)
    theta = (0.05 * torch.randn(C, dim, device=DEV, generator=g)).cpu().numpy().astype(np.float64)
    y_h = y.cpu().numpy()

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    prep = P.Prepared(x)
    torch.cuda.synchronize()
    prepare_ms = (time.perf_counter() - t0) * 1e3
    obj = P._Objective(prep, y.int(), C, args.l2)
    run = lambda: (obj.value(theta), obj.grad())      # noqa: E731
    ms, (f, grad) = wall_ms(run, args.iters)
    ops.profile_start()
    run()
    prof = ops.profile_stop()
    rec = {"N": N, "D": D, "C": C, "device": torch.cuda.get_device_name(0), "iters": args.iters,
           "prepare_ms": round(prepare_ms, 2), "engine_ms": round(ms, 2),
           "engine_kernels_ms": {k: round(v["ms"], 3) for k, v in sorted(prof.items())},
           "kernel_tflops": {k: round(v["work"] / v["ms"] / 1e9, 1) for k, v in sorted(prof.items()) if v["work"] and v["ms"]},
           "logits_bytes": 4 * C * N, "workspace_bytes": int(ops.lib.query("clipa_logreg_grad_workspace", C, dim, N, 0))}
    if not args.no_torch:
        torch.backends.cuda.matmul.allow_tf32 = False
        torch.set_float32_matmul_precision("highest")
        xp = prep.xp
        th = torch.from_numpy(theta.astype(np.float32)).to(DEV)
        rows = torch.arange(N, device=DEV)

        def torch_eval():
            z = xp @ th.t()
            lse = torch.logsumexp(z, dim=1)
            ce = (lse - z[rows, y]).sum(dtype=torch.float64)
            p = torch.exp(z - lse[:, None])
            p[rows, y] -= 1.0
            return ce, p.t() @ xp

        t_ms, (ce, gt) = device_ms(torch_eval, args.iters)
        p = torch.empty(N, C, device=DEV)
        mm1, _ = device_ms(lambda: xp @ th.t(), args.iters)
        mm2, _ = device_ms(lambda: p.t() @ xp, args.iters)
        f_t = float(ce) / N + 0.5 * args.l2 * float(np.sum(theta[:, :-1] ** 2))
        g_t = gt.cpu().numpy().astype(np.float64) / N
        g_t[:, :-1] += args.l2 * theta[:, :-1]
        flops = 2.0 * N * C * dim
        rec.update({"torch_ms": round(t_ms, 2), "torch_matmul_ms": {"logits": round(mm1, 3), "grad": round(mm2, 3)},
                    "torch_tflops": {"logits": round(flops / mm1 / 1e9, 1), "grad": round(flops / mm2 / 1e9, 1)},
                    "f_diff": abs(f - f_t), "g_diff_max": float(np.abs(grad - g_t).max()),
                    "engine_kernels_vs_torch": round(sum(v["ms"] for v in prof.values()) / t_ms, 2)})
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
