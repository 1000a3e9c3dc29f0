"""The attention-pooling kernels (clipa_amd.ops.mappool_fwd / mappool_bwd, csrc/mappool.hip) against their byte floor, beside the
existing mean-pooling head (ops.pool_fwd / pool_bwd with POOL_MEAN_ALL), which reads and writes the same bytes.
    python tools/mappool_bench.py [--shape 4096x197x1024x16 ...] [--iters 20] >> profiles/mappool_bench.jsonl
One JSON line per B x L x D x H shape (B is halved until the tensors fit in a third of the free memory):
  fwd_ms / bwd_ms            HIP-event time of one call, median of --iters calls after 3 warm-up calls on random data
                             (bwd_ms includes the operand-transpose and the
                             partial-reduction kernels of clipa_mappool_bwd)
  fwd_gbs / bwd_gbs          the byte floor over that time: 2 B L D bytes forward (x read once), 4 B L D backward (x read, dx
                             written); z, dz, U and the workspace are not counted
  meanpool_fwd_ms / _bwd_ms  ops.pool_fwd / pool_bwd at the same shape, the same way; their floors are 2 B L D each (pool_bwd
                             reads no x)
No time is gated.  Every number is a measurement of the run that printed it, on the device named in the record."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clipa_amd import ops  # noqa: E402

DEV = "cuda"
SHAPES = ["4096x197x1024x16", "2048x257x1280x16", "4096x50x768x12"]


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
    return ts[len(ts) // 2], ts[0], ts[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", nargs="*", default=SHAPES, help="BxLxDxH")
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mappool_bench: no GPU visible; nothing is measured without one")
    for shape in args.shape:
        B, L, D, H = (int(v) for v in shape.split("x"))
        asked = B
        free = torch.cuda.mem_get_info()[0]
        while B > 1 and 3 * (4 * B * L * D + 12 * B * H * D) > free:      # x and dx, z / dz / workspace, twice over for slack
            B //= 2
        g = torch.Generator(device=DEV).manual_seed(B + L + D + H)
        x = (torch.randn(B * L, D, device=DEV, generator=g)).to(torch.bfloat16)
        u = (torch.randn(H, D, device=DEV, generator=g) * D ** -0.5).to(torch.bfloat16)
        dz = torch.randn(B, H, D, device=DEV, generator=g)
        z, stats = ops.mappool_fwd(x, u, B, L, H)
        pooled = ops.pool_fwd(x, B, L, ops.POOL_MEAN_ALL)
        fwd = timed(lambda: ops.mappool_fwd(x, u, B, L, H), args.iters)
        bwd = timed(lambda: ops.mappool_bwd(x, u, z, stats, dz, B, L, H), args.iters)
        mfwd = timed(lambda: ops.pool_fwd(x, B, L, ops.POOL_MEAN_ALL), args.iters)
        mbwd = timed(lambda: ops.pool_bwd(pooled, B, L, ops.POOL_MEAN_ALL), args.iters)
        floor = 2.0 * B * L * D
        gbs = lambda nbytes, ms: round(nbytes / ms / 1e6, 1)      # noqa: E731
        rec = {"B": B, "B_asked": asked, "L": L, "D": D, "H": H, "device": torch.cuda.get_device_name(0), "iters": args.iters,
               "fwd_ms": round(fwd[0], 3), "fwd_ms_min_max": [round(fwd[1], 3), round(fwd[2], 3)], "fwd_gbs": gbs(floor, fwd[0]),
               "bwd_ms": round(bwd[0], 3), "bwd_ms_min_max": [round(bwd[1], 3), round(bwd[2], 3)], "bwd_gbs": gbs(2 * floor, bwd[0]),
               "meanpool_fwd_ms": round(mfwd[0], 3), "meanpool_fwd_gbs": gbs(floor, mfwd[0]),
               "meanpool_bwd_ms": round(mbwd[0], 3), "meanpool_bwd_gbs": gbs(floor, mbwd[0]),
               "floor_bytes_fwd": floor, "floor_bytes_bwd": 2 * floor}
        print(json.dumps(rec), flush=True)
        del x, dz, z, stats, pooled


if __name__ == "__main__":
    main()
