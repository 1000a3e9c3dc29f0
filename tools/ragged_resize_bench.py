"""The ragged device resampler (clipa_resample_ragged_u8, csrc/resample_ragged.hip) against its two yardsticks.
    python tools/ragged_resize_bench.py [--cases uniform,imagenet-mix] [--iters 5] >> profiles/ragged_resize_bench.jsonl
One JSON line per case:
  uniform        4096 x 256 x 256 -> 224, RandomResizedCrop boxes at scale (0.4, 1): the same staged batch and the same boxes
                 through the ragged entry and through the untouched clipa_resized_crop_u8.  Both move the same bytes; the ragged
                 path adds a descriptor table, a validation launch and a block-to-sample lookup.  `ratio` = ragged / uniform
                 device time; the expectation recorded in DESIGN section 7 is <= 1.25.
  imagenet-mix   --images decoded images of ImageNet-like mixed sizes (sides 120 .. 800, a few multi-megapixel photographs)
                 -> the 224 inference transform: DeviceEvalTransform on one packed batch against
                 clipa_amd.transform.image_transform(is_train=False) (Pillow) on --procs host processes.
`*_dev_ms` are HIP-event times of the launches (ops.profile_start), `*_wall_ms` wall clock of the whole call ending in a device
synchronise (host layout and the descriptor copy included); each is the median of --iters runs after one warm-up.  The host
side is timed once over all images, decoded arrays in, uint8 CHW tensors out.  Outputs are compared byte for byte (`equal`).
There is no pass / fail threshold.  Every number is a measurement of the run that printed it, on the device named in the record."""
import argparse
import json
import multiprocessing
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clipa_amd import data as D  # noqa: E402
from clipa_amd import transform as T  # noqa: E402

DEV = "cuda"
_IMAGES = None      # the decoded images, inherited by the forked host workers


def _host_one(i):
    from PIL import Image
    return T.image_transform(224, is_train=False, to_float_on_device=True)(Image.fromarray(_IMAGES[i])).numpy()


def mixed_images(n, seed=0):
    rng = np.random.default_rng(seed)
    sizes = [(int(rng.integers(120, 801)), int(rng.integers(120, 801))) for _ in range(n)]
    for k, hw in enumerate(((3000, 4000), (2448, 3264), (4000, 3000), (1080, 1920))):
        if k < n:
            sizes[k * (n // 4)] = hw
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]


def host_transform(procs):
    """Every image through the Pillow transform on `procs` forked processes -> (seconds, uint8 [N, 3, 224, 224])."""
    with multiprocessing.get_context("fork").Pool(procs) as pool:
        pool.map(_host_one, range(min(len(_IMAGES), 2 * procs)))          # workers started, Pillow imported
        t0 = time.perf_counter()
        out = pool.map(_host_one, range(len(_IMAGES)), chunksize=4)
        return time.perf_counter() - t0, np.stack(out)


def timed(fn, iters, key):
    """-> (median wall ms, median device ms of the launches recorded under `key`, last result)."""
    from clipa_amd import ops
    fn()
    torch.cuda.synchronize()
    wall, dev = [], []
    for _ in range(iters):
        ops.profile_start()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(ops.profile_stop()[key]["ms"])
    return sorted(wall)[iters // 2], sorted(dev)[iters // 2], out


def main():
    global _IMAGES
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="uniform,imagenet-mix")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--images", type=int, default=512)
    ap.add_argument("--procs", type=int, default=16)
    args = ap.parse_args()
    cases = args.cases.split(",")
    host = None
    if "imagenet-mix" in cases:       # the host side first: its workers are forked before this process opens the GPU
        _IMAGES = mixed_images(args.images)
        host = host_transform(args.procs)
    if not torch.cuda.is_available():
        raise SystemExit("ragged_resize_bench: no GPU visible; nothing is measured without one")
    from clipa_amd import ops
    name = torch.cuda.get_device_name(0)
    if "uniform" in cases:
        B, Hs, S = 4096, 256, 224
        g = torch.Generator().manual_seed(7)
        base = torch.randint(0, 256, (64, Hs, Hs, 3), generator=g, dtype=torch.uint8).to(DEV)
        src = base.repeat(B // 64, 1, 1, 1).contiguous()
        boxes = D.sample_crop_boxes(B, Hs, Hs, (0.4, 1.0), (3 / 4, 4 / 3), g)
        d_boxes = boxes.to(DEV)
        geometry = torch.cat([boxes, torch.tensor([[S, S, 0, 0]], dtype=torch.int32).repeat(B, 1)], 1)
        ragged = D.RaggedImages.from_uniform(src)
        u_wall, u_dev, u_out = timed(lambda: ops.resized_crop_u8(src, d_boxes, S), args.iters, "resized_crop")
        r_wall, r_dev, r_out = timed(lambda: ops.resample_ragged_u8(ragged, geometry, S), args.iters, "resample_ragged")
        print(json.dumps({"case": "uniform", "B": B, "source": [Hs, Hs], "size": S, "iters": args.iters, "device": name,
                          "uniform_dev_ms": round(u_dev, 3), "ragged_dev_ms": round(r_dev, 3), "ratio": round(r_dev / u_dev, 3),
                          "uniform_wall_ms": round(u_wall, 3), "ragged_wall_ms": round(r_wall, 3),
                          "equal": bool(torch.equal(u_out, r_out))}), flush=True)
        del src, ragged, u_out, r_out
    if "imagenet-mix" in cases:
        host_s, host_out = host
        t0 = time.perf_counter()
        packed = D.pack_images(_IMAGES, pinned=True)
        pack_ms = (time.perf_counter() - t0) * 1e3
        tf = D.DeviceEvalTransform(224)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        on_dev = packed.to(DEV, non_blocking=True)
        torch.cuda.synchronize()
        h2d_ms = (time.perf_counter() - t0) * 1e3
        wall, dev, out = timed(lambda: tf(on_dev), args.iters, "resample_ragged")
        n = len(_IMAGES)
        print(json.dumps({"case": "imagenet-mix", "images": n, "megabytes": round(packed.data.numel() / 1e6, 1), "size": 224,
                          "iters": args.iters, "device": name, "host_procs": args.procs, "host_s": round(host_s, 3),
                          "host_images_per_s": round(n / host_s, 1), "pack_ms": round(pack_ms, 3), "h2d_ms": round(h2d_ms, 3),
                          "device_dev_ms": round(dev, 3), "device_wall_ms": round(wall, 3),
                          "device_images_per_s": round(n / (wall / 1e3), 1),
                          "device_images_per_s_with_pack_and_copy": round(n / ((wall + pack_ms + h2d_ms) / 1e3), 1),
                          "equal": bool(np.array_equal(out.cpu().numpy(), host_out))}), flush=True)
    ops.check_token_ids(wait=True)


if __name__ == "__main__":
    main()
