"""Generate tests/golden/distill_loss.npz from the REAL reference open_clip.loss.DistillClipLoss (CPU, fp32).

Run where the reference checkout is available (oracle/ref_loader.py finds it):  python tools/make_distill_golden.py
The GPU tests read the .npz and regenerate its inputs with `features` below; they never need the reference.  Cases:
  * W = 1, student E_s = 512, teacher E_t = 768, R = 64 and R = 100 (not a multiple of 8)      keys w1_r{R}_*
  * a 2-rank gloo group, all four local_loss x gather_with_grad variants                       keys w2_{ll}{gwg}_r{rank}_*
Each case stores both losses (contrastive, distill) and d/d student image features, text features and scale of their
sum (the reference trainer backpropagates sum(losses.values()), train.py:206-213).  To keep the fixture small the input
features are not stored: `features(n, e_s, e_t, seed)` regenerates them (numpy MT19937, rounded to bf16, the engine's
operand precision) from the seeds stored beside the results, and the feature gradients are stored as fp16 relative to
their largest magnitude, those with more than GRAD_SAMPLES entries as a fixed random sample of them plus the full norm
(`grad(z, key)` decodes them).  Scales are realistic (student 1/0.07, teacher 100) so both softmaxes are peaked.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, "tests", "golden", "distill_loss.npz")
E_S, E_T = 512, 768
W1_ROWS = (64, 100)
W2_B, W2_ES, W2_ET = 10, 128, 192          # per-rank batch 10: the gathered N = 20 is not a multiple of 8 either
SCALE_S, SCALE_T = 1.0 / 0.07, 100.0
W2_SEED = 303


def w1_seed(R):
    return 100 + R


def features(n, e_s, e_t, seed):
    """Paired, L2-normalised, bf16-representable student and teacher features [n, e] (fp32 arrays)."""
    rng = np.random.RandomState(seed)

    def pair(e, noise):
        base = rng.standard_normal((n, e))
        out = []
        for _ in range(2):
            x = torch.from_numpy(base + noise * rng.standard_normal((n, e))).float()
            x = x / x.norm(dim=-1, keepdim=True)
            out.append(x.to(torch.bfloat16).float().numpy())
        return out

    img, txt = pair(e_s, 1.5)
    dimg, dtxt = pair(e_t, 2.5)      # the teacher's softmax is peaked but not one-hot: distill != contrastive
    return img, txt, dimg, dtxt


GRAD_SAMPLES = 2048      # feature gradients larger than this are stored as a fixed random sample of their entries


def _put(arrays, prefix, lc, ld, gi, gt, gs):
    arrays.update({f"{prefix}_closs": lc, f"{prefix}_dloss": ld, f"{prefix}_gs": gs})
    for key, g in (("gi", gi), ("gt", gt)):
        flat = g.reshape(-1)
        arrays[f"{prefix}_{key}_norm"] = np.float32(np.linalg.norm(flat.astype(np.float64)))
        if flat.size > GRAD_SAMPLES:
            idx = np.sort(np.random.RandomState(flat.size).choice(flat.size, GRAD_SAMPLES, replace=False)).astype(np.int32)
            arrays[f"{prefix}_{key}_idx"] = idx
            flat = flat[idx]
        amax = np.float32(np.abs(flat).max())
        arrays[f"{prefix}_{key}"], arrays[f"{prefix}_{key}_amax"] = (flat / amax).astype(np.float16), amax


def grad(z, key):
    """Decode a stored feature gradient -> (fp32 values, flat indices into the gradient or None = all of it, full L2 norm)."""
    vals = z[key].astype(np.float32) * z[key + "_amax"]
    idx = z[key + "_idx"] if key + "_idx" in z.files else None
    return vals, idx, float(z[key + "_norm"])


def _run(ref_loss_mod, img, txt, dimg, dtxt, **kw):
    i = torch.from_numpy(img).clone().requires_grad_(True)
    t = torch.from_numpy(txt).clone().requires_grad_(True)
    s = torch.tensor(SCALE_S, requires_grad=True)
    fn = ref_loss_mod.DistillClipLoss(cache_labels=True, **kw)
    with torch.no_grad():
        di, dt, u = torch.from_numpy(dimg), torch.from_numpy(dtxt), torch.tensor(SCALE_T)
    out = fn(i, t, s, di, dt, u, output_dict=True)
    (out["contrastive_loss"] + out["distill_loss"]).backward()
    return (np.float32(out["contrastive_loss"].item()), np.float32(out["distill_loss"].item()), i.grad.numpy().copy(),
            t.grad.numpy().copy(), np.float32(s.grad.item()))


def _w2_worker(rank, world, port, q):
    import torch.distributed as dist
    from oracle import ref_loader
    torch.set_num_threads(1)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    _, ref_loss, _ = ref_loader.load()
    img, txt, dimg, dtxt = features(world * W2_B, W2_ES, W2_ET, seed=W2_SEED)
    sl = slice(rank * W2_B, (rank + 1) * W2_B)
    res = {}
    for local_loss in (True, False):
        for gwg in (True, False):
            res[f"{int(local_loss)}{int(gwg)}"] = _run(ref_loss, img[sl], txt[sl], dimg[sl], dtxt[sl], local_loss=local_loss,
                                                       gather_with_grad=gwg, rank=rank, world_size=world)
    q.put((rank, res))
    dist.barrier()
    dist.destroy_process_group()


def generate(port=29741):
    """-> dict of the fixture's arrays (deterministic: seeded inputs, single-threaded fp32 reference maths)."""
    from oracle import ref_loader
    import torch.multiprocessing as mp
    torch.set_num_threads(1)
    _, ref_loss, _ = ref_loader.load()
    arrays = {"scale_s": np.float32(SCALE_S), "scale_t": np.float32(SCALE_T)}
    for R in W1_ROWS:
        img, txt, dimg, dtxt = features(R, E_S, E_T, seed=w1_seed(R))
        arrays.update({f"w1_r{R}_seed": np.int64(w1_seed(R)), f"w1_r{R}_es": np.int64(E_S), f"w1_r{R}_et": np.int64(E_T)})
        _put(arrays, f"w1_r{R}", *_run(ref_loss, img, txt, dimg, dtxt))
    world = 2
    arrays.update({"w2_B": np.int64(W2_B), "w2_seed": np.int64(W2_SEED), "w2_es": np.int64(W2_ES), "w2_et": np.int64(W2_ET)})
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_w2_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=300) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        if p.exitcode != 0:
            raise RuntimeError(f"2-rank reference worker exited with {p.exitcode}")
    for rank in range(world):
        for key, vals in got[rank].items():
            _put(arrays, f"w2_{key}_r{rank}", *vals)
    return arrays


def main():
    arrays = generate()
    np.savez_compressed(OUT, **arrays)
    print(f"wrote {OUT}: " + ", ".join(f"{k}={float(v):.5f}" for k, v in arrays.items() if k.endswith("loss")))


if __name__ == "__main__":
    main()
