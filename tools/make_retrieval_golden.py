"""Generate tests/golden/retrieval_metrics.npz from the REAL reference get_clip_metrics (training/train.py:432-449, CPU).

Run where the reference checkout is available (oracle/ref_loader.py finds it):  python tools/make_retrieval_golden.py
The GPU tests read the .npz and regenerate the inputs with `features` below; they never need the reference.  Cases:
  * A: N = 2000, E = 512, scale 100.  No near ties: for every row and column every |x_ij - x_ii| (j != i) exceeds 1e-4 in
       fp64, so the reference's fp32 summation order cannot change a rank and the engine must match it exactly.
  * B: N = 1531 (not a multiple of the kernel's 128-row tile), E = 768, scale 1/0.07, about 5 % of the captions duplicates
       of other captions: exact ties in image -> text.  Every other entry is again at least 1e-4 from its positive.
Features: shared concept vectors (a duplicated caption's image shares its source's concept) plus independent image and
text noise, L2-normalised, fp32.  A pair whose row or column has a near tie is redrawn with fresh noise; `redraws`
(stored) says how often, so `features` is a pure function of the stored seed and redraws (the duplicate map follows from
the seed).  Stored: seeds, redraws, the reference's 10 metrics and its preds in both directions.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, "tests", "golden", "retrieval_metrics.npz")
CASES = {"A": dict(n=2000, e=512, scale=100.0, dup=0.0, noise=2.7, seed=4001),
         "B": dict(n=1531, e=768, scale=1.0 / 0.07, dup=0.05, noise=2.6, seed=4002)}
MARGIN = 1e-4
KEYS = [f"{d}_{m}" for d in ("image_to_text", "text_to_image") for m in ("mean_rank", "median_rank", "R@1", "R@5", "R@10")]


def duplicates(n, frac, seed):
    """dup[i] = index of the caption that caption i copies, or -1.  Sources are never copies themselves."""
    dup = np.full(n, -1, dtype=np.int64)
    if frac <= 0:
        return dup
    rng = np.random.RandomState(seed + 7)
    perm = rng.permutation(n)
    m = int(round(frac * n))
    dup[perm[:m]] = perm[m:2 * m]
    return dup


def features(n, e, noise, seed, redraws, dup):
    """-> image, text features fp32 [n, e] (L2-normalised rows; text i == text dup[i] where dup[i] >= 0)."""
    base = np.random.RandomState(seed).standard_normal((n, e))
    src = dup >= 0
    base[src] = base[dup[src]]                  # a duplicated caption describes a second image of the same concept
    img = np.empty((n, e))
    txt = np.empty((n, e))
    for i in range(n):
        rng = np.random.RandomState([seed, i, int(redraws[i])])
        img[i] = base[i] + noise * rng.standard_normal(e)
        txt[i] = base[i] + noise * rng.standard_normal(e)
    img = torch.from_numpy(img).float()
    txt = torch.from_numpy(txt).float()
    img = (img / img.norm(dim=-1, keepdim=True)).numpy()
    txt = (txt / txt.norm(dim=-1, keepdim=True)).numpy()
    txt[src] = txt[dup[src]]
    return img, txt


def near_ties(img, txt, dup):
    """Pairs i whose row i or column i holds an entry within MARGIN of the positive that is not an exact duplicate."""
    x = img.astype(np.float64) @ txt.astype(np.float64).T
    d = np.diag(x).copy()
    n = len(d)
    same_txt = np.arange(n)[None, :] == np.arange(n)[:, None]
    for i in np.nonzero(dup >= 0)[0]:           # text i == text dup[i]: row i ties exactly at column dup[i] and vice versa
        same_txt[i, dup[i]] = same_txt[dup[i], i] = True
        for k in np.nonzero(dup == dup[i])[0]:
            same_txt[i, k] = True
    row_bad = ((np.abs(x - d[:, None]) <= MARGIN) & ~same_txt).any(axis=1)
    col_bad = ((np.abs(x - d[None, :]) <= MARGIN) & ~np.eye(n, dtype=bool)).any(axis=0)
    return np.nonzero(row_bad | col_bad)[0]


def case_inputs(name, redraws=None):
    c = CASES[name]
    dup = duplicates(c["n"], c["dup"], c["seed"])
    if redraws is None:
        redraws = np.zeros(c["n"], dtype=np.int64)
    return features(c["n"], c["e"], c["noise"], c["seed"], redraws, dup), dup


def solve_redraws(name):
    """Redraw the pairs with near ties until there are none; -> redraws [n]."""
    c = CASES[name]
    redraws = np.zeros(c["n"], dtype=np.int64)
    for _ in range(50):
        (img, txt), dup = case_inputs(name, redraws)
        bad = near_ties(img, txt, dup)
        if len(bad) == 0:
            return redraws
        redraws[bad] += 1
    raise RuntimeError(f"case {name}: near ties remain")


def ref_preds(logits):
    """The reference's own preds (train.py:441-443) from a logit matrix."""
    gt = torch.arange(logits.shape[0]).view(-1, 1)
    ranking = torch.argsort(logits, descending=True)
    return torch.where(ranking == gt)[1].numpy()


def generate():
    from oracle import trainer_harness
    torch.set_num_threads(1)
    train = trainer_harness.load_trainer("reference")
    try:
        arrays = {}
        for name, c in CASES.items():
            redraws = solve_redraws(name)
            (img, txt), dup = case_inputs(name, redraws)
            assert len(near_ties(img, txt, dup)) == 0
            it, tt, s = torch.from_numpy(img), torch.from_numpy(txt), torch.tensor(c["scale"])
            metrics = train.get_clip_metrics(image_features=it, text_features=tt, logit_scale=s)
            logits = (s * it @ tt.t()).detach()                       # the same expression as train.py:434
            i2t, t2i = ref_preds(logits), ref_preds(logits.t())
            assert np.isclose(i2t.mean() + 1, metrics["image_to_text_mean_rank"])
            arrays.update({f"{name}_{k}": np.int64(c[k]) for k in ("n", "e", "seed")})
            arrays.update({f"{name}_scale": np.float64(c["scale"]), f"{name}_noise": np.float64(c["noise"]),
                           f"{name}_dup_frac": np.float64(c["dup"]), f"{name}_redraws": redraws.astype(np.int8),
                           f"{name}_i2t": i2t.astype(np.int16), f"{name}_t2i": t2i.astype(np.int16)})
            arrays[f"{name}_metric_keys"] = np.array(KEYS)
            arrays[f"{name}_metrics"] = np.array([np.float64(metrics[k]) for k in KEYS])
            print(name, {k: round(float(metrics[k]), 4) for k in KEYS}, "redrawn pairs:", int((redraws > 0).sum()))
    finally:
        trainer_harness.unload()
    return arrays


def main():
    arrays = generate()
    np.savez_compressed(OUT, **arrays)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
