"""Generate tests/golden/zeroshot.npz: synthetic zero-shot classification cases with well-defined per-row ranks.

The expected values come from the host restatements of tests/zeroshot_cases.py: `ranks_fp64` (float64 products of the float32
inputs) gives gt / eq / pred, `chain_fp32` (the engine's ascending-k float32 chain) the size of float32 noise.  Run (numpy
only):
    python tools/make_zeroshot_golden.py
The tests read the .npz and regenerate the inputs with `case_inputs` / `classmean_inputs`; they never need anything else.

Cases: class prototypes proto [C, E] ~ N(0, 1); image i has label y_i and features normalize(proto[y_i] + noise * N(0, 1)); the
classifier is normalize(proto + 0.1 * N(0, 1)), perturbed prototypes.  All float32.
  S   C = 37,   E = 71,  B = 300,  noise 3.0   single label; nothing a multiple of a tile or of 4
  M   C = 300,  E = 130, B = 600,  noise 4.0   multi-label: rows 1 mod 3 carry a second label, rows 2 mod 3 a second and a third,
                                               the others -1 padding; three class tiles, five row tiles
  L   C = 1000, E = 96,  B = 1000, noise 3.5   single label; the class count of ImageNet

Margin rule: dev = the largest |chain_fp32 - fp64 logit| of the case; every image with a class that is not one of its labels
inside 64 * dev of its target logit t_i (the largest logit among its labels), or whose two largest logits are closer than that,
is redrawn with fresh noise (`redraws` says how often, so the inputs are a pure function of the stored seeds and counts) until
none is left, dev being measured again on every round.  With nothing inside the margin an implementation whose logits are within
float32 noise of the exact ones must reproduce every gt and every pred, and every eq is 0: nothing is left out of the
comparison.  The noise level of a case keeps its fp64 top-1 accuracy away from 0 and 1: a saturated case would show nothing.

Class-mean case W: C = 37 classes of 1 to 9 unit-norm prompt rows, E = 199; dev_w = the largest |class_mean_fp32 - class_mean_fp64|
over eps in {0, 1e-8}, the yardstick of the kernel's general test.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests import zeroshot_cases as Z      # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "zeroshot.npz")
MARGIN_FACTOR = 64
TOPK = (1, 5)
CASES = {"S": dict(c=37, e=71, b=300, noise=3.0, seed=8101, multi=False),
         "M": dict(c=300, e=130, b=600, noise=4.0, seed=8102, multi=True),
         "L": dict(c=1000, e=96, b=1000, noise=3.5, seed=8103, multi=False)}
ACC_RANGE = (0.1, 0.9)
CLASSMEAN = dict(c=37, e=199, seed=8201)


def _normalize(x):
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def case_labels(name):
    """-> int64 [B] (single label) or [B, 3] padded with -1."""
    k = CASES[name]
    y = np.random.RandomState(k["seed"] + 2).randint(0, k["c"], size=k["b"]).astype(np.int64)
    if not k["multi"]:
        return y
    extra = np.random.RandomState(k["seed"] + 4).randint(1, k["c"], size=(k["b"], 2))
    lab = np.stack([y, (y + extra[:, 0]) % k["c"], (y + extra[:, 1]) % k["c"]], axis=1)      # the extras differ from y
    rows = np.arange(k["b"])
    lab[rows % 3 == 0, 1:] = -1
    lab[rows % 3 == 1, 2] = -1
    return lab


def case_inputs(name, redraws):
    """-> image features fp32 [B, E], classifier fp32 [C, E], labels int64 [B] or [B, 3]."""
    k = CASES[name]
    c, e, seed = k["c"], k["e"], k["seed"]
    proto = np.random.RandomState(seed + 1).standard_normal((c, e))
    w = _normalize(proto + 0.1 * np.random.RandomState(seed + 3).standard_normal((c, e)))
    lab = case_labels(name)
    y = lab if lab.ndim == 1 else lab[:, 0]
    f = np.stack([_normalize(proto[y[i]] + k["noise"] * np.random.RandomState([seed, 1, i, int(redraws[i])]).standard_normal(e))
                  for i in range(k["b"])])
    return f.astype(np.float32), w.astype(np.float32), lab


def measure(name, redraws):
    f, w, lab = case_inputs(name, redraws)
    v = Z.logits_fp64(f, w)
    dev = float(np.abs(Z.chain_fp32(f, w).astype(np.float64) - v).max())
    gt, eq, pred = Z.ranks_from_logits(v, lab)
    mask = Z.label_mask(lab, v.shape[1])
    t = np.where(mask, v, -np.inf).max(axis=1)
    near = np.where(mask, np.inf, np.abs(v - t[:, None])).min(axis=1)      # the closest class that is not a label
    top2 = np.sort(v, axis=1)[:, -2:]
    return dict(dev=dev, gt=gt, eq=eq, pred=pred, gap=np.minimum(near, top2[:, 1] - top2[:, 0]), labels=lab)


def solve_redraws(name):
    redraws = np.zeros(CASES[name]["b"], dtype=np.int64)
    for rounds in range(60):
        m = measure(name, redraws)
        bad = m["gap"] < MARGIN_FACTOR * m["dev"]
        if not bad.any():
            return redraws, m, rounds
        redraws[bad] += 1
    raise RuntimeError(f"case {name}: rows inside the margin remain")


def classmean_inputs():
    """-> prompt embeddings fp32 [N, E] (unit-norm rows, sorted by class), offsets int64 [C + 1]."""
    k = CLASSMEAN
    rng = np.random.RandomState(k["seed"])
    counts = rng.randint(1, 10, size=k["c"])
    proto = rng.standard_normal((k["c"], k["e"]))
    emb = _normalize(np.repeat(proto, counts, axis=0) + 0.7 * rng.standard_normal((int(counts.sum()), k["e"])))
    return emb.astype(np.float32), np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def generate():
    arrays = {}
    for name, k in CASES.items():
        redraws, m, rounds = solve_redraws(name)
        counts = Z.counts_from_ranks(m["gt"], m["eq"], k["c"], TOPK)
        acc = {kk: counts[f"hits{kk}"] / k["b"] for kk in TOPK}
        if not ACC_RANGE[0] <= acc[1] <= ACC_RANGE[1]:
            raise RuntimeError(f"case {name}: fp64 top-1 accuracy {acc[1]} outside {ACC_RANGE}: choose another noise level")
        assert (m["eq"] == 0).all()
        arrays.update({f"{name}_c": np.int64(k["c"]), f"{name}_e": np.int64(k["e"]), f"{name}_b": np.int64(k["b"]),
                       f"{name}_seed": np.int64(k["seed"]), f"{name}_noise": np.float64(k["noise"]),
                       f"{name}_redraws": redraws.astype(np.int8), f"{name}_dev": np.float64(m["dev"]),
                       f"{name}_margin": np.float64(MARGIN_FACTOR * m["dev"]), f"{name}_gap": m["gap"].astype(np.float64),
                       f"{name}_labels": m["labels"].astype(np.int32), f"{name}_gt": m["gt"].astype(np.int32),
                       f"{name}_eq": m["eq"].astype(np.int32), f"{name}_pred": m["pred"].astype(np.int32),
                       f"{name}_count": np.int64(counts["count"]), f"{name}_ties": np.int64(counts["ties"])})
        arrays.update({f"{name}_hits{kk}": np.int64(counts[f"hits{kk}"]) for kk in TOPK})
        arrays.update({f"{name}_top{kk}": np.float64(acc[kk]) for kk in TOPK})
        print(name, "C", k["c"], "E", k["e"], "B", k["b"], "dev", f"{m['dev']:.3g}", "margin", f"{MARGIN_FACTOR * m['dev']:.3g}",
              "smallest gap", f"{m['gap'].min():.3g}", "rounds", rounds, "redrawn rows", int((redraws > 0).sum()), "top-1", acc[1],
              "top-5", acc[5])
    emb, offsets = classmean_inputs()
    dev_w = max(float(np.abs(Z.class_mean_fp32(emb, offsets, eps).astype(np.float64) - Z.class_mean_fp64(emb, offsets, eps)).max())
                for eps in (0.0, 1e-8))
    arrays.update({"W_c": np.int64(CLASSMEAN["c"]), "W_e": np.int64(CLASSMEAN["e"]), "W_seed": np.int64(CLASSMEAN["seed"]),
                   "W_offsets": offsets, "W_dev": np.float64(dev_w)})
    print("W", "rows", len(emb), "dev_w", f"{dev_w:.3g}")
    return arrays


def main():
    arrays = generate()
    np.savez_compressed(OUT, **arrays)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
