"""Generate tests/golden/fewshot_lsr.npz: synthetic few-shot linear-probe tasks with well-defined per-row predictions.

The reference's evaluator (clipa_jax/evaluators/fewshot_lsr.py) needs jax and big_vision, so the expected values come from
the two host restatements of tests/fewshot_cases.py: `lsr_fp64` (the exact ridge solution) gives the predictions,
`lsr_fp32` (the reference's operation order in float32) the size of float32 noise.  Run (numpy only):
    python tools/make_fewshot_golden.py
The tests read the .npz and regenerate the features with `case_inputs`; they never need anything else.

Cases (Nt = 1000 each): class prototypes plus noise, train rows in class order.
  A1  C = 20, D = 96, 10 shots, l2 = 1024   route A (N = 200 >= dim = 97)
  A2  the same task with l2 = 1
  B1  C = 20, D = 96, 2 shots, l2 = 1024    route B (N = 40)
  B2  C = 37, D = 199, 3 shots, l2 = 16     route B, nothing a multiple of a tile (N = 111, dim = 200)
  E   C = 20, D = 59, 3 shots, l2 = 64      N = 60 == dim: route A at the boundary

Margin rule: dev = the largest |lsr_fp32 logit - lsr_fp64 logit| of the case; every test row whose fp64 top-1 / top-2 gap is
below 64 * dev is redrawn with fresh noise (`redraws` says how often, so the features are a pure function of the stored
seeds and counts) until none is left, dev being measured again on every round.  With no row inside the margin an
implementation whose logits are within float32 noise of the exact ones must reproduce every prediction.  The noise level of
a case is chosen so that its fp64 accuracy lies in [0.5, 0.97]: a saturated case would show nothing.
Stored per case: shapes, l2, seed, noise, redraws, dev, margin, the fp64 predictions, maxima and gaps, the test labels,
the count of correct rows and the accuracy, and the route of the float32 stand-in.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests import fewshot_cases as F      # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "fewshot_lsr.npz")
NT = 1000
MARGIN_FACTOR = 64
CASES = {"A1": dict(c=20, d=96, shots=10, l2=1024.0, noise=2.0, seed=7101),
         "A2": dict(c=20, d=96, shots=10, l2=1.0, noise=2.0, seed=7101),
         "B1": dict(c=20, d=96, shots=2, l2=1024.0, noise=2.0, seed=7103),
         "B2": dict(c=37, d=199, shots=3, l2=16.0, noise=2.0, seed=7104),
         "E": dict(c=20, d=59, shots=3, l2=64.0, noise=2.0, seed=7105)}
ACC_RANGE = (0.5, 0.97)


def case_inputs(name, redraws):
    """-> x_train fp32 [C * shots, D] (class order), y_train int64, x_test fp32 [NT, D], y_test int64."""
    k = CASES[name]
    c, d, seed = k["c"], k["d"], k["seed"]
    proto = np.random.RandomState(seed + 1).standard_normal((c, d))
    y = np.repeat(np.arange(c), k["shots"])
    yt = np.random.RandomState(seed + 2).randint(0, c, size=NT)
    x = np.stack([proto[y[i]] + k["noise"] * np.random.RandomState([seed, 0, i, 0]).standard_normal(d) for i in range(len(y))])
    xt = np.stack([proto[yt[t]] + k["noise"] * np.random.RandomState([seed, 1, t, int(redraws[t])]).standard_normal(d)
                   for t in range(NT)])
    return x.astype(np.float32), y.astype(np.int64), xt.astype(np.float32), yt.astype(np.int64)


def measure(name, redraws):
    """-> dict(dev, pred, best, gap, route, y_test) of the case as it stands."""
    k = CASES[name]
    x, y, xt, yt = case_inputs(name, redraws)
    l64 = F.lsr_fp64(x, y, xt, k["c"], k["l2"])
    l32, route = F.lsr_fp32(x, y, xt, k["c"], k["l2"])
    top2 = np.sort(l64, axis=1)[:, -2:]
    return dict(dev=float(np.abs(l32.astype(np.float64) - l64).max()), pred=np.argmax(l64, axis=1), best=top2[:, 1],
                gap=top2[:, 1] - top2[:, 0], route=route, y_test=yt)


def solve_redraws(name):
    redraws = np.zeros(NT, dtype=np.int64)
    for _ in range(60):
        m = measure(name, redraws)
        bad = m["gap"] < MARGIN_FACTOR * m["dev"]
        if not bad.any():
            return redraws, m
        redraws[bad] += 1
    raise RuntimeError(f"case {name}: rows inside the margin remain")


def generate():
    arrays = {}
    for name, k in CASES.items():
        redraws, m = solve_redraws(name)
        correct = int((m["pred"] == m["y_test"]).sum())
        acc = correct / NT
        if not ACC_RANGE[0] <= acc <= ACC_RANGE[1]:
            raise RuntimeError(f"case {name}: fp64 accuracy {acc} outside {ACC_RANGE}: choose another noise level")
        n, dim = k["c"] * k["shots"], k["d"] + 1
        assert m["route"] == ("A" if n >= dim else "B")
        arrays.update({f"{name}_c": np.int64(k["c"]), f"{name}_d": np.int64(k["d"]), f"{name}_shots": np.int64(k["shots"]),
                       f"{name}_l2": np.float64(k["l2"]), f"{name}_seed": np.int64(k["seed"]), f"{name}_noise": np.float64(k["noise"]),
                       f"{name}_redraws": redraws.astype(np.int8), f"{name}_dev": np.float64(m["dev"]),
                       f"{name}_margin": np.float64(MARGIN_FACTOR * m["dev"]), f"{name}_pred": m["pred"].astype(np.int32),
                       f"{name}_best": m["best"].astype(np.float64), f"{name}_gap": m["gap"].astype(np.float64),
                       f"{name}_y_test": m["y_test"].astype(np.int32), f"{name}_correct": np.int64(correct),
                       f"{name}_accuracy": np.float64(acc), f"{name}_route": np.str_(m["route"])})
        print(name, "N", n, "dim", dim, "route", m["route"], "dev", f"{m['dev']:.3g}", "margin", f"{MARGIN_FACTOR * m['dev']:.3g}",
              "smallest gap", f"{m['gap'].min():.3g}", "redrawn rows", int((redraws > 0).sum()), "accuracy", acc)
    return arrays


def main():
    arrays = generate()
    np.savez_compressed(OUT, **arrays)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
