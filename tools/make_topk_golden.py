"""Generate tests/golden/topk.npz: seeded cases for the end-to-end tests of top-k similarity search (clipa_amd/search.py).

The expected lists come from the host restatements of tests/topk_cases.py on float64 products of the float32 inputs;
`chain_fp32` (the engine's ascending-k float32 chain) gives the size of float32 noise.  Run (numpy only):
    python tools/make_topk_golden.py
The tests read the .npz and regenerate the inputs with `case_inputs`; they never need anything else.

Cases (all float32, unit-norm rows; prototypes proto [C, E] ~ N(0, 1), a row of class y is normalize(proto[y] + noise * N(0, 1))):
  classify   B = 200 images against a classifier of C = 300 classes (three gallery tiles), E = 71, k = 5
  retrieve   Ni = 150 images and Nt = 260 texts of 40 topics, E = 64, k = 10, both directions
  knn        N = 700 training rows of 10 classes (fed in shards of 300), Nt = 150 test rows, E = 48, k = 20, T = 0.07

Margin rule (that of the zero-shot fixture, for lists): dev = the largest |chain_fp32 - fp64| over the case.  A row is "inside"
when any two neighbours among its first k + 1 fp64-sorted values are closer than 64 * dev - then float32 noise may swap two
entries of its list, or the last entry with the first one left out.  For kNN a row is also inside when its two best class
scores s1 >= s2 satisfy s1 - s2 < 64 * (dev / T) * (s1 + s2): a value off by dev changes its vote exp(v / T) by the relative
amount dev / T, so the gap of two scores by at most (dev / T) * (s1 + s2).  Rows outside must come out exactly; at most 2 % of a
case's rows may be inside, and a case that does not meet that is drawn again with the next seed (`draw` says how often).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests import topk_cases as T      # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "topk.npz")
MARGIN_FACTOR = 64
INSIDE_CAP = 0.02
CASES = {"classify": dict(nq=200, ng=300, e=71, k=5, classes=300, noise=3.0, seed=9101),
         "retrieve": dict(nq=150, ng=260, e=64, k=10, classes=40, noise=1.5, seed=9102),
         "knn": dict(nq=150, ng=700, e=48, k=20, classes=10, noise=2.0, seed=9103, temperature=0.07, chunk_rows=300)}


def _normalize(x):
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def case_inputs(name, draw):
    """-> queries fp32 [Nq, E], gallery fp32 [Ng, E], query classes int64 [Nq], gallery classes int64 [Ng].  classify: the
    gallery is the classifier (perturbed prototypes, class j = row j); the other cases draw gallery rows like query rows."""
    c = CASES[name]
    rng = np.random.RandomState([c["seed"], int(draw)])
    proto = rng.standard_normal((c["classes"], c["e"]))
    yq = rng.randint(0, c["classes"], size=c["nq"]).astype(np.int64)
    q = _normalize(proto[yq] + c["noise"] * rng.standard_normal((c["nq"], c["e"])))
    if name == "classify":
        yg = np.arange(c["ng"], dtype=np.int64)
        g = _normalize(proto + 0.1 * rng.standard_normal(proto.shape))
    else:
        yg = rng.randint(0, c["classes"], size=c["ng"]).astype(np.int64)
        g = _normalize(proto[yg] + c["noise"] * rng.standard_normal((c["ng"], c["e"])))
    return q.astype(np.float32), g.astype(np.float32), yq, yg


def inside_rows(v64, k, dev):
    """bool [Nq]: two neighbours among the first k + 1 sorted values closer than 64 * dev."""
    top = -np.sort(-v64, axis=1)[:, :k + 1]
    return (top[:, :-1] - top[:, 1:]).min(axis=1) < MARGIN_FACTOR * dev if top.shape[1] > 1 else np.zeros(len(v64), dtype=bool)


def measure(name, draw):
    c = CASES[name]
    q, g, yq, yg = case_inputs(name, draw)
    v = T.logits_fp64(q, g)
    dev = float(np.abs(T.chain_fp32(q, g).astype(np.float64) - v).max())
    out = dict(dev=dev)
    val, idx = T.topk_reference(v, c["k"])
    out.update(val=val, idx=idx, inside=inside_rows(v, c["k"], dev))
    if name == "retrieve":
        val_t, idx_t = T.topk_reference(v.T, c["k"])
        out.update(val_t=val_t, idx_t=idx_t, inside_t=inside_rows(v.T, c["k"], dev))
    if name == "knn":
        pred, scores = T.knn_vote_reference(val, yg[idx], c["temperature"], c["classes"])
        s = -np.sort(-scores, axis=1)[:, :2]
        close = s[:, 0] - s[:, 1] < MARGIN_FACTOR * (dev / c["temperature"]) * (s[:, 0] + s[:, 1])
        out.update(pred=pred, inside_vote=out["inside"] | close, top1=float((pred == yq).mean()))
    return out


def fractions(m):
    return [float(m[key].mean()) for key in ("inside", "inside_t", "inside_vote") if key in m]


def solve(name):
    for draw in range(20):
        m = measure(name, draw)
        if max(fractions(m)) <= INSIDE_CAP:
            return draw, m
    raise RuntimeError(f"case {name}: no draw keeps the rows inside the margin below {INSIDE_CAP}")


def generate():
    arrays = {}
    for name, c in CASES.items():
        draw, m = solve(name)
        arrays.update({f"{name}_{key}": np.int64(c[key]) for key in ("nq", "ng", "e", "k", "classes", "seed")})
        arrays.update({f"{name}_draw": np.int64(draw), f"{name}_dev": np.float64(m["dev"])})
        for key in ("idx", "idx_t"):
            if key in m:
                arrays[f"{name}_{key}"] = m[key].astype(np.int32)
        for key in ("inside", "inside_t", "inside_vote"):
            if key in m:
                arrays[f"{name}_{key}"] = m[key]
        if name == "knn":
            arrays.update({"knn_pred": m["pred"].astype(np.int32), "knn_top1": np.float64(m["top1"])})
        print(name, "draw", draw, "dev", f"{m['dev']:.3g}", "inside", fractions(m), "top1" if name == "knn" else "", m.get("top1", ""))
    return arrays


def main():
    arrays = generate()
    np.savez_compressed(OUT, **arrays)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
