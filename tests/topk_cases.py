"""Host restatements of top-k similarity search (csrc/topk.hip, clipa_amd/search.py) and the exact kernel-level cases, shared by
tools/make_topk_golden.py and the topk tests.

  first_k / topk_reference   the order, the whole definition of the result: (v, g) precedes (v', g') iff v > v', or v == v' and
                             g < g' (IEEE ==, so -0 and +0 tie; zeros are reported as +0); a NaN precedes every number, NaNs
                             among themselves by index; an index of -1 is an empty slot, after everything, reported as (-inf, -1)
  knn_vote_reference         the vote rule of knn_classify, entry by entry
  chain_fp32                 tests/zeroshot_cases.py: the engine's arithmetic, one ascending-k chain of fused multiply-adds

Kernel-level inputs are exactly representable - small integers, every partial sum far below 2^24 - so float32, float64 and any
summation order agree and every comparison is for equality over every row.
"""
import math

import numpy as np

from .zeroshot_cases import chain_fp32, logits_fp64      # noqa: F401  (re-exported)


def first_k(values, indices, k):
    """values [Nq, n] floats, indices [Nq, n] int64 (-1 = empty slot) -> (float32-or-float64 [Nq, k], int64 [Nq, k]): the first k
    of every row in the order; a stable descending sort (np.lexsort is stable and the index is the last key anyway)."""
    v = np.asarray(values)
    g = np.broadcast_to(np.asarray(indices, dtype=np.int64), v.shape)
    nq, n = v.shape
    out_v = np.full((nq, k), -np.inf, dtype=v.dtype if v.dtype.kind == "f" else np.float64)
    out_g = np.full((nq, k), -1, dtype=np.int64)
    for i in range(nq):
        real = g[i] >= 0
        vi, gi = v[i][real], g[i][real]
        nan = np.isnan(vi)
        with np.errstate(invalid="ignore"):
            order = np.lexsort((gi, -np.where(nan, 0, vi), ~nan))       # NaN first; then the larger value (-0 == +0); then the index
        order = order[:k]
        out_v[i, :len(order)] = vi[order] + 0.0                         # -0 + 0 = +0
        out_g[i, :len(order)] = gi[order]
    return out_v, out_g


def topk_reference(v, k, index_base=0):
    """v [Nq, Ng] -> the first k entries of every row, column j carrying the index index_base + j."""
    v = np.asarray(v)
    return first_k(v, index_base + np.arange(v.shape[1], dtype=np.int64)[None, :], k)


def knn_vote_reference(values, neighbour_labels, temperature, num_classes):
    """-> (pred int64 [Nt], scores float64 [Nt, C]): every neighbour votes exp(v / T) for its class, the votes of a row are added
    in list order in float64, the lowest class among the best scores wins; a label of -1 is no neighbour."""
    nt, k = np.asarray(values).shape
    scores = np.zeros((nt, num_classes), dtype=np.float64)
    for i in range(nt):
        for j in range(k):
            c = int(neighbour_labels[i][j])
            if c >= 0:
                scores[i, c] += math.exp(float(values[i][j]) / float(temperature))
    pred = np.array([min(c for c in range(num_classes) if scores[i, c] == scores[i].max()) for i in range(nt)], dtype=np.int64)
    return pred, scores


# ---- exact kernel-level inputs ---------------------------------------------------------------------------------------------
def integer_case(nq, ng, e, seed, lo=-3, hi=3):
    """Small integers: |q . g| <= 9 e, exact in every format; with so few distinct values every row is full of ties."""
    rng = np.random.RandomState(seed)
    return rng.randint(lo, hi + 1, size=(nq, e)).astype(np.float32), rng.randint(lo, hi + 1, size=(ng, e)).astype(np.float32)


def fraction_case(nq, ng, e, seed):
    """Multiples of 2^-6 in [-1, 1]: products are multiples of 2^-12 and every partial sum stays below e < 2^11, so 23 bits hold
    it exactly.  Many distinct values, few ties."""
    rng = np.random.RandomState(seed)
    return (rng.randint(-64, 65, size=(nq, e)) / 64.0).astype(np.float32), (rng.randint(-64, 65, size=(ng, e)) / 64.0).astype(np.float32)


def position_coded(nq, ng, e):
    """One-hot query rows (row i selects column i mod e) against G[j, d] = ((7 j + 3 d) mod 61) - 30: v_ij = G[j, i mod e], so
    every value names its (i, j)."""
    q = np.zeros((nq, e), dtype=np.float32)
    q[np.arange(nq), np.arange(nq) % e] = 1.0
    j, d = np.arange(ng)[:, None], np.arange(e)[None, :]
    return q, (((7 * j + 3 * d) % 61) - 30).astype(np.float32)


def exact_product(q, g, scale=None):
    """float64 q @ g^T of exactly representable inputs, times an exactly representable scale: what every format computes."""
    v = np.asarray(q, dtype=np.float64) @ np.asarray(g, dtype=np.float64).T
    return v if scale is None else float(scale) * v
