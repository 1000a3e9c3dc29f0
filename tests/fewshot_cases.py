"""Host restatements of the few-shot linear probe (the reference's clipa_jax/evaluators/fewshot_lsr.py), shared by
tools/make_fewshot_golden.py and the fewshot tests.  jax and big_vision are not installable next to this project, so the
reference's functions cannot be imported; the two functions below are written from its formulas:

  whitening   mean = x.mean(0); std = sqrt(mean((x - mean)^2, 0)) + 1e-5; z = (x - mean) / std, one more column holding 100.0
              (test rows use the train statistics);
  targets     Y = +1 at the label, -1 elsewhere;
  weights     w = (z^T z + l2 I)^-1 z^T Y, by eigh(z^T z) when N >= dim (route A) and as z^T (z z^T + l2 I)^-1 Y by
              eigh(z z^T) when N < dim (route B);
  prediction  argmax(z_test @ w, axis=1), the lowest index among equal maxima.

`lsr_fp64` solves the normal equations directly in float64 (no eigendecomposition, no route): the ground truth.  `lsr_fp32`
follows the reference's operation order and routes in float32 and stands in for its arithmetic; the difference between
the two is the yardstick `dev` of the golden file.
"""
import numpy as np

BIAS_CONSTANT = 100.0


def targets(y, num_classes, dtype):
    t = -np.ones((len(y), num_classes), dtype=dtype)
    t[np.arange(len(y)), y] = 1
    return t


def lsr_fp64(x, y, x_test, num_classes, l2):
    """-> float64 logits [Nt, C] of the exact ridge solution on fp32 inputs."""
    x, x_test = np.asarray(x, dtype=np.float64), np.asarray(x_test, dtype=np.float64)
    mean = x.mean(0)
    std = np.sqrt(((x - mean) ** 2).mean(0)) + 1e-5
    pad = lambda a: np.concatenate([(a - mean) / std, np.full((len(a), 1), BIAS_CONSTANT)], axis=1)      # noqa: E731
    z, zt = pad(x), pad(x_test)
    w = np.linalg.solve(z.T @ z + l2 * np.eye(z.shape[1]), z.T @ targets(y, num_classes, np.float64))
    return zt @ w


def lsr_fp32(x, y, x_test, num_classes, l2):
    """-> (float32 logits [Nt, C], route): every step in float32, in the reference's order."""
    f = np.float32
    x, x_test = np.asarray(x, dtype=f), np.asarray(x_test, dtype=f)
    mean = x.mean(0, keepdims=True, dtype=f)
    std = np.sqrt(np.mean(np.abs(x - mean) ** 2, axis=0, keepdims=True, dtype=f)) + f(1e-5)
    z = np.pad((x - mean) / std, ((0, 0), (0, 1)), constant_values=f(BIAS_CONSTANT))
    t = targets(y, num_classes, f)
    n, dim = z.shape
    if n >= dim:
        eigs, q = np.linalg.eigh(z.T @ z)
        rhs, lhs, route = q.T @ (z.T @ t), q, "A"
    else:
        eigs, q = np.linalg.eigh(z @ z.T)
        rhs, lhs, route = q.T @ t, z.T @ q, "B"
    scaling = (f(1.0) / (eigs + f(l2) * np.ones_like(eigs))).reshape(1, -1)
    w = (lhs * scaling) @ rhs
    zt = np.pad((x_test - mean) / std, ((0, 0), (0, 1)), constant_values=f(BIAS_CONSTANT))
    logits = zt @ w
    assert logits.dtype == f and w.dtype == f
    return logits, route


def subsets(labels, num_classes, seed, shots):
    """The reference's task sampling, restated: {shots: (indices, labels)} in class order."""
    labels = np.asarray(labels)
    rng = np.random.default_rng(seed)
    per_class = [rng.permutation(np.where(labels == c)[0]) for c in range(num_classes)]
    out = {}
    for k in shots:
        idx = np.concatenate([p[:k] for p in per_class], axis=0)
        out[k] = (idx, labels[idx])
    return out
