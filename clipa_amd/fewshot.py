"""Few-shot linear-probe evaluation through the MI355X engine: the reference's `clipa_jax/evaluators/fewshot_lsr.py`
(big_vision's closed-form L2-regularised least-squares classifier on frozen image features, at several shot counts and seeds).

The reference copies every representation to the host and runs the regression on its CPU backend.  Here the representations
stay on the GPU: the whitening statistics, the whitened (and transposed) copy, the Gram matrix z^T z (route A, N >= dim) or
z z^T (route B), z^T y and the argmax of z_test @ w are HIP kernels (`ops.fewshot_*`, csrc/fewshot.hip), all fp32 as the
reference.  Only the [dim, dim] (or [N, N]) Gram matrix and z^T y travel to the host - on route B, where N < dim, the N
whitened rows too - and the ridge system is solved there in numpy fp64, the one step the reference also keeps on the CPU.
The [Nt, C] logits are never formed.
"""
import numpy as np
import torch

from . import ops
from ._eval_common import _features


def class_indices(labels, num_classes, seed):
    """The reference's task sampling (compute_fewshot_metrics, fewshot_lsr.py:206-208): one generator per seed, a permutation
    of each class's example indices in class order.  labels: host array or tensor.  -> list of num_classes int64 arrays."""
    labels = np.asarray(labels.cpu() if torch.is_tensor(labels) else labels)
    rng = np.random.default_rng(seed)
    return [rng.permutation(np.where(labels == c)[0]) for c in range(num_classes)]


def _labels(y, n, num_classes, name, who):
    y = np.asarray(y.cpu() if torch.is_tensor(y) else y)
    if y.ndim != 1 or y.shape[0] != n or y.dtype.kind not in "iu":
        raise RuntimeError(f"clipa_amd.{who}: {name} must hold one integer label per row ({n}); got {y.dtype} {y.shape}")
    y = y.astype(np.int64)
    if n and (y.min() < 0 or y.max() >= num_classes):
        raise RuntimeError(f"clipa_amd.{who}: {name} values must lie in [0, {num_classes}); got [{y.min()}, {y.max()}]")
    return y


def _ridge(S, rhs, l2_reg):
    """(S + l2 I)^-1 rhs in fp64."""
    S = S.astype(np.float64)
    S[np.diag_indices_from(S)] += float(l2_reg)
    return np.linalg.solve(S, rhs.astype(np.float64))


def route(n, dim):
    """The reference's switch (fewshot_lsr.py:72): "A" (eigh of z^T z) when num_points >= dim, N == dim included, else "B"."""
    return "A" if n >= dim else "B"


def _task(x, index, counts, x_test, y_test, l2_reg):
    """One regression task on rows `index` (host int array of valid rows | None) of x, already in class order with counts[c]
    rows of class c.  -> (correct, route, pred, best)."""
    if index is not None:                          # built on the host from the labels' own positions: nothing to validate
        index = torch.from_numpy(np.ascontiguousarray(index, dtype=np.int32)).to(x.device)
    mean, std = ops.fewshot_moments(x, index, validate=False)
    n, dim, C = int(counts.sum()), x.shape[1] + 1, len(counts)
    offsets = np.concatenate([[0], np.cumsum(counts)])
    which = route(n, dim)
    if which == "A":                               # (z^T z + l2 I)^-1 z^T y
        z, zt = ops.fewshot_whiten(x, mean, std, index, transpose=True, validate=False)
        S, R = ops.fewshot_gram(zt), ops.fewshot_class_sums(z, offsets)
        w = _ridge(S.cpu().numpy(), R.cpu().numpy(), l2_reg)
    else:                                          # z^T (z z^T + l2 I)^-1 y
        z = ops.fewshot_whiten(x, mean, std, index, validate=False)
        S = ops.fewshot_gram(z)
        y = -np.ones((n, C))
        y[np.arange(n), np.repeat(np.arange(C), counts)] = 1.0
        w = z.cpu().numpy().astype(np.float64).T @ _ridge(S.cpu().numpy(), y, l2_reg)
    wt = torch.from_numpy(np.ascontiguousarray(w.T).astype(np.float32)).to(x.device)      # class-major [C, dim]
    pred, best = ops.fewshot_predict(ops.fewshot_whiten(x_test, mean, std), wt)
    return int((pred == y_test).sum()), which, pred, best


def _check_problem(x_train, x_test, num_classes, l2_reg, who):
    feats = []
    for name, t in (("x_train", x_train), ("x_test", x_test)):
        t = _features(t, name, who, check_finite=True)
        if t.shape[0] < 1 or t.shape[1] < 1:
            raise RuntimeError(f"clipa_amd.{who}: {name} is empty: shape {tuple(t.shape)}")
        if t.data_ptr() % 16:                      # a misaligned view: one dense copy here instead of one per kernel
            t = t.clone(memory_format=torch.contiguous_format)
        feats.append(t)
    x_train, x_test = feats
    if x_train.shape[1] != x_test.shape[1]:
        raise RuntimeError(f"clipa_amd.{who}: feature widths differ: {x_train.shape[1]} vs {x_test.shape[1]}")
    if int(num_classes) < 1 or not float(l2_reg) > 0.0:
        raise RuntimeError(f"clipa_amd.{who}: num_classes = {num_classes} must be >= 1 and l2_reg = {l2_reg} > 0")
    return x_train, x_test


def fewshot_lsr(x_train, y_train, x_test, y_test, num_classes, l2_reg, return_predictions=False):
    """`_precompute_cache` + `_eig_fewshot_acc_fn` of fewshot_lsr.py for one task: train features [N, D] with labels in
    [0, num_classes), test features [Nt, D] with labels (2-D GPU tensors of any float dtype, used as fp32; labels host or
    device integers).  -> {"accuracy": np.float64, "correct": int, "num_test": int, "route": "A" | "B"}; route A
    (N >= D + 1) solves with z^T z, route B with z z^T, as the reference.  Rows not already grouped by class are taken in
    stable class order.  return_predictions adds "pred" (int32 [Nt]) and "best" (the winning logit, f32 [Nt]), GPU tensors.
    CPU features, non-finite features, labels out of range and empty sets raise: there is no host fallback."""
    who = "fewshot_lsr"
    x_train, x_test = _check_problem(x_train, x_test, num_classes, l2_reg, who)
    y = _labels(y_train, x_train.shape[0], num_classes, "y_train", who)
    yt = _labels(y_test, x_test.shape[0], num_classes, "y_test", who)
    order = np.argsort(y, kind="stable")
    index = None if np.array_equal(order, np.arange(len(y))) else order
    counts = np.bincount(y, minlength=num_classes)
    correct, which, pred, best = _task(x_train, index, counts, x_test, torch.from_numpy(yt).to(x_test.device), l2_reg)
    out = {"accuracy": np.float64(correct) / np.float64(len(yt)), "correct": correct, "num_test": len(yt), "route": which}
    if return_predictions:
        out.update(pred=pred, best=best)
    return out


def fewshot_metrics(repr_train, labels_train, repr_test, labels_test, num_classes, shots, l2_reg, seed):
    """`compute_fewshot_metrics` of fewshot_lsr.py:205-223 on representations that stay on the GPU: per entry of `shots` the
    first `shots` indices of every class's seeded permutation (a class with fewer examples gives what it has), gathered on the
    device by index list, the test rows whitened anew with each subset's statistics.  -> {shots: np.float64 accuracy}."""
    who = "fewshot_metrics"
    repr_train, repr_test = _check_problem(repr_train, repr_test, num_classes, l2_reg, who)
    y = _labels(labels_train, repr_train.shape[0], num_classes, "labels_train", who)
    yt = _labels(labels_test, repr_test.shape[0], num_classes, "labels_test", who)
    yt_dev = torch.from_numpy(yt).to(repr_test.device)
    per_class = class_indices(y, num_classes, seed)
    results = {}
    for k in shots:
        picked = [idx[:k] for idx in per_class]
        index = np.concatenate(picked)
        counts = np.array([len(p) for p in picked], dtype=np.int64)
        correct, _, _, _ = _task(repr_train, index, counts, repr_test, yt_dev, l2_reg)
        results[k] = np.float64(correct) / np.float64(len(yt))
    return results


def _represent(model, batches, normalize, who):
    feats, labels = [], []
    for images, y in batches:
        feats.append(model.encode_image(images, normalize=normalize).float())
        labels.append(torch.as_tensor(y).reshape(-1).cpu())
    if not feats:
        raise RuntimeError(f"clipa_amd.{who}: a dataset yielded no batches")
    return torch.cat(feats), torch.cat(labels).numpy()


def evaluate_fewshot(model, datasets, shots=(1, 5, 10, 25), l2_reg=2.0 ** 10, num_seeds=3, representation="features",
                     display_first=()):
    """`Evaluator.run` of fewshot_lsr.py:225-234 on one process.  datasets: {name: (train_batches, test_batches,
    num_classes)}, the batches yielding (images, labels) with the images already on the device in the form
    `model.encode_image` accepts.  Every dataset is encoded once (no_grad, eval mode - the model's previous mode is put
    back after each dataset's encoding; representation "features": encode_image(normalize=False), "normalized":
    normalize=True).  As the reference's `_repr` cache, every dataset's representations stay on the GPU until the last seed
    has run (fp32, (N_train + N_test) x embed_dim per dataset); the generator releases them when it ends.  Yields (name, value) in the reference's order - seeds, then datasets, then shots - under its names:
    "{a/ if (name, shots) in display_first else z/}{name}_{shots}shot-seed-{seed}"."""
    who = "evaluate_fewshot"
    if representation not in ("features", "normalized"):
        raise RuntimeError(f"clipa_amd.{who}: representation must be 'features' or 'normalized', got {representation!r}")
    cache = {}
    for seed in range(num_seeds):
        for name, (train_batches, test_batches, num_classes) in datasets.items():
            if name not in cache:
                was_training = model.training
                model.eval()
                try:
                    with torch.no_grad():
                        cache[name] = (_represent(model, train_batches, representation == "normalized", who) +
                                       _represent(model, test_batches, representation == "normalized", who))
                finally:
                    model.train(was_training)
            xtr, ytr, xte, yte = cache[name]
            for k, v in fewshot_metrics(xtr, ytr, xte, yte, num_classes, shots, l2_reg, seed).items():
                prefix = "a/" if (name, k) in display_first else "z/"
                yield f"{prefix}{name}_{k}shot-seed-{seed}", v
