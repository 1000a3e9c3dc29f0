"""Host restatements of zero-shot classification, shared by tools/make_zeroshot_golden.py and the zeroshot tests.

  ranks_from_logits / ranks_fp64   what csrc/zeroshot.hip computes per image, from a [B, C] logit matrix (float64 products of the
                                   fp32 inputs: the ground truth; or exact integers)
  chain_fp32                       the engine's arithmetic restated: one ascending-k chain of fused multiply-adds per logit
  class_mean_fp64 / class_mean_fp32  the prompt-ensemble classifier, exactly and in the kernel's documented float32 order
  accuracy_torch_reference         clipa_torch/training/zero_shot.py:47-50 (`accuracy`: topk, then compare with the target)
  any_match_jax_reference          clipa_jax/evaluators/proj/image_text/discriminative_classifier.py:303-312 (argmax, then "any
                                   label matches")
"""
import numpy as np

CM_THREADS = 256                              # csrc/zeroshot.hip: columns d, d + 256, ... belong to one thread's partial sum


def label_mask(labels, num_classes):
    """labels [B] or [B, Lmax] with -1 = none -> bool [B, C].  As in the kernel, a value outside [0, C) names no class."""
    lab = np.asarray(labels)
    lab = lab[:, None] if lab.ndim == 1 else lab
    mask = np.zeros((len(lab), num_classes), dtype=bool)
    rows, cols = np.nonzero((lab >= 0) & (lab < num_classes))
    mask[rows, lab[rows, cols]] = True
    return mask


def ranks_from_logits(v, labels):
    """-> (gt, eq, pred) int64 [B]: classes above / equal to (labels excluded) the best label's logit; np.argmax (lowest index
    among equal maxima).  A row without labels: t = -inf, so gt = C and eq = 0."""
    v = np.asarray(v)
    mask = label_mask(labels, v.shape[1])
    t = np.where(mask, v.astype(np.float64), -np.inf).max(axis=1)[:, None]
    return (v > t).sum(1).astype(np.int64), ((v == t) & ~mask).sum(1).astype(np.int64), np.argmax(v, axis=1).astype(np.int64)


def logits_fp64(feat, w):
    return np.asarray(feat, dtype=np.float64) @ np.asarray(w, dtype=np.float64).T


def ranks_fp64(feat, w, labels):
    return ranks_from_logits(logits_fp64(feat, w), labels)


def chain_fp32(feat, w):
    """float32 [B, C]: acc = fma(a_k, b_k, acc) for k = 0, 1, ... (the product of two float32 is exact in float64; the sum is
    rounded to float64 and then to float32, which differs from a true fma only in rare double-rounding cases - good enough for
    the size of the error, which is all this is used for)."""
    a, b = np.asarray(feat, dtype=np.float32), np.asarray(w, dtype=np.float32)
    acc = np.zeros((a.shape[0], b.shape[0]), dtype=np.float32)
    for k in range(a.shape[1]):
        acc = (acc.astype(np.float64) + np.outer(a[:, k].astype(np.float64), b[:, k].astype(np.float64))).astype(np.float32)
    return acc


def counts_from_ranks(gt, eq, num_classes, topk):
    """The engine's counts, restated: a hit at k is gt < min(k, C)."""
    out = {"count": int(len(gt)), "ties": int((np.asarray(eq) > 0).sum())}
    out.update({f"hits{k}": int((np.asarray(gt) < min(k, num_classes)).sum()) for k in topk})
    return out


def class_mean_fp64(emb, offsets, eps):
    emb = np.asarray(emb, dtype=np.float64)
    m = np.stack([emb[a:b].mean(axis=0) for a, b in zip(offsets[:-1], offsets[1:])])
    return m / (eps + np.linalg.norm(m, axis=1, keepdims=True))


def class_mean_fp32(emb, offsets, eps):
    """Every step a float32 operation in the order csrc/zeroshot.hip documents: rows added in ascending order, one division by n,
    squares accumulated by fused multiply-add per thread (columns t, t + 256, ...) in ascending column order, the 256 partial
    sums added in ascending t, m / (eps + sqrt(ss))."""
    f = np.float32
    emb = np.asarray(emb, dtype=f)
    E = emb.shape[1]
    out = np.zeros((len(offsets) - 1, E), dtype=f)
    for c, (a, b) in enumerate(zip(offsets[:-1], offsets[1:])):
        s = np.zeros(E, dtype=f)
        for r in range(a, b):
            s = s + emb[r]
        m = s / f(b - a)
        q = np.zeros(CM_THREADS, dtype=f)
        for d0 in range(0, E, CM_THREADS):                  # q = fma(m, m, q): the product is exact in float64, see chain_fp32
            md = m[d0:d0 + CM_THREADS].astype(np.float64)
            q[:len(md)] = (q[:len(md)].astype(np.float64) + md * md).astype(f)
        ss = f(0)
        for t in range(CM_THREADS):
            ss = f(ss + q[t])
        out[c] = m / f(f(eps) + np.sqrt(ss))
    assert out.dtype == f
    return out


def accuracy_torch_reference(output, target, topk=(1,)):
    """zero_shot.py:47-50 on host tensors.  -> list of float counts."""
    import torch                              # only here: the golden tool needs numpy alone
    output, target = torch.as_tensor(output), torch.as_tensor(target)
    pred = output.topk(max(topk), 1, True, True)[1].t()
    correct = pred.eq(target.view(1, -1).expand_as(pred))
    return [float(correct[:k].reshape(-1).float().sum(0, keepdim=True).cpu().numpy()[0]) for k in topk]


def any_match_jax_reference(logits, labels, mask=None):
    """discriminative_classifier.py:303-312: best_txt = argmax; matching = (best_txt[:, None] == labels).sum(1); correct =
    where(mask, matching > 0, 0).sum().  labels [B, Lmax] padded with -1."""
    logits, labels = np.asarray(logits), np.asarray(labels)
    assert labels.ndim == 2, labels.shape
    best_txt = logits.argmax(axis=1)
    matching = (best_txt[:, None] == labels).sum(axis=1)
    mask = np.ones(len(labels), dtype=bool) if mask is None else np.asarray(mask)
    return int(np.where(mask, (matching > 0).astype(np.int32), 0).sum())
