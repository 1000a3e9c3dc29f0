"""Zero-shot classification through the MI355X engine.  Mirrors
clipa_torch/training/zero_shot.py:29-90 - `zero_shot_classifier` (per class: encode the prompt templates, L2-normalise,
average, re-normalise, stack into [E, C]) and `run` (encode images, normalise, logits = 100 * f @ classifier, top-1 /
top-5) - on pre-tokenised prompts: the tokenizer itself (open_clip/tokenizer.py) is host-side text processing outside
the hot path.  Every matrix product and normalisation below is a libclipa_hip.so launch (encode_text / encode_image
are the engine's towers, the class logits are one gemm_nt); only topk / eq bookkeeping is torch.

The second half of the file is the fused fp32 evaluator (csrc/zeroshot.hip): `build_classifier` encodes all prompts in large
chunks and averages them per class in one kernel (`class_mean_embeddings`; eps = 1e-8 gives `_average_embeddings` of
clipa_jax/evaluators/proj/image_text/discriminative_classifier.py:152-171), `zero_shot_ranks` ranks every image's best label
among the classes in fp32 without the [B, C] logits and with multi-label targets (ImageNet-ReaL, :303-312), and
`zero_shot_counts` / `zero_shot_metrics` / `evaluate_zero_shot` turn the ranks into additive counts and top-k accuracies.  A hit
at k means fewer than k classes beat the label: ties resolve in the label's favour, the rule of the validation ranks
(evaluate.py), where `torch.topk` leaves the order of equal logits unspecified."""
import numpy as np
import torch

from . import ops
from ._eval_common import _features, _inference, unwrap_model


@torch.no_grad()
def zero_shot_classifier(model, class_token_ids):
    """class_token_ids: int64 [C, T, ctx] (C classes x T prompt templates, tokenised) or a list of [T_c, ctx] tensors.
    -> bf16 classifier [C8, E] (class embeddings as rows, zero-padded to a multiple of 8 classes) and C."""
    m = unwrap_model(model)
    rows = []
    for toks in class_token_ids:
        emb = m.encode_text(toks, normalize=True)                       # [T, E] f32, L2-normalised (model.py:263)
        mean = emb.mean(dim=0, keepdim=True)
        rows.append(ops.l2norm_fwd(mean.contiguous())[0])               # class_embedding /= class_embedding.norm()
    w = torch.cat(rows, dim=0)                                          # [C, E]
    C = w.shape[0]
    C8 = (C + 7) // 8 * 8
    wb = torch.zeros((C8, w.shape[1]), device=w.device, dtype=torch.bfloat16)
    wb[:C] = ops.to_bf16(w)
    return wb, C


@torch.no_grad()
def zero_shot_logits(model, classifier, num_classes, images):
    """100 * normalize(encode_image(images)) @ classifier^T -> f32 [B, C].  images: uint8 / float [B,3,S,S] on the GPU."""
    f = unwrap_model(model).encode_image(images, normalize=True)
    return ops.gemm_nt(ops.to_bf16(f), classifier, alpha=100.0, out_f32=True)[:, :num_classes]


def accuracy(output, target, topk=(1,)):      # zero_shot.py:47-50
    pred = output.topk(max(topk), 1, True, True)[1].t()
    correct = pred.eq(target.view(1, -1).expand_as(pred))
    return [float(correct[:k].reshape(-1).float().sum()) for k in topk]


@torch.no_grad()
def run(model, classifier, num_classes, batches, topk=(1, 5)):
    """batches: iterable of (images, targets) already on the model's device -> accuracies for `topk`."""
    hits = [0.0] * len(topk)
    n = 0
    for images, target in batches:
        logits = zero_shot_logits(model, classifier, num_classes, images)
        for i, a in enumerate(accuracy(logits, target, topk=tuple(min(k, num_classes) for k in topk))):
            hits[i] += a
        n += images.shape[0]
    return [h / max(n, 1) for h in hits]


# ---- the fused fp32 evaluator (csrc/zeroshot.hip) --------------------------------------------------------------------------
MAX_LABELS = 32                               # labels per image the rank kernel takes (ZS_MAX_LABELS)


def _topk(topk, who):
    ks = tuple(topk)
    if not ks or any(not isinstance(k, (int, np.integer)) or isinstance(k, bool) or k < 1 for k in ks):
        raise RuntimeError(f"clipa_amd.{who}: topk must be a non-empty sequence of integers >= 1, got {topk!r}")
    return tuple(int(k) for k in ks)


def prompt_order(prompt_class, num_classes):
    """Host side of the prompt ensemble: prompt_class (host array or tensor, one class index per prompt, in any order; several
    names of one class - the aliases of `expand_aliases`, discriminative_classifier.py:87-92 - simply share its index) ->
    (order, offsets): the stable sort of the prompts by class (None when they are already sorted) and the C + 1 row bounds of
    the classes in that order.  A class index outside [0, num_classes) and a class without prompts raise."""
    who = "class_mean_embeddings"
    pc = np.asarray(prompt_class.cpu() if torch.is_tensor(prompt_class) else prompt_class)
    if pc.ndim != 1 or pc.dtype.kind not in "iu":
        raise RuntimeError(f"clipa_amd.{who}: prompt_class must hold one integer class per prompt; got {pc.dtype} {pc.shape}")
    C = int(num_classes)
    if C < 1:
        raise RuntimeError(f"clipa_amd.{who}: num_classes = {num_classes} must be >= 1")
    pc = pc.astype(np.int64)
    if len(pc) and (pc.min() < 0 or pc.max() >= C):
        raise RuntimeError(f"clipa_amd.{who}: prompt_class values must lie in [0, {C}); got [{pc.min()}, {pc.max()}]")
    counts = np.bincount(pc, minlength=C)
    missing = np.nonzero(counts == 0)[0]
    if len(missing):
        raise RuntimeError(f"clipa_amd.{who}: Classes without embeddings: {missing[:8].tolist()}{'...' if len(missing) > 8 else ''}")
    order = np.argsort(pc, kind="stable")
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return (None if np.array_equal(order, np.arange(len(pc))) else order), offsets


def class_mean_embeddings(emb, prompt_class, num_classes, eps=0.0):
    """emb [N, E] prompt embeddings (2-D float GPU tensor, used as fp32), prompt_class [N] -> fp32 [C, E] classifier, class c's
    row = m_c / (eps + ||m_c||) with m_c the mean of its prompts' rows (ops.zeroshot_class_mean).  eps = 0 on unit-norm rows is
    zero_shot.py:37-38, eps = 1e-8 `_average_embeddings(normalize=True)`.  Rows of the result are 16-byte aligned (a view of a
    buffer padded to a multiple of 4 columns), so the rank kernel reads it in place."""
    who = "class_mean_embeddings"
    emb = _features(emb, "emb", who)
    order, offsets = prompt_order(prompt_class, num_classes)
    if int(offsets[-1]) != emb.shape[0] or emb.shape[1] < 1:
        raise RuntimeError(f"clipa_amd.{who}: emb {tuple(emb.shape)} must hold one row of E >= 1 columns per entry of prompt_class "
                           f"({int(offsets[-1])})")
    if not bool(torch.isfinite(emb).all()):
        raise RuntimeError(f"clipa_amd.{who}: emb holds non-finite values")
    if order is not None:
        emb = emb.index_select(0, torch.from_numpy(order).to(emb.device))
    return ops.zeroshot_class_mean(emb, offsets.tolist(), eps)


def build_classifier(model, prompt_tokens, prompt_class, num_classes, *, text_batch_size=1024, eps=0.0):
    """The zero-shot classifier from ALL prompts at once: prompt_tokens int [N, ctx] on the device (every template of every
    class name, in any order), prompt_class [N] their class indices.  encode_text(normalize=True) runs on chunks of
    text_batch_size prompts - ceil(N / text_batch_size) tower runs instead of one per class (zero_shot.py:33-39) - under no_grad
    and in eval mode (the model's previous mode is put back); -> class_mean_embeddings of the result, fp32 [C, E]."""
    who = "build_classifier"
    if not torch.is_tensor(prompt_tokens) or not prompt_tokens.is_cuda or prompt_tokens.dim() != 2 or prompt_tokens.shape[0] < 1:
        raise RuntimeError(f"clipa_amd.{who}: prompt_tokens must be a [N >= 1, ctx] GPU tensor of token ids")
    bs = int(text_batch_size)
    if bs < 1:
        raise RuntimeError(f"clipa_amd.{who}: text_batch_size = {text_batch_size} must be >= 1")
    _, offsets = prompt_order(prompt_class, num_classes)                   # fail before the towers run
    if int(offsets[-1]) != prompt_tokens.shape[0]:
        raise RuntimeError(f"clipa_amd.{who}: {prompt_tokens.shape[0]} prompts but {int(offsets[-1])} class indices")
    with _inference(model) as m:
        emb = torch.cat([m.encode_text(prompt_tokens[i:i + bs], normalize=True).float()
                         for i in range(0, prompt_tokens.shape[0], bs)])
    return class_mean_embeddings(emb, prompt_class, num_classes, eps)


def _labels2d(labels, B, device, who):
    """-> integer [B, Lmax] tensor on `device` in its own dtype (the range check wants the unconverted values)."""
    if not torch.is_tensor(labels):
        labels = torch.as_tensor(np.asarray(labels))
    if labels.dtype.is_floating_point or labels.dtype.is_complex or labels.dtype == torch.bool:
        raise RuntimeError(f"clipa_amd.{who}: labels must be integers, got {labels.dtype}")
    if labels.dim() == 1:
        labels = labels[:, None]
    if labels.dim() != 2 or labels.shape[0] != B:
        raise RuntimeError(f"clipa_amd.{who}: labels must be [B] or [B, Lmax] with B = {B}; got {tuple(labels.shape)}")
    if not 1 <= labels.shape[1] <= MAX_LABELS:
        raise RuntimeError(f"clipa_amd.{who}: Lmax = {labels.shape[1]} labels per image; the kernel takes 1 to {MAX_LABELS}")
    return labels.to(device)


def _operands(image_features, classifier, who):
    f, w = _features(image_features, "image_features", who), _features(classifier, "classifier", who)
    if f.shape[1] != w.shape[1] or w.shape[0] < 1 or w.shape[1] < 1:
        raise RuntimeError(f"clipa_amd.{who}: image_features {tuple(f.shape)} and classifier {tuple(w.shape)} must be [B, E] and "
                           f"[C >= 1, E >= 1]")
    return f, w


def _ranks_and_stats(f, w, labels, ks):
    """One launch and its bookkeeping, all on the device: -> (gt, eq, pred, stats) with stats int64 [len(ks) + 4] = hits per k,
    rows with eq > 0, rows, labels outside [-1, C), non-finite feature rows.  No host sync."""
    C = w.shape[0]
    bad = ((labels < -1) | (labels >= C)).sum()
    nonfinite = (~torch.isfinite(f)).any(dim=1).sum() if f.shape[0] else bad * 0
    gt, eq, pred = ops.zeroshot_ranks(f, w, labels.to(torch.int32))
    stats = torch.stack([(gt < min(k, C)).sum() for k in ks] + [(eq > 0).sum(), bad * 0 + f.shape[0], bad, nonfinite])
    return gt, eq, pred, stats


def _raise_on_flags(stats, who, what="labels"):
    """stats: the host list of _ranks_and_stats (summed or not), its last entry the classifier's non-finite count added."""
    if stats[-3]:
        raise RuntimeError(f"clipa_amd.{who}: {stats[-3]} {what} values outside [-1, C) (-1 = no label)")
    if stats[-2] or stats[-1]:
        raise RuntimeError(f"clipa_amd.{who}: non-finite values in {stats[-2]} image feature rows / {stats[-1]} classifier entries")


def _counts(stats, ks):
    out = {"count": int(stats[len(ks) + 1]), "ties": int(stats[len(ks)])}
    out.update({f"hits{k}": int(h) for k, h in zip(ks, stats)})
    return out


def metrics_from_counts(counts, topk=(1, 5)):
    """Counts (of one call, or the sums over the shards of a dataset: they are additive) -> the counts plus
    {f"top{k}": np.float64 accuracy}.  No rows: the accuracies are NaN, the mean of nothing."""
    n = counts["count"]
    out = dict(counts)
    out.update({f"top{k}": np.float64(counts[f"hits{k}"]) / np.float64(n) if n else np.float64("nan") for k in _topk(topk, "metrics_from_counts")})
    return out


def _run_ranks(image_features, classifier, labels, ks, who):
    f, w = _operands(image_features, classifier, who)
    labels = _labels2d(labels, f.shape[0], f.device, who)
    gt, eq, pred, stats = _ranks_and_stats(f, w, labels, ks)
    stats = torch.cat([stats, (~torch.isfinite(w)).sum().reshape(1)]).tolist()       # the one host sync
    _raise_on_flags(stats, who)
    return gt, eq, pred, stats


def zero_shot_ranks(image_features, classifier, labels):
    """image_features [B, E], classifier [C, E] (2-D float GPU tensors, used as fp32; unit-norm rows in the evaluators), labels
    [B] or [B, Lmax <= 32] integers, -1 = no label (the padding of multi-label targets, discriminative_classifier.py:304).
    -> {"gt", "eq", "pred"}, int32 [B] on the device (ops.zeroshot_ranks): per image the classes whose fp32 dot product beats /
    ties (labels excluded) that of its best label, and the argmax class, the lowest index among equal maxima (jnp.argmax, :303).
    An image without labels has gt = C.  B == 0 gives empty tensors without a launch.  CPU tensors, non-finite values, labels
    outside [-1, C), mismatched widths and Lmax > 32 raise: there is no host fallback."""
    gt, eq, pred, _ = _run_ranks(image_features, classifier, labels, (), "zero_shot_ranks")
    return {"gt": gt, "eq": eq, "pred": pred}


def zero_shot_counts(image_features, classifier, labels, topk=(1, 5)):
    """-> {"count": rows, "ties": rows with eq > 0, f"hits{k}": rows with gt < min(k, C)}, Python ints.  A hit at k: fewer than k
    classes beat the image's best label (the label wins a tie; k above C is the reference's clipped k).  An image without labels
    is counted and never a hit, as the JAX evaluator counts it.  The counts are additive over the shards of a dataset."""
    who = "zero_shot_counts"
    ks = _topk(topk, who)
    return _counts(_run_ranks(image_features, classifier, labels, ks, who)[3], ks)


def zero_shot_metrics(image_features, classifier, labels, topk=(1, 5)):
    """zero_shot_counts plus {f"top{k}": np.float64 accuracy} (metrics_from_counts)."""
    return metrics_from_counts(zero_shot_counts(image_features, classifier, labels, topk), topk)


def evaluate_zero_shot(model, classifier, datasets, topk=(1, 5)):
    """`run` for every dataset (zero_shot.py:93-117): datasets = {name: batches}, batches yielding (images, labels) on the device
    (labels [b] or [b, Lmax], -1 = no label).  Per batch: encode_image(normalize=True), the rank kernel, the counts added on the
    device; one host sync per dataset.  no_grad and eval mode, the model's previous mode put back.
    -> {f"{name}-top{k}": np.float64, f"{name}-count": int}; with the name "imagenet-zeroshot-val" the keys of :108-109."""
    who = "evaluate_zero_shot"
    ks = _topk(topk, who)
    w = _features(classifier, "classifier", who)
    w_bad = (~torch.isfinite(w)).sum().reshape(1)
    results = {}
    with _inference(model) as m:
        for name, batches in datasets.items():
            total = None
            for images, labels in batches:
                f, _ = _operands(m.encode_image(images, normalize=True), w, who)
                stats = _ranks_and_stats(f, w, _labels2d(labels, f.shape[0], f.device, who), ks)[3]
                total = stats if total is None else total + stats
            if total is None:
                raise RuntimeError(f"clipa_amd.{who}: dataset {name!r} yielded no batches")
            total = torch.cat([total, w_bad]).tolist()                 # the dataset's one host sync
            _raise_on_flags(total, f"{who} ({name})")
            met = metrics_from_counts(_counts(total, ks), ks)
            results.update({f"{name}-top{k}": met[f"top{k}"] for k in ks})
            results[f"{name}-count"] = met["count"]
    return results
