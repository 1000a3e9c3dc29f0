"""CLIP validation through the MI355X engine: the `should_val` branch of the reference's `evaluate`
(clipa_torch/training/train.py:317-430) and its `get_clip_metrics` (train.py:432-449).

The reference copies every validation feature to the host, builds the [N, N] fp32 logits on the CPU and argsorts every
row and every column.  Here the features stay on the GPU and one kernel pair (`ops.retrieval_ranks`,
csrc/retrieval.hip) counts, per row and per column, the entries that beat or tie the positive: O(N) memory, no logit
matrix anywhere.  Only the 2 N int32 ranks travel to the host, where `metrics_from_ranks` applies the reference's
formulas.

Tie rule (deliberately different from the reference): `torch.argsort(descending=True)` on the CPU is not stable, so among
exactly equal logits the reference's 0-based position of the positive is some value in [gt, gt + eq].  The engine reports
gt, the optimistic position - deterministic, and equal to the reference's whenever the positive has no exact tie.
"""
import numpy as np
import torch

from . import ops
from .loss import ClipLoss

DIRECTIONS = ("image_to_text", "text_to_image")


def metrics_from_ranks(i2t, t2i):
    """0-based ranks of the positives (array-likes [N]) -> the reference's 10 metrics (train.py:441-447), np.float64."""
    metrics = {}
    for name, preds in zip(DIRECTIONS, (i2t, t2i)):
        preds = np.asarray(preds.cpu() if torch.is_tensor(preds) else preds).astype(np.int64)
        metrics[f"{name}_mean_rank"] = preds.mean() + 1
        metrics[f"{name}_median_rank"] = np.floor(np.median(preds)) + 1
        for k in [1, 5, 10]:
            metrics[f"{name}_R@{k}"] = np.mean(preds < k)
    return metrics


def get_clip_metrics(image_features, text_features, logit_scale):
    """Drop-in for the reference's get_clip_metrics: image / text features [N, E] on the GPU (any float dtype; ranked
    in fp32), logit_scale a device tensor or a float.  CPU features raise: there is no host fallback."""
    for name, t in (("image_features", image_features), ("text_features", text_features)):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise RuntimeError(f"clipa_amd.get_clip_metrics: {name} must be a GPU tensor (no CPU fallback); got "
                               f"{t.device if torch.is_tensor(t) else type(t).__name__}")
    dev = image_features.device
    if torch.is_tensor(logit_scale):
        scale = logit_scale.detach().to(device=dev, dtype=torch.float32).reshape(-1)[:1]     # no .item(): stays on the device
    else:
        scale = torch.full((1,), float(logit_scale), device=dev, dtype=torch.float32)
    i2t_gt, _, t2i_gt, _ = ops.retrieval_ranks(image_features.detach().float(), text_features.detach().float(), scale)
    return metrics_from_ranks(i2t_gt, t2i_gt)


def _outputs(out):
    if isinstance(out, dict):
        return out["image_features"], out["text_features"], out["logit_scale"]
    return out[0], out[1], out[2]


def evaluate(model, batches, epoch=0):
    """The validation branch of train.py:317-430 on one rank (the reference evaluates on the master rank only).
    batches: iterable of (images, texts) already on the device, in the form the engine's forward accepts.  Returns
    {**get_clip_metrics(...), "clip_val_loss", "epoch", "num_samples"}; the metrics use the last batch's logit_scale, as
    the reference does."""
    model.eval()
    loss_fn = ClipLoss()
    cumulative_loss = None
    num_samples = 0
    all_image_features, all_text_features = [], []
    logit_scale = None
    with torch.no_grad():
        for images, texts in batches:
            image_features, text_features, logit_scale = _outputs(model(images, texts))
            all_image_features.append(image_features.float())         # kept on the GPU (the reference moves them to the host)
            all_text_features.append(text_features.float())
            logit_scale = logit_scale.mean()
            batch_size = images.shape[0]
            total_loss = loss_fn(image_features, text_features, logit_scale)     # (CE(I->T) + CE(T->I)) / 2
            weighted = total_loss.float() * batch_size
            cumulative_loss = weighted if cumulative_loss is None else cumulative_loss + weighted
            num_samples += batch_size
        if num_samples == 0:
            raise RuntimeError("clipa_amd.evaluate: no validation batches")
        val_metrics = get_clip_metrics(torch.cat(all_image_features), torch.cat(all_text_features), logit_scale)
    loss = cumulative_loss / num_samples
    return {**val_metrics, "clip_val_loss": loss.item(), "epoch": epoch, "num_samples": num_samples}
