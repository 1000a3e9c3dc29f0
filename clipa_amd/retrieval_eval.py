"""Zero-shot image-text retrieval with several captions per image (COCO, Flickr30k) through the MI355X engine: the
reference's `image_to_text_retrieval_eval` / `text_to_image_retrieval_eval`
(clipa_jax/evaluators/proj/image_text/image_text_retrieval.py) and the one-process `Evaluator.evaluate` of
clipa_jax/evaluators/proj/image_text/retrieval.py.

The reference builds the [N_img, N_txt] similarity matrix on the host and argsorts every row and every column.  Here the
features stay on the GPU and one kernel chain (`ops.retrieval_ranks_multi`, csrc/retrieval_multi.hip) counts, per image
and per text, the entries that beat the positive: O(N_img + N_txt) memory, no similarity matrix anywhere.  Only the ranks
travel to the host, where `recalls_from_ranks` applies the reference's Recall@k.

Tie rule (as `clipa_amd.evaluate`): the reference's unstable argsort places a positive anywhere among the entries that tie
with it; the engine reports the optimistic position, equal to the reference's whenever the positive has no exact tie.
"""
import numpy as np
import torch

from . import ops

RECALL_THRESHOLDS = (1, 5, 10)


def _host(x):
    return np.asarray(x.cpu() if torch.is_tensor(x) else x).astype(np.int64)


def recalls_from_ranks(i2t, t2i, has_caption, recall_thresholds=RECALL_THRESHOLDS):
    """0-based ranks of the positives -> {"img2txt": {"Recall@k": ...}, "txt2img": {...}} (np.float64).  i2t [N_img]:
    position of each image's best caption; t2i [N_txt]: position of each text's image; has_caption [N_img] bool.  An
    image without a caption misses at every k, as the reference's `any` over no captions does."""
    i2t, t2i, has = _host(i2t), _host(t2i), np.asarray(has_caption, dtype=bool)
    return {"img2txt": {f"Recall@{k}": np.mean(has & (i2t < k)) for k in recall_thresholds},
            "txt2img": {f"Recall@{k}": np.mean(t2i < k) for k in recall_thresholds}}


def _correspondence(c, n_images, n_texts, device):
    c = torch.as_tensor(c)
    if c.dim() != 1 or c.shape[0] != n_texts:
        raise RuntimeError(f"clipa_amd.image_text_retrieval: text_image_correspondence must hold one image index per text "
                           f"({n_texts}); got shape {tuple(c.shape)}")
    if c.dtype.is_floating_point or c.dtype.is_complex or c.dtype == torch.bool:
        raise RuntimeError(f"clipa_amd.image_text_retrieval: text_image_correspondence must be integer, got {c.dtype}")
    c = c.to(device=device, dtype=torch.int64)
    lo, hi = torch.stack([c.min(), c.max()]).tolist()
    if lo < 0 or hi >= n_images:
        raise RuntimeError(f"clipa_amd.image_text_retrieval: text_image_correspondence values must lie in "
                           f"[0, {n_images}); got [{lo}, {hi}]")
    return c


def image_text_retrieval(image_features, text_features, text_image_correspondence, recall_thresholds=RECALL_THRESHOLDS):
    """Image -> text and text -> image Recall@k of the reference's image_text_retrieval.py on the GPU: image features
    [N_img, E], text features [N_txt, E] (any float dtype; ranked in fp32 by their plain dot product, as the reference's
    `np.dot`), text_image_correspondence [N_txt] (list, array or tensor): text t describes image c[t].  Returns
    {"img2txt": {"Recall@1": ...}, "txt2img": {...}} with np.float64 values.  CPU features raise: there is no host
    fallback."""
    for name, t in (("image_features", image_features), ("text_features", text_features)):
        if not torch.is_tensor(t) or not t.is_cuda or t.dim() != 2:
            raise RuntimeError(f"clipa_amd.image_text_retrieval: {name} must be a 2-D GPU tensor (no CPU fallback); got "
                               f"{(t.device, tuple(t.shape)) if torch.is_tensor(t) else type(t).__name__}")
    if image_features.shape[1] != text_features.shape[1]:
        raise RuntimeError(f"clipa_amd.image_text_retrieval: feature widths differ: {image_features.shape[1]} vs "
                           f"{text_features.shape[1]}")
    n_img, n_txt = image_features.shape[0], text_features.shape[0]
    c = _correspondence(text_image_correspondence, n_img, n_txt, image_features.device)
    i2t_gt, _, t2i_gt, _ = ops.retrieval_ranks_multi(image_features.detach().float(), text_features.detach().float(), c)
    has_caption = torch.bincount(c, minlength=n_img) > 0
    return recalls_from_ranks(i2t_gt, t2i_gt, has_caption.cpu().numpy(), recall_thresholds)


def _ids(ids):
    return [int(v) for v in (ids.reshape(-1).tolist() if torch.is_tensor(ids) or isinstance(ids, np.ndarray) else ids)]


def correspondence_from_ids(image_ids, text_ids):
    """The reference's `id2img` step (retrieval.py, Evaluator.evaluate): text t describes the image whose id equals
    text_ids[t].  Raises on a duplicate image id and on a text whose image id was never seen.  -> np.int64 [N_txt]."""
    id2img = {}
    for i, v in enumerate(image_ids):
        if v in id2img:
            raise RuntimeError(f"clipa_amd.evaluate_retrieval: image id {v} appears twice (images {id2img[v]} and {i})")
        id2img[v] = i
    missing = [v for v in text_ids if v not in id2img]
    if missing:
        raise RuntimeError(f"clipa_amd.evaluate_retrieval: {len(missing)} text(s) name an image id that no image has, "
                           f"e.g. {missing[0]}")
    return np.array([id2img[v] for v in text_ids], dtype=np.int64)


def evaluate_retrieval(model, image_batches, text_batches):
    """`Evaluator.evaluate` of retrieval.py on one process.  image_batches yields (images, image_ids), text_batches
    (texts, image_ids), the inputs already on the device in the form the engine's encoders accept and the ids per
    sample (list, array or tensor).  Encodes with normalize=True under no_grad, keeps the features on the GPU, and returns
    {"img2txt", "txt2img", "num_images", "num_texts"}."""
    model.eval()
    img_feats, txt_feats, img_ids, txt_ids = [], [], [], []
    with torch.no_grad():
        for images, ids in image_batches:
            img_feats.append(model.encode_image(images, normalize=True).float())
            img_ids += _ids(ids)
        for texts, ids in text_batches:
            txt_feats.append(model.encode_text(texts, normalize=True).float())
            txt_ids += _ids(ids)
    if not img_feats or not txt_feats:
        raise RuntimeError("clipa_amd.evaluate_retrieval: no image or no text batches")
    img, txt = torch.cat(img_feats), torch.cat(txt_feats)
    if img.shape[0] != len(img_ids) or txt.shape[0] != len(txt_ids):
        raise RuntimeError(f"clipa_amd.evaluate_retrieval: {img.shape[0]} images / {txt.shape[0]} texts encoded but "
                           f"{len(img_ids)} / {len(txt_ids)} ids given")
    c = correspondence_from_ids(img_ids, txt_ids)
    out = image_text_retrieval(img, txt, torch.from_numpy(c))
    return {**out, "num_images": img.shape[0], "num_texts": txt.shape[0]}
