"""Top-k similarity search on the engine (csrc/topk.hip): "which are the best k?" - the five most likely classes of an image
(`output.topk` of clipa_torch/training/zero_shot.py:47-50), the ten nearest images of a caption (the top-k lists of
clipa_jax/evaluators/proj/image_text/image_text_retrieval.py:77-82), the twenty nearest training images of a test image (the
weighted k-nearest-neighbour probe of Wu et al. 2018, "Unsupervised Feature Learning via Non-Parametric Instance
Discrimination", as DINO and others report it) - without the [Nq, Ng] similarity matrix, in O(Nq k) memory.  The gallery may
have any size because it arrives in shards: every call merges its shard into the running lists of the earlier ones.

The order is strict and total - the larger fp32 value first, equal values by the lower gallery index, a NaN before every
number - so the lists are a function of the inputs alone: the same bit for bit whatever the shard sizes, the shard order or the
launch shape.  There is no host fallback: CPU tensors raise."""
import numpy as np
import torch

from . import ops
from ._eval_common import _features, _inference

MAX_K = 32                                    # entries per list the kernel keeps (TK_MAX)


def _k(k, who):
    if not isinstance(k, (int, np.integer)) or isinstance(k, bool) or not 1 <= k <= MAX_K:
        raise RuntimeError(f"clipa_amd.{who}: k = {k!r} must be an integer in [1, {MAX_K}]")
    return int(k)


def _shards(gallery, chunk_rows, who):
    """-> an iterator over the gallery's shards in index order."""
    if torch.is_tensor(gallery):
        if chunk_rows is None:
            return iter((gallery,))
        if not isinstance(chunk_rows, (int, np.integer)) or isinstance(chunk_rows, bool) or chunk_rows < 1:
            raise RuntimeError(f"clipa_amd.{who}: chunk_rows = {chunk_rows!r} must be an integer >= 1")
        return (gallery[a:a + int(chunk_rows)] for a in range(0, max(gallery.shape[0], 1), int(chunk_rows)))
    if chunk_rows is not None:
        raise RuntimeError(f"clipa_amd.{who}: chunk_rows cuts a tensor; an iterable gallery brings its own shards")
    return iter(gallery)


def topk_similarity(queries, gallery, k, *, scale=None, chunk_rows=None, check_finite=True):
    """queries [Nq, E]; gallery [Ng, E] or an iterable of [n_s, E] shards in index order (the way a dataset's features arrive); 2-D
    float GPU tensors, used as fp32.  A tensor gallery is cut into shards of chunk_rows rows when that is given.  scale: an
    optional f32 device scalar s, values = fl(s * q . g).
    -> (values f32 [Nq, k], indices int64 [Nq, k]) on the device, best first (ops.topk_similarity): index = the row's position
    in the whole gallery; with fewer than k gallery rows the tail is (-inf, -1).  One launch pair per shard, the running lists
    carried from shard to shard.  A NaN leads its row's list, so check_finite looks at the first slots only - one reduction
    over [Nq] and one host read - and raises; with check_finite=False nothing synchronises."""
    who = "topk_similarity"
    k = _k(k, who)
    q = _features(queries, "queries", who)
    carry, base = None, 0
    for shard in _shards(gallery, chunk_rows, who):
        g = _features(shard, "gallery", who)
        if g.shape[1] != q.shape[1]:
            raise RuntimeError(f"clipa_amd.{who}: queries {tuple(q.shape)} and gallery shard {tuple(g.shape)} must be [Nq, E] and "
                               f"[n, E]")
        carry = ops.topk_similarity(q, g, k, scale=scale, index_base=base, carry=carry)
        base += g.shape[0]
    if carry is None:                          # an iterable without shards: the empty gallery
        carry = ops.topk_similarity(q, q[:0], k, scale=scale)
    values, indices = carry
    if check_finite and q.shape[0]:
        bad = int(torch.isnan(values[:, 0]).sum())
        if bad:
            raise RuntimeError(f"clipa_amd.{who}: NaN similarities in {bad} of {q.shape[0]} query rows (non-finite features or scale)")
    return values, indices


def classify_topk(image_features, classifier, k=5):
    """The k most likely classes of every image against a classifier from build_classifier: image_features [B, E], classifier
    [C, E] -> (class_ids int64 [B, k], logits f32 [B, k]), best first, equal logits by the lower class.  logits = f . w in fp32
    without the reference's `100 *` (zero_shot.py:77): it changes no order but can merge neighbours (see clipa_zeroshot_ranks).
    k above C leaves (-1, -inf) in the tail."""
    values, indices = topk_similarity(image_features, classifier, _k(k, "classify_topk"))
    return indices, values


def zero_shot_predict(model, classifier, batches, k=5):
    """The loop of zero_shot.run (zero_shot.py:70-84) without labels: batches yield images (or tuples whose first entry is the
    images) on the device; per batch encode_image(normalize=True) and classify_topk.  no_grad and eval mode, the model's
    previous mode put back.  -> (class_ids int64 [N, k], logits f32 [N, k]), concatenated on the device; one host read at the
    end for the NaN check of all batches."""
    who = "zero_shot_predict"
    k = _k(k, who)
    w = _features(classifier, "classifier", who)
    ids, logits = [], []
    with _inference(model) as m:
        for batch in batches:
            images = batch[0] if isinstance(batch, (tuple, list)) else batch
            v, i = topk_similarity(m.encode_image(images, normalize=True), w, k, check_finite=False)
            ids.append(i)
            logits.append(v)
    if not ids:
        raise RuntimeError(f"clipa_amd.{who}: no batches")
    ids, logits = torch.cat(ids), torch.cat(logits)
    bad = int(torch.isnan(logits[:, 0]).sum()) if logits.shape[0] else 0
    if bad:
        raise RuntimeError(f"clipa_amd.{who}: NaN logits in {bad} of {logits.shape[0]} images")
    return ids, logits


def retrieve_topk(image_features, text_features, k=10):
    """Both directions of retrieval: -> {"i2t": (values, indices), "t2i": (values, indices)}, the k nearest texts of each image
    [Ni, k] and the k nearest images of each text [Nt, k] - two searches with the operands swapped."""
    k = _k(k, "retrieve_topk")
    return {"i2t": topk_similarity(image_features, text_features, k), "t2i": topk_similarity(text_features, image_features, k)}


def knn_votes(values, neighbour_labels, temperature, num_classes):
    """The vote rule of the weighted kNN probe on host arrays: values [Nt, k] similarities and neighbour_labels [Nt, k] (-1 = no
    neighbour) -> (pred int64 [Nt], scores float64 [Nt, C]): class c scores the sum of exp(v / T) over the neighbours labelled c,
    added in list order in float64; the prediction is the lowest class among the best scores."""
    v = np.asarray(values, dtype=np.float64)
    lab = np.asarray(neighbour_labels, dtype=np.int64)
    scores = np.zeros((v.shape[0], int(num_classes)), dtype=np.float64)
    rows = np.arange(v.shape[0])
    for j in range(v.shape[1]):
        ok = lab[:, j] >= 0
        np.add.at(scores, (rows[ok], lab[ok, j]), np.exp(v[ok, j] / float(temperature)))
    return scores.argmax(axis=1).astype(np.int64), scores


def knn_classify(train_features, train_labels, test_features, k=20, temperature=0.07, num_classes=None, chunk_rows=None):
    """Weighted k-nearest-neighbour classification (Wu et al. 2018): train_features [N, E] (a tensor or an iterable of shards) and
    test_features [Nt, E], unit-norm rows supplied by the caller; train_labels [N] integers in [0, C).  The top-k search over
    the training features runs on the device, in shards of chunk_rows rows; the votes exp(v / temperature) are summed per class
    on the host in float64 from the [Nt, k] result (knn_votes), ties to the lowest class.
    -> {"pred": int64 [Nt] (host array), "values", "indices": the [Nt, k] search result on the device}."""
    who = "knn_classify"
    k = _k(k, who)
    if not float(temperature) > 0:
        raise RuntimeError(f"clipa_amd.{who}: temperature = {temperature} must be > 0")
    y = np.asarray(train_labels.cpu() if torch.is_tensor(train_labels) else train_labels)
    if y.ndim != 1 or y.dtype.kind not in "iu" or (len(y) and y.min() < 0):
        raise RuntimeError(f"clipa_amd.{who}: train_labels must be a 1-D array of integers >= 0")
    C = int(num_classes) if num_classes is not None else (int(y.max()) + 1 if len(y) else 1)
    if len(y) and y.max() >= C:
        raise RuntimeError(f"clipa_amd.{who}: train_labels reach {int(y.max())} with num_classes = {C}")
    values, indices = topk_similarity(test_features, train_features, k, chunk_rows=chunk_rows)
    idx = indices.cpu().numpy()
    if len(idx) and idx.max() >= len(y):
        raise RuntimeError(f"clipa_amd.{who}: {len(y)} train_labels for a gallery with row {int(idx.max())}")
    lab = np.where(idx >= 0, y.astype(np.int64)[np.maximum(idx, 0)], -1) if len(y) else np.full(idx.shape, -1, dtype=np.int64)
    pred, _ = knn_votes(values.cpu().numpy(), lab, temperature, C)
    return {"pred": pred, "values": values, "indices": indices}


def knn_metrics(train_features, train_labels, test_features, test_labels, k=20, temperature=0.07, num_classes=None,
                chunk_rows=None):
    """knn_classify against test_labels [Nt] -> {"knn-count": int, "knn-top1": np.float64} (NaN without rows)."""
    t = np.asarray(test_labels.cpu() if torch.is_tensor(test_labels) else test_labels).astype(np.int64)
    pred = knn_classify(train_features, train_labels, test_features, k, temperature, num_classes, chunk_rows)["pred"]
    if t.shape != pred.shape:
        raise RuntimeError(f"clipa_amd.knn_metrics: test_labels {t.shape} for {pred.shape[0]} test rows")
    n = int(len(t))
    return {"knn-count": n, "knn-top1": np.float64((pred == t).sum()) / np.float64(n) if n else np.float64("nan")}
