"""Top-k similarity search without a GPU: the fixture of tools/make_topk_golden.py against its generator and the margin cap, the
order's restatement (tests/topk_cases.py) against numpy's stable argsort and torch.topk, every public function of
clipa_amd/search.py on a host stand-in for the kernel (shard iteration, the carry, index_base, the empty and the iterable
gallery, kNN votes and ties), the argument errors of the C entry point (returned before any launch) and the exports."""
import os
from unittest import mock

import numpy as np
import pytest
import torch

import clipa_amd
from clipa_amd import search
from tools import make_topk_golden as G

from . import topk_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "topk.npz")
NAMES = ("classify", "retrieve", "knn")


@pytest.fixture(scope="module")
def golden():
    return np.load(FIXTURE, allow_pickle=False)


class HostOps:
    """Stands in for clipa_amd.ops on CPU tensors: the kernel by chain_fp32 + first_k."""

    def __init__(self):
        self.calls = []                       # (gallery rows, index_base, carry given)

    def topk_similarity(self, q, g, k, scale=None, index_base=0, carry=None, splits=0):
        self.calls.append((g.shape[0], index_base, carry is not None))
        assert q.dtype == g.dtype == torch.float32 and q.dim() == g.dim() == 2 and q.shape[1] == g.shape[1]
        with np.errstate(all="ignore"):
            v = T.chain_fp32(q.numpy(), g.numpy())
            if scale is not None:
                v = (np.float32(scale.item()) * v).astype(np.float32)
        idx = np.broadcast_to(index_base + np.arange(g.shape[0], dtype=np.int64)[None, :], v.shape)
        if carry is not None:
            assert tuple(carry[0].shape) == tuple(carry[1].shape) == (q.shape[0], k) and carry[1].dtype == torch.int64
            v, idx = np.concatenate([carry[0].numpy(), v], axis=1), np.concatenate([carry[1].numpy(), idx], axis=1)
        val, ind = T.first_k(v, idx, k)
        return torch.from_numpy(val.astype(np.float32)), torch.from_numpy(ind)


@pytest.fixture
def host_engine():
    """CPU tensors claim to be on the GPU and the kernel is the host stand-in: the Python glue runs as it does on the device."""
    ops = HostOps()
    with mock.patch.object(torch.Tensor, "is_cuda", True), mock.patch.object(search, "ops", ops):
        yield ops


def test_functions_are_exported():
    for name in ("topk_similarity", "classify_topk", "zero_shot_predict", "retrieve_topk", "knn_classify", "knn_metrics"):
        assert getattr(clipa_amd, name) is getattr(search, name)
    assert clipa_amd.search is search


# ---- the fixture -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_fixture_against_its_generator_and_the_margin_cap(golden, name):
    z, c = golden, G.CASES[name]
    for key in ("nq", "ng", "e", "k", "classes", "seed"):
        assert int(z[f"{name}_{key}"]) == c[key], key
    m = G.measure(name, int(z[f"{name}_draw"]))
    assert m["dev"] == float(z[f"{name}_dev"]) and 0 < m["dev"] < 1e-6
    keys = [("idx", "inside")] + ([("idx_t", "inside_t")] if name == "retrieve" else [])
    for ik, nk in keys:
        assert np.array_equal(m[ik], z[f"{name}_{ik}"]) and np.array_equal(m[nk], z[f"{name}_{nk}"])
        assert z[f"{name}_{nk}"].mean() <= G.INSIDE_CAP == 0.02
        assert m[ik].min() >= 0 and m[ik].shape[1] == c["k"]
    if name == "knn":
        assert np.array_equal(m["pred"], z["knn_pred"]) and np.array_equal(m["inside_vote"], z["knn_inside_vote"])
        assert z["knn_inside_vote"].mean() <= 0.02 and 0.2 < float(z["knn_top1"]) == m["top1"] < 0.95
    # the reference alone stays within the cap: the float32 chain's lists differ from the fp64 ones on rows inside the margin only
    q, g, _, _ = G.case_inputs(name, int(z[f"{name}_draw"]))
    v32 = T.chain_fp32(q, g)
    for (ik, nk), v in zip(keys, (v32, v32.T)):
        val, idx = T.topk_reference(v, c["k"])
        differ = (idx != m[ik]).any(axis=1)
        assert not (differ & ~m[nk]).any() and differ.mean() <= 0.02


# ---- the order -------------------------------------------------------------------------------------------------------------
def test_reference_equals_stable_argsort_and_torch_topk_on_tie_free_data():
    rng = np.random.RandomState(5)
    v = rng.permutation(40 * 90).reshape(40, 90).astype(np.float32) / 8 - 200          # distinct, exactly representable
    for k in (1, 7, 32):
        val, idx = T.topk_reference(v, k, index_base=1000)
        order = np.argsort(-v, axis=1, kind="stable")[:, :k]
        assert np.array_equal(idx, 1000 + order) and np.array_equal(val, np.take_along_axis(v, order, axis=1))
        tv, ti = torch.topk(torch.from_numpy(v), k, dim=1, largest=True, sorted=True)
        assert np.array_equal(idx - 1000, ti.numpy()) and np.array_equal(val, tv.numpy())


def test_reference_ties_nan_signed_zeros_and_empty_slots():
    nan, inf = float("nan"), float("inf")
    v = np.array([[1.0, 3.0, 3.0, -0.0, 0.0, 3.0],
                  [nan, 5.0, inf, nan, -inf, 5.0],
                  [-0.0, -1.0, 0.0, -0.0, -2.0, 0.0]], dtype=np.float32)
    val, idx = T.topk_reference(v, 4)
    assert idx.tolist() == [[1, 2, 5, 0], [0, 3, 2, 1], [0, 2, 3, 5]]                   # the stable sort: ties by the lower index
    assert np.isnan(val[1, :2]).all() and val[1, 2:].tolist() == [inf, 5.0] and val[0].tolist() == [3.0, 3.0, 3.0, 1.0]
    assert not np.signbit(val[2]).any()                                                   # zeros come out as +0
    val, idx = T.topk_reference(v[:, :2], 4, index_base=1 << 40)                          # fewer entries than k
    assert (idx[:, 2:] == -1).all() and np.isneginf(val[:, 2:]).all() and idx[0, :2].tolist() == [(1 << 40) + 1, 1 << 40]
    # an empty slot comes after a real -inf; merging a list with itself changes nothing
    mv, mi = T.first_k(np.array([[-inf, -inf, 2.0]]), np.array([[-1, 7, 3]]), 3)
    assert mi.tolist() == [[3, 7, -1]] and mv.tolist() == [[2.0, -inf, -inf]]


# ---- search.py on the host stand-in ----------------------------------------------------------------------------------------
def _rows(n, e, seed):
    x = np.random.RandomState(seed).standard_normal((n, e))
    return torch.from_numpy((x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32))


def test_shards_carry_and_index_base(host_engine):
    q, g = _rows(9, 16, 1), _rows(50, 16, 2)
    want_v, want_i = T.topk_reference(T.chain_fp32(q.numpy(), g.numpy()), 6)
    val, idx = search.topk_similarity(q, g, 6)
    assert host_engine.calls == [(50, 0, False)]
    assert np.array_equal(idx.numpy(), want_i) and np.array_equal(val.numpy(), want_v) and idx.dtype == torch.int64
    host_engine.calls.clear()
    val2, idx2 = search.topk_similarity(q, g, 6, chunk_rows=20)
    assert host_engine.calls == [(20, 0, False), (20, 20, True), (10, 40, True)]
    assert torch.equal(val2, val) and torch.equal(idx2, idx)
    host_engine.calls.clear()
    val3, idx3 = search.topk_similarity(q, (s for s in (g[:7], g[7:7], g[7:31], g[31:])), 6)       # an iterable, with an empty shard
    assert host_engine.calls == [(7, 0, False), (0, 7, True), (24, 7, True), (19, 31, True)]
    assert torch.equal(val3, val) and torch.equal(idx3, idx)
    # scale: a device scalar; -1 reverses the order
    valn, idxn = search.topk_similarity(q, g, 6, scale=torch.tensor(-1.0))
    want_v, want_i = T.topk_reference(-T.chain_fp32(q.numpy(), g.numpy()), 6)
    assert np.array_equal(idxn.numpy(), want_i) and np.array_equal(valn.numpy(), want_v)


def test_empty_gallery_and_fewer_rows_than_k(host_engine):
    q = _rows(4, 8, 3)
    for gallery in (q[:0], [], [q[:0], q[:0]]):
        val, idx = search.topk_similarity(q, gallery, 3)
        assert (idx == -1).all() and torch.isneginf(val).all() and tuple(val.shape) == (4, 3)
    val, idx = search.topk_similarity(q, q[:2], 5)
    assert (idx[:, :2] >= 0).all() and (idx[:, 2:] == -1).all() and torch.isneginf(val[:, 2:]).all()
    val, idx = search.topk_similarity(q[:0], q, 5)
    assert tuple(val.shape) == tuple(idx.shape) == (0, 5)


def test_check_finite_raises_on_a_nan_and_can_be_switched_off(host_engine):
    q, g = _rows(5, 8, 4), _rows(12, 8, 5)
    g[7, 3] = float("nan")
    with pytest.raises(RuntimeError, match="NaN similarities in 5 of 5 query rows"):
        search.topk_similarity(q, g, 3)
    val, idx = search.topk_similarity(q, g, 3, check_finite=False)
    assert (idx[:, 0] == 7).all() and torch.isnan(val[:, 0]).all() and not torch.isnan(val[:, 1:]).any()


def test_classify_retrieve_and_predict(host_engine):
    f, w, t = _rows(20, 12, 6), _rows(7, 12, 7), _rows(15, 12, 8)
    v = T.chain_fp32(f.numpy(), w.numpy())
    ids, logits = search.classify_topk(f, w, k=5)
    want_v, want_i = T.topk_reference(v, 5)
    assert np.array_equal(ids.numpy(), want_i) and np.array_equal(logits.numpy(), want_v)
    assert np.array_equal(ids[:, 0].numpy(), v.argmax(axis=1))
    r = search.retrieve_topk(f, t, k=4)
    vt = T.chain_fp32(f.numpy(), t.numpy())
    assert np.array_equal(r["i2t"][1].numpy(), T.topk_reference(vt, 4)[1]) and tuple(r["i2t"][1].shape) == (20, 4)
    assert np.array_equal(r["t2i"][1].numpy(), T.topk_reference(T.chain_fp32(t.numpy(), f.numpy()), 4)[1]) and tuple(r["t2i"][1].shape) == (15, 4)

    class Model(torch.nn.Module):
        def encode_image(self, images, normalize=False):
            assert normalize and not self.training
            return images * 1.0

    m = Model().train()
    ids2, logits2 = search.zero_shot_predict(m, w, [f[:8], (f[8:], "labels are ignored")], k=5)
    assert m.training and torch.equal(ids2, ids) and torch.equal(logits2, logits)
    bad = f.clone()
    bad[3, 0] = float("nan")
    with pytest.raises(RuntimeError, match="NaN logits in 1 of 20 images"):
        search.zero_shot_predict(m, w, [bad], k=5)
    with pytest.raises(RuntimeError, match="no batches"):
        search.zero_shot_predict(m, w, [], k=5)
    assert m.training


def test_knn_votes_ties_and_metrics(host_engine):
    # the vote rule against its restatement, with a planted tie: two classes with the same votes -> the lower class
    values = np.array([[0.9, 0.88, 0.88, 0.1], [0.5, 0.5, 0.2, 0.2], [0.3, 0.2, 0.1, 0.0]])
    labels = np.array([[2, 1, 1, 0], [3, 1, 1, 3], [0, -1, -1, -1]])
    pred, scores = search.knn_votes(values, labels, 0.07, 4)
    want, want_scores = T.knn_vote_reference(values, labels, 0.07, 4)
    assert pred.tolist() == want.tolist() == [1, 1, 0] and np.array_equal(scores, want_scores)
    assert scores[1, 1] == scores[1, 3] and scores[0, 1] > scores[0, 2]                  # two weaker neighbours outvote the nearest
    # the whole probe on separable clusters, in shards, against the restatement
    rng = np.random.RandomState(9)
    proto = rng.standard_normal((5, 16))
    ytr, yte = rng.randint(0, 5, size=120), rng.randint(0, 5, size=30)
    norm = lambda x: torch.from_numpy((x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32))     # noqa: E731
    tr, te = norm(proto[ytr] + 0.5 * rng.standard_normal((120, 16))), norm(proto[yte] + 0.5 * rng.standard_normal((30, 16)))
    out = search.knn_classify(tr, torch.from_numpy(ytr), te, k=7, temperature=0.07, chunk_rows=50)
    assert [c[:2] for c in host_engine.calls[-3:]] == [(50, 0), (50, 50), (20, 100)]
    val, idx = T.topk_reference(T.chain_fp32(te.numpy(), tr.numpy()), 7)
    assert np.array_equal(out["indices"].numpy(), idx)
    assert np.array_equal(out["pred"], T.knn_vote_reference(val, ytr[idx], 0.07, 5)[0]) and out["pred"].dtype == np.int64
    met = search.knn_metrics(tr, ytr, te, yte, k=7, chunk_rows=50)
    assert met == {"knn-count": 30, "knn-top1": np.float64((out["pred"] == yte).mean())} and met["knn-top1"] > 0.8
    assert type(met["knn-top1"]) is np.float64 and type(met["knn-count"]) is int
    # fewer training rows than k: the empty slots do not vote
    few = search.knn_classify(tr[:3], ytr[:3], te, k=7, num_classes=5)
    assert (few["indices"][:, 3:] == -1).all() and set(few["pred"].tolist()) <= set(ytr[:3].tolist())
    for bad, match in ((dict(temperature=0.0), "temperature"), (dict(num_classes=2), "num_classes"), (dict(k=33), r"\[1, 32\]")):
        with pytest.raises(RuntimeError, match=match):
            search.knn_classify(tr, ytr, te, **bad)
    with pytest.raises(RuntimeError, match="train_labels for a gallery"):
        search.knn_classify(tr, ytr[:100], te, k=7)


def test_argument_errors_are_raised(host_engine):
    q, g = _rows(4, 8, 1), _rows(6, 8, 2)
    for k in (0, 33, 2.0, True):
        with pytest.raises(RuntimeError, match=r"integer in \[1, 32\]"):
            search.topk_similarity(q, g, k)
    with pytest.raises(RuntimeError, match=r"must be \[Nq, E\] and"):
        search.topk_similarity(q, g[:, :7], 2)
    with pytest.raises(RuntimeError, match="chunk_rows"):
        search.topk_similarity(q, g, 2, chunk_rows=0)
    with pytest.raises(RuntimeError, match="brings its own shards"):
        search.topk_similarity(q, [g], 2, chunk_rows=3)
    with pytest.raises(RuntimeError, match="2-D float GPU tensor"):
        search.topk_similarity(q[0], g, 2)


def test_cpu_tensors_raise():
    q, g = torch.zeros(4, 8), torch.zeros(3, 8)
    for call in (lambda: search.topk_similarity(q, g, 2), lambda: search.classify_topk(q, g), lambda: search.retrieve_topk(q, g, 2),
                 lambda: search.knn_classify(g, [0, 1, 2], q, k=2), lambda: search.zero_shot_predict(torch.nn.Identity(), g, [q])):
        with pytest.raises(RuntimeError, match="GPU"):
            call()


# ---- the C entry point ---------------------------------------------------------------------------------------------------
def test_c_entry_argument_errors_come_back_as_codes():
    """CLIPA_ERR_ARG plus clipa_last_error, before any device is touched."""
    from clipa_amd import lib
    h = lib.load()
    p = 4096                                                    # an aligned, never dereferenced address
    big = 1 << 40

    def call(Q=p, G=p, Nq=3, Ng=5, E=8, ldq=8, ldg=8, scale=None, k=4, base=0, splits=0, cv=None, ci=None, ov=p, oi=p, ws=p, wsb=big):
        return h.clipa_topk(Q, G, Nq, Ng, E, ldq, ldg, scale, k, base, splits, cv, ci, ov, oi, ws, wsb, None)

    assert call(Nq=0, Q=None, G=None, ov=None, oi=None, ws=None, wsb=0) == 0              # Nq = 0: nothing to do
    for k in (0, 33):
        assert call(k=k) < 0 and f"k = {k}" in lib.last_error()
    assert call(Nq=-1) < 0 and "must be >= 0" in lib.last_error()
    assert call(Ng=-1) < 0 and "must be >= 0" in lib.last_error()
    assert call(Ng=(1 << 31) - 128) < 0 and "too large" in lib.last_error() and "shards" in lib.last_error()
    assert call(Nq=(1 << 31) - 128) < 0 and "too large" in lib.last_error()
    assert call(ldq=7) < 0 and "lda = 7" in lib.last_error()
    assert call(ldg=10) < 0 and "multiples of 4" in lib.last_error()
    assert call(Q=None) < 0 and "pointer argument 0 is null" in lib.last_error()
    assert call(G=p + 4) < 0 and "pointer argument 1 is null or not 16-byte aligned" in lib.last_error()
    assert call(oi=None) < 0 and "pointer argument 3 is null" in lib.last_error()
    assert call(ws=None) < 0 and "pointer argument 4 is null" in lib.last_error()
    assert call(scale=p + 2) < 0 and "scale" in lib.last_error()
    assert call(cv=p) < 0 and "come together" in lib.last_error()
    assert call(ci=p) < 0 and "come together" in lib.last_error()
    assert call(cv=p + 8, ci=p) < 0 and "carry pointers" in lib.last_error()
    assert call(base=-1) < 0 and "index_base" in lib.last_error()
    assert call(splits=-1) < 0 and "splits = -1" in lib.last_error()
    assert call(Ng=257, splits=4) < 0 and "splits = 4" in lib.last_error()               # three gallery tiles
    assert call(Ng=0, splits=2) < 0 and "splits = 2" in lib.last_error()
    assert call(Ng=257, splits=3, wsb=3 * 3 * 4 * 8 - 1) < 0 and "workspace too small" in lib.last_error()
    # the size function: splits x Nq x k keys of 8 bytes; splits = 0 is the entry's own choice, at most one per gallery tile
    assert h.clipa_topk_workspace(3, 257, 4, 3) == 3 * 3 * 4 * 8 and h.clipa_topk_workspace(3, 257, 4, 0) == 3 * 3 * 4 * 8
    assert h.clipa_topk_workspace(3, 1 << 20, 4, 0) == 512 * 3 * 4 * 8 and h.clipa_topk_workspace(128 * 512, 1 << 20, 4, 0) == 128 * 512 * 4 * 8
    assert h.clipa_topk_workspace(3, 0, 4, 0) == 16 and h.clipa_topk_workspace(0, 5, 4, 0) == 16
