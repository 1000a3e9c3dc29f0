"""GPU tests of top-k similarity search (csrc/topk.hip, clipa_amd/search.py).  Kernel level: exactly representable inputs (small
integers, or multiples of 2^-6 with every partial sum far below 2^24), so float32, float64 and any summation order agree and
every comparison is for equality over every row, at the smallest shapes at which the tiling can go wrong: a row-tile edge, two
column-tile edges, the 32-wide k chunk, every split count, shards that are not tile aligned.  End to end: the fixture of
tools/make_topk_golden.py under its margin rule, and a toy engine model."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import clipa_amd
from clipa_amd import lib, ops, search, zero_shot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tools import make_topk_golden as G             # noqa: E402
from . import topk_cases as T                       # noqa: E402
from .conftest import load_golden                   # noqa: E402
from .test_zeroshot_gpu import _toy_images, _toy_prompts      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
FIXTURE = os.path.join(ROOT, "tests", "golden", "topk.npz")
NQ, NG, E, LDQ = 130, 257, 36, 40                   # a row-tile edge, two column-tile edges; ldq = 40, ldg = 36
SPLITS = (0, 1, 2, 3)


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=DEV, dtype=dtype)


def _host(t):
    return t.detach().cpu().numpy()


def _padded(a, ld):
    """a [n, e] -> its [n, e] view of a [n, ld] device buffer whose other columns hold 77 (never to be read as data)."""
    buf = torch.full((a.shape[0], ld), 77.0, device=DEV)
    buf[:, :a.shape[1]] = _dev(a)
    return buf[:, :a.shape[1]]


def _run(q, g, k, scale=None, ldq=None, **kw):
    qd = _padded(q, ldq) if ldq else _dev(q)
    s = None if scale is None else torch.tensor([scale], device=DEV, dtype=torch.float32)
    val, idx = ops.topk_similarity(qd, _dev(g), k, scale=s, **kw)
    assert val.dtype == torch.float32 and idx.dtype == torch.int64 and tuple(val.shape) == tuple(idx.shape) == (q.shape[0], k)
    return _host(val), _host(idx)


def _same(got, want):
    return np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0], equal_nan=True)


@pytest.fixture(scope="module")
def ragged():
    """name -> (q, g, exact products): computed once, shared, never written to."""
    out = {}
    for name, (q, g) in (("integer", T.integer_case(NQ, NG, E, 41)), ("fraction", T.fraction_case(NQ, NG, E, 42)),
                         ("position", T.position_coded(NQ, NG, E))):
        out[name] = (q, g, T.exact_product(q, g))
    q, g = T.fraction_case(NQ, NG, E, 43)
    g[101] = g[100]
    g[228] = g[100]                                   # duplicates at j, j + 1 and j + 128
    g[128] = g[127]                                   # across the boundary of splits 2 and 3
    g[256] = g[255]                                   # and into the last, one-row tile
    q[0] = g[100]                                     # |g_100|^2 is the best of row 0: the triple leads its list
    out["ties"] = (q, g, T.exact_product(q, g))
    return out


# ---- 1. minimal and ragged shapes, splits ----------------------------------------------------------------------------------
def test_one_by_one():
    val, idx = _run(np.array([[3.0]], dtype=np.float32), np.array([[-2.0]], dtype=np.float32), 1)
    assert val.tolist() == [[-6.0]] and idx.tolist() == [[0]]


@pytest.mark.parametrize("k", [1, 5, 32])
@pytest.mark.parametrize("name", ["integer", "fraction", "position", "ties"])
def test_ragged_shapes_equal_the_reference_for_every_split(ragged, name, k):
    q, g, v = ragged[name]
    want = T.topk_reference(v, k)
    if name == "position":                            # every value names its (i, j)
        assert np.array_equal(want[0], g[want[1], (np.arange(NQ) % E)[:, None]])
    if name == "ties" and k >= 5:
        assert want[1][0, :3].tolist() == [100, 101, 228]
    first = None
    for splits in SPLITS:
        got = _run(q, g, k, ldq=LDQ, splits=splits)
        assert _same(got, want), (name, k, splits)
        first = first or got
        assert got[0].tobytes() == first[0].tobytes() and got[1].tobytes() == first[1].tobytes()      # bit-identical


@pytest.mark.parametrize("ng", [20, 40])
def test_fewer_entries_than_k(ng):
    q, g = T.integer_case(NQ, ng, E, 44)
    val, idx = _run(q, g, 32)
    want = T.topk_reference(T.exact_product(q, g), 32)
    assert _same((val, idx), want)
    if ng < 32:
        assert (idx[:, ng:] == -1).all() and np.isneginf(val[:, ng:]).all() and (idx[:, :ng] >= 0).all()


# ---- 2. planted ties -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("splits", SPLITS)
def test_all_equal_gallery_and_a_tie_at_the_kth_position(splits):
    q = T.integer_case(NQ, 1, E, 45)[0]
    val, idx = _run(q, np.ones((NG, E), dtype=np.float32), 32, splits=splits)
    assert np.array_equal(idx, np.broadcast_to(np.arange(32), (NQ, 32))) and np.array_equal(val, np.broadcast_to(q.sum(1, keepdims=True), (NQ, 32)))
    # column 0 of the gallery falls in pairs: rows 2m and 2m + 1 tie, so for odd k the tie sits at the k-th / (k + 1)-th entry
    e0 = np.zeros((3, E), dtype=np.float32)
    e0[:, 0] = (1, 2, 3)
    g = np.zeros((NG, E), dtype=np.float32)
    g[:, 0] = -(np.arange(NG) // 2)
    for k in (5, 31):
        val, idx = _run(e0, g, k, splits=splits)
        assert np.array_equal(idx, np.broadcast_to(np.arange(k), (3, k))) and _same((val, idx), T.topk_reference(T.exact_product(e0, g), k))
    # and rising: rows 128 .. 256 all hold the best value - the whole second tile and the one row of the third - in index order
    g[:, 0] = np.minimum(np.arange(NG), 128)
    val, idx = _run(e0, g, 7, splits=splits)
    assert np.array_equal(idx, np.broadcast_to(np.arange(128, 135), (3, 7)))


def test_signed_zeros_tie():
    q, g = T.integer_case(NQ, NG, E, 46)
    q[3] = 0
    q[129] = 0
    for scale in (-1.0, None):                         # a zero row times -1: every entry is -0
        val, idx = _run(q, g, 6, scale=scale)
        assert _same((val, idx), T.topk_reference(T.exact_product(q, g, scale), 6))
        assert np.array_equal(idx[[3, 129]], np.broadcast_to(np.arange(6), (2, 6))) and (val[[3, 129]] == 0).all()
        assert not np.signbit(val[[3, 129]]).any()


# ---- 3. sharding -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k", [("integer", 5), ("ties", 32), ("fraction", 32)])
def test_shards_in_any_sequence_equal_one_call(ragged, name, k):
    q, g, v = ragged[name]
    qd, gd = _dev(q), _dev(g)
    whole = ops.topk_similarity(qd, gd, k)
    assert _same((_host(whole[0]), _host(whole[1])), T.topk_reference(v, k))
    cuts = [(0, 100), (100, 228), (228, 257)]         # not tile aligned
    for order in (cuts, cuts[::-1], [cuts[1], cuts[2], cuts[0]]):
        carry = None
        for a, b in order:
            carry = ops.topk_similarity(qd, gd[a:b], k, index_base=a, carry=carry, splits=1 if a else 0)
        assert torch.equal(carry[0], whole[0]) and torch.equal(carry[1], whole[1]), order
    # the public function cuts the same gallery itself
    val, idx = search.topk_similarity(qd, gd, k, chunk_rows=100)
    assert torch.equal(val, whole[0]) and torch.equal(idx, whole[1])
    val, idx = search.topk_similarity(qd, [gd[:100], gd[100:228], gd[228:]], k)
    assert torch.equal(val, whole[0]) and torch.equal(idx, whole[1])


def test_index_base_above_2_31_and_out_aliasing_carry(ragged):
    q, g, v = ragged["integer"]
    k, base = 9, (1 << 33) + 5
    want = T.topk_reference(v, k, index_base=base)
    assert want[1].min() > 1 << 33
    assert _same(_run(q, g, k, index_base=base), want)
    # the C entry with out = carry: first shard [100, 257) into fresh buffers, then [0, 100) merged in place
    qd, gd = _dev(q), _dev(g)
    val = torch.empty((NQ, k), device=DEV)
    idx = torch.empty((NQ, k), device=DEV, dtype=torch.int64)
    ws = torch.empty(lib.query("clipa_topk_workspace", NQ, NG, k, 0) // 4, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())       # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    g2 = gd[100:].contiguous()
    lib.call("clipa_topk", p(qd), p(g2), NQ, NG - 100, E, E, E, None, k, base + 100, 0, None, None, p(val), p(idx), p(ws),
             ws.numel() * 4, stream)
    lib.call("clipa_topk", p(qd), p(gd), NQ, 100, E, E, E, None, k, base, 0, p(val), p(idx), p(val), p(idx), p(ws),
             ws.numel() * 4, stream)
    assert _same((_host(val), _host(idx)), want)


def test_empty_gallery_and_zero_columns(ragged):
    q, g, v = ragged["integer"]
    qd = _dev(q)
    val, idx = ops.topk_similarity(qd, _dev(g)[:0], 4)
    assert (idx == -1).all() and torch.isneginf(val).all()
    carry = ops.topk_similarity(qd, _dev(g), 4, index_base=10)
    val, idx = ops.topk_similarity(qd, _dev(g)[:0], 4, index_base=500, carry=carry)       # the output is the carry
    assert torch.equal(val, carry[0]) and torch.equal(idx, carry[1])
    val, idx = ops.topk_similarity(qd[:, :0], _dev(g)[:, :0], 4, index_base=7)            # E = 0: every value is +0
    assert (val == 0).all() and np.array_equal(_host(idx), np.broadcast_to(np.arange(7, 11), (NQ, 4)))
    val, idx = ops.topk_similarity(qd[:0], _dev(g), 4)
    assert tuple(val.shape) == tuple(idx.shape) == (0, 4)


# ---- 4. scale and NaN ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [100.0, -1.0, None])
def test_scale_is_read_on_the_device(ragged, scale):
    q, g, _ = ragged["fraction"]                      # 100 * (a multiple of 2^-12 below 2^6) still fits 24 bits
    want = T.topk_reference(T.exact_product(q, g, scale), 10)
    assert _same(_run(q, g, 10, scale=scale, ldq=LDQ), want)
    if scale == -1.0:                                 # the order is reversed: the best are the fp64 smallest
        assert np.array_equal(want[1][:, 0], np.argmin(T.exact_product(q, g), axis=1))


def test_a_nan_leads_every_list(ragged):
    q, g, _ = ragged["integer"]
    g = g.copy()
    g[177, 3] = np.nan
    with np.errstate(invalid="ignore"):
        want = T.topk_reference(T.exact_product(q, g), 5)
    for splits in SPLITS:
        val, idx = _run(q, g, 5, splits=splits)
        assert (idx[:, 0] == 177).all() and np.isnan(val[:, 0]).all() and not np.isnan(val[:, 1:]).any()
        assert _same((val, idx), want)
    with pytest.raises(RuntimeError, match=f"NaN similarities in {NQ} of {NQ} query rows"):
        search.topk_similarity(_dev(q), _dev(g), 5)
    val, idx = search.topk_similarity(_dev(q), _dev(g), 5, check_finite=False)
    assert _same((_host(val), _host(idx)), want)


# ---- 5. the three kernels on rank_tile agree on data that is not exact -----------------------------------------------------
def test_first_entry_equals_the_other_rank_tile_kernels_bit_for_bit():
    rng = np.random.RandomState(7)
    f, w = rng.standard_normal((200, 512)), rng.standard_normal((300, 512))
    fd = _dev(f / np.linalg.norm(f, axis=1, keepdims=True))
    wd = _dev(w / np.linalg.norm(w, axis=1, keepdims=True))
    val, idx = ops.topk_similarity(fd, wd, 5)
    _, _, pred = ops.zeroshot_ranks(fd, wd, torch.zeros((200, 1), device=DEV, dtype=torch.int32))
    pred2, best = ops.fewshot_predict(fd, wd)
    assert torch.equal(idx[:, 0], pred.to(torch.int64)) and torch.equal(pred2, pred)
    assert torch.equal(val[:, 0], best)               # bit for bit: one chain per entry, whichever kernel
    assert (val[:, :-1] >= val[:, 1:]).all()


# ---- 6. end to end on the fixture ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    return np.load(FIXTURE, allow_pickle=False)


def _check_lists(name, got_val, got_idx, want_idx, inside, v64, dev):
    out = ~inside
    wrong = (got_idx != want_idx).any(axis=1)
    err = np.abs(got_val.astype(np.float64) - np.take_along_axis(v64, np.maximum(got_idx, 0), axis=1)).max()
    print(f"{name}: rows inside the margin {int(inside.sum())} of {len(inside)}, rows that differ {int(wrong.sum())}, "
          f"max |value - fp64| {err:.3g} = {err / dev:.2f} dev")
    assert inside.mean() <= 0.02
    assert np.array_equal(got_idx[out], want_idx[out])                     # rows outside the margin: exactly
    # a reported value is the float32 chain of its own entry: within float32 noise of the fp64 product (8 dev, as fewshot's best)
    assert err <= 8 * dev


def test_classify_retrieve_and_knn_on_the_fixture(golden):
    z = golden
    q, g, _, _ = G.case_inputs("classify", int(z["classify_draw"]))
    ids, logits = search.classify_topk(_dev(q), _dev(g), k=5)
    assert ids.dtype == torch.int64 and logits.dtype == torch.float32 and ids.is_cuda
    _check_lists("classify", _host(logits), _host(ids), z["classify_idx"], z["classify_inside"], T.logits_fp64(q, g), float(z["classify_dev"]))

    q, g, _, _ = G.case_inputs("retrieve", int(z["retrieve_draw"]))
    r = search.retrieve_topk(_dev(q), _dev(g), k=10)
    v = T.logits_fp64(q, g)
    _check_lists("i2t", _host(r["i2t"][0]), _host(r["i2t"][1]), z["retrieve_idx"], z["retrieve_inside"], v, float(z["retrieve_dev"]))
    _check_lists("t2i", _host(r["t2i"][0]), _host(r["t2i"][1]), z["retrieve_idx_t"], z["retrieve_inside_t"], v.T, float(z["retrieve_dev"]))

    c = G.CASES["knn"]
    q, g, yq, yg = G.case_inputs("knn", int(z["knn_draw"]))
    out = search.knn_classify(_dev(g), yg, _dev(q), k=c["k"], temperature=c["temperature"], num_classes=c["classes"],
                              chunk_rows=c["chunk_rows"])
    _check_lists("knn", _host(out["values"]), _host(out["indices"]), z["knn_idx"], z["knn_inside"], T.logits_fp64(q, g), float(z["knn_dev"]))
    sure = ~z["knn_inside_vote"]
    assert z["knn_inside_vote"].mean() <= 0.02 and np.array_equal(out["pred"][sure], z["knn_pred"][sure])
    met = search.knn_metrics(_dev(g), yg, _dev(q), yq, k=c["k"], temperature=c["temperature"], num_classes=c["classes"],
                             chunk_rows=c["chunk_rows"])
    hits = int((z["knn_pred"][sure] == yq[sure]).sum())
    assert met["knn-count"] == c["nq"] and hits <= round(met["knn-top1"] * c["nq"]) <= hits + int((~sure).sum())


# ---- 7. on a toy engine model ----------------------------------------------------------------------------------------------
def test_zero_shot_predict_on_an_engine_model():
    g = load_golden("cls_erf")
    m = clipa_amd.CLIP(**g.cfg, output_dict=True)
    m.load_state_dict(g.sd, strict=True)
    m.to(DEV).train()
    ctx, vocab = g.cfg["text_cfg"]["context_length"], g.cfg["text_cfg"]["vocab_size"]
    C, Tn, B = 11, 3, 96
    images = _toy_images(B, g.cfg["vision_cfg"]["image_size"], seed=17).to(DEV)
    clf = zero_shot.build_classifier(m, _toy_prompts(C, Tn, ctx, vocab).to(DEV), np.repeat(np.arange(C), Tn), C, text_batch_size=16)
    rec = []
    enc = m.encode_image
    m.encode_image = lambda *a, **k: (rec.append(enc(*a, **k)), rec[-1])[1]
    try:
        ids, logits = search.zero_shot_predict(m, clf, [images[:50], (images[50:], None)], k=5)
    finally:
        m.encode_image = enc
    assert m.training and [len(t) for t in rec] == [50, 46]
    assert tuple(ids.shape) == tuple(logits.shape) == (B, 5) and ids.dtype == torch.int64 and logits.dtype == torch.float32
    assert ids.is_cuda and logits.is_cuda
    assert (logits[:, :-1] >= logits[:, 1:]).all() and (ids >= 0).all() and (ids < C).all()
    assert all(len(set(row)) == 5 for row in _host(ids).tolist())
    feat = torch.cat(rec).float()
    pred = zero_shot.zero_shot_ranks(feat, clf, torch.zeros(B, dtype=torch.int64, device=DEV))["pred"]
    assert torch.equal(ids[:, 0], pred.to(torch.int64))
    ids12, _ = search.classify_topk(feat, clf, k=12)                      # k above C: the tail is empty
    assert (ids12[:, 11] == -1).all() and torch.equal(ids12[:, :5], ids)
