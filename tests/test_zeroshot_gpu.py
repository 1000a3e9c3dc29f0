"""GPU tests of fused zero-shot classification (clipa_amd/zero_shot.py, csrc/zeroshot.hip; the references'
clipa_torch/training/zero_shot.py and clipa_jax/evaluators/proj/image_text/discriminative_classifier.py).  Kernel level: exactly
representable inputs (small integers, every sum far below 2^24), so every comparison is for equality, with planted ties at the
smallest shapes at which the tiling can go wrong.  End to end: the fixture of tools/make_zeroshot_golden.py, whose margin rule
makes every per-row rank well defined; build_classifier / evaluate_zero_shot on a stand-in model that records its calls and on a
toy engine model."""
import math
import os
import sys

import numpy as np
import pytest
import torch

import clipa_amd
from clipa_amd import ops, zero_shot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tools import make_zeroshot_golden as G         # noqa: E402
from . import zeroshot_cases as Z                   # noqa: E402
from .conftest import load_golden                   # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
FIXTURE = os.path.join(ROOT, "tests", "golden", "zeroshot.npz")


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=DEV, dtype=dtype)


def _host(t):
    return t.detach().cpu().numpy()


def _padded(a, ld):
    """a [n, e] -> its [n, e] view of a [n, ld] device buffer whose other columns hold 77 (never to be read as data)."""
    buf = torch.full((a.shape[0], ld), 77.0, device=DEV)
    buf[:, :a.shape[1]] = _dev(a)
    return buf[:, :a.shape[1]]


@pytest.fixture(scope="module")
def golden():
    return np.load(FIXTURE, allow_pickle=False)


# ---- 1. class mean, exact --------------------------------------------------------------------------------------------------
CM_COUNTS = (1, 3, 80, 2, 7)


def _integer_prompts():
    """Integer rows whose class means are integers in [-3, 3]: every sum, the means and the sum of squares (<= 630) are exact."""
    rng = np.random.RandomState(31)
    E, rows, means = 70, [], []
    for n in CM_COUNTS:
        m = rng.randint(-3, 4, size=E)
        d = rng.randint(-2, 3, size=(n, E))
        d[-1] = -d[:-1].sum(0)                        # deviations that add up to zero (n = 1: none)
        rows.append(m + d)
        means.append(m)
    return np.concatenate(rows).astype(np.float32), np.stack(means).astype(np.float32), np.concatenate([[0], np.cumsum(CM_COUNTS)])


@pytest.mark.parametrize("eps", [0.0, 1e-8])
def test_class_mean_is_bit_equal_on_exact_inputs(eps):
    emb, means, offsets = _integer_prompts()
    assert emb.shape == (93, 70) and (np.abs(means).sum(1) > 0).all()
    f = np.float32
    ss = (means * means).sum(1, dtype=f)
    want = means / (f(eps) + np.sqrt(ss))[:, None]
    assert want.dtype == f
    W = ops.zeroshot_class_mean(_padded(emb, 72), offsets, eps)
    assert tuple(W.shape) == (5, 70) and tuple(W._base.shape) == (5, 72)
    assert np.array_equal(_host(W), want)
    assert np.array_equal(_host(W._base)[:, 70:], np.zeros((5, 2), dtype=f))      # the padding columns are written, as zeros
    assert torch.equal(W, ops.zeroshot_class_mean(_dev(emb), offsets, eps))       # lde = 70: the same values
    assert np.array_equal(_host(W), Z.class_mean_fp32(emb, offsets, eps))         # and the restatement agrees


def test_class_mean_empty_class_raises():
    emb, _, _ = _integer_prompts()
    with pytest.raises(RuntimeError, match=r"Classes without embeddings: \[1\]"):
        ops.zeroshot_class_mean(_dev(emb), [0, 4, 4, 93])
    with pytest.raises(RuntimeError, match=r"Classes without embeddings: \[2\]"):
        zero_shot.class_mean_embeddings(_dev(emb[:5]), [0, 1, 1, 3, 0], 4)


# ---- 2. class mean, general ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", [0.0, 1e-8])
def test_class_mean_within_float32_noise_of_fp64(golden, eps):
    """Unit-norm rows, (C, E) = (37, 199).  Bound 4 * dev_w, dev_w = the largest |class_mean_fp32 - fp64| of the case (stored in
    the fixture): another summation order of the same length changes the realisation of the rounding error, not its scale."""
    emb, offsets = G.classmean_inputs()
    assert np.array_equal(offsets, golden["W_offsets"]) and emb.shape[1] == 199 and len(offsets) == 38
    dev_w = float(golden["W_dev"])
    W = _host(ops.zeroshot_class_mean(_dev(emb), offsets, eps))
    err = np.abs(W.astype(np.float64) - Z.class_mean_fp64(emb, offsets, eps)).max()
    same = np.array_equal(W, Z.class_mean_fp32(emb, offsets, eps))
    print(f"class_mean eps {eps}: max |W - fp64| {err:.3g} = {err / dev_w:.2f} dev_w (bound 4 dev_w = {4 * dev_w:.3g}); "
          f"bit-equal to class_mean_fp32: {same}")
    assert err <= 4 * dev_w, (err, dev_w)
    assert np.abs(np.linalg.norm(W.astype(np.float64), axis=1) - 1).max() < 1e-6
    # prompts in any order through the public entry: the stable class sort gives the same rows in the same order
    pc = np.repeat(np.arange(37), np.diff(offsets))
    perm = np.random.RandomState(2).permutation(len(pc))
    got = zero_shot.class_mean_embeddings(_dev(emb[perm]), pc[perm], 37, eps=eps)
    stable = perm[np.argsort(pc[perm], kind="stable")]
    assert np.array_equal(_host(got), _host(ops.zeroshot_class_mean(_dev(emb[stable]), offsets, eps)))


# ---- 3. ranks, exact -------------------------------------------------------------------------------------------------------
def _integer_case(B, C, E, Lmax, seed):
    """Integers in [-3, 3]: every dot product is exact in any order.  -> features, classifier, labels [B, Lmax], and the rows
    that carry each planted tie."""
    rng = np.random.RandomState(seed)
    z = rng.randint(-3, 4, size=(B, E)).astype(np.int64)
    w = rng.randint(-3, 4, size=(C, E)).astype(np.int64)
    lab = np.full((B, Lmax), -1, dtype=np.int64)
    lab[:, 0] = rng.randint(0, C, size=B)
    if Lmax > 1:
        for j in range(1, Lmax):
            extra = rng.randint(0, C, size=B)
            lab[:, j] = np.where(rng.rand(B) < 0.5, extra, -1)      # duplicates of label 0 and holes before a label included
    plant = {}
    if C >= 5:
        # a: class 1 copies class 0's row; rows whose only label is 0 tie with it
        w[1] = w[0]
        rows = np.arange(0, B, 9)
        lab[rows] = -1
        lab[rows, 0] = 0
        plant["copy of the label's row"] = rows
    if C >= 5 and Lmax >= 2:
        # b: classes 2 and 3 share a row and are both labels of these images
        w[3] = w[2]
        rows = np.arange(1, B, 9)
        lab[rows] = -1
        lab[rows, 0], lab[rows, Lmax - 1] = 3, 2
        plant["two equal labels"] = rows
    if C > 128:
        # c: a row of +-3 that beats every other class (v . v = 9 E), in class tiles 0 and 1 (and 2 when there is one)
        v = 3 * (2 * rng.randint(0, 2, size=E) - 1)
        twins = (129, 7) if C < 257 else (256, 129, 7)
        w[list(twins)] = v
        rows = np.arange(2, B, 9)
        z[rows] = v
        plant["maximum in several class tiles"] = rows
    # d: no label at all
    rows = np.arange(3, B, 9) if B > 3 else np.arange(0)
    lab[rows] = -1
    plant["no label"] = rows
    return z, w, lab, plant


@pytest.mark.parametrize("B,C,E,Lmax,ld", [(1, 1, 8, 1, 8), (127, 5, 71, 1, 72), (129, 130, 40, 3, 40), (200, 257, 130, 3, 132)])
def test_ranks_equal_int64_numpy_with_planted_ties(B, C, E, Lmax, ld):
    z, w, lab, plant = _integer_case(B, C, E, Lmax, seed=B + C)
    logits = z @ w.T
    gt, eq, pred = Z.ranks_from_logits(logits, lab)
    # the plants are what they claim to be
    if "copy of the label's row" in plant:
        rows = plant["copy of the label's row"]
        assert (eq[rows] >= 1).all() and (logits[rows, 1] == logits[rows, 0]).all()
        assert (gt[rows] == (logits[rows] > logits[rows, :1]).sum(1)).all()      # the copy is in eq, not in gt
    if "two equal labels" in plant:
        rows = plant["two equal labels"]
        assert (logits[rows, 2] == logits[rows, 3]).all()
        others = np.delete(logits[rows], [2, 3], axis=1)
        assert (gt[rows] == (others > logits[rows, 2:3]).sum(1)).all() and (eq[rows] == (others == logits[rows, 2:3]).sum(1)).all()
    if "maximum in several class tiles" in plant:
        rows = plant["maximum in several class tiles"]
        assert (pred[rows] == 7).all() and (logits[rows, 129] == logits[rows, 7]).all() and (logits[rows].max(1) == 9 * E).all()
    rows = plant["no label"]
    assert (gt[rows] == C).all() and (eq[rows] == 0).all()
    assert B < 4 or len(rows) > 0
    got = ops.zeroshot_ranks(_padded(z, ld), _padded(w, ld), _dev(lab, torch.int32))
    again = ops.zeroshot_ranks(_padded(z, ld), _padded(w, ld), _dev(lab, torch.int32))
    for name, g, a, want in zip(("gt", "eq", "pred"), got, again, (gt, eq, pred)):
        assert g.dtype == torch.int32 and tuple(g.shape) == (B,) and torch.equal(g, a), name
        bad = np.nonzero(_host(g) != want)[0]
        assert len(bad) == 0, (name, bad[:10], _host(g)[bad[:10]], want[bad[:10]], lab[bad[:10]])
    # the public entry on the same data: any integer dtype, the same ranks, counts by the rule gt < min(k, C)
    out = zero_shot.zero_shot_ranks(_dev(z), _dev(w), _dev(lab, torch.int64))
    assert all(torch.equal(out[k], g) for k, g in zip(("gt", "eq", "pred"), got))
    counts = zero_shot.zero_shot_counts(_dev(z), _dev(w), _dev(lab, torch.int16), topk=(1, 5))
    assert counts == Z.counts_from_ranks(gt, eq, C, (1, 5))


def test_three_classes_with_top5():
    """C = 3 with top-5: k is clipped to C as `run` clips it, so an image without labels is still no hit."""
    z, w, lab, _ = _integer_case(40, 3, 16, 2, seed=5)
    lab[:6] = -1
    gt, eq, _ = Z.ranks_from_logits(z @ w.T, lab)
    got = zero_shot.zero_shot_metrics(_dev(z), _dev(w), lab, topk=(1, 5))
    want = Z.counts_from_ranks(gt, eq, 3, (1, 5))
    assert {k: got[k] for k in want} == want and got["hits5"] == int((lab >= 0).any(1).sum()) <= 34
    assert type(got["top5"]) is np.float64 and got["top5"] == np.float64(got["hits5"]) / np.float64(40)
    single = lab[:, 0].copy()
    single[single < 0] = 0
    want = Z.accuracy_torch_reference(torch.from_numpy((z @ w.T).astype(np.float64)), torch.from_numpy(single), topk=(3,))
    assert zero_shot.zero_shot_counts(_dev(z), _dev(w), single, topk=(5,))["hits5"] == want[0] == 40


# ---- 4. views --------------------------------------------------------------------------------------------------------------
def test_ranks_on_column_slices_of_wider_matrices():
    g = torch.Generator(device=DEV).manual_seed(4)
    big_f, big_w = torch.randn(300, 96, device=DEV, generator=g), torch.randn(140, 64, device=DEV, generator=g)
    f, w = big_f[:, 8:48], big_w[:, 4:44]                  # ld 96 / 64 > E = 40, offsets of 32 and 16 bytes
    assert f.data_ptr() % 16 == 0 and w.data_ptr() % 16 == 0 and f.stride(0) == 96 and w.stride(0) == 64
    lab = torch.randint(0, 140, (300, 2), device=DEV, generator=g)
    want = ops.zeroshot_ranks(f.contiguous(), w.contiguous(), lab.int())
    got = ops.zeroshot_ranks(f, w, lab.int())
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    out = zero_shot.zero_shot_ranks(f, w, lab)
    assert all(torch.equal(out[k], b) for k, b in zip(("gt", "eq", "pred"), want))
    # a misaligned slice is copied by the wrapper: still the same ranks
    got = ops.zeroshot_ranks(big_f[:, 7:47], big_w[:, 3:43], lab.int())
    want = ops.zeroshot_ranks(big_f[:, 7:47].contiguous(), big_w[:, 3:43].contiguous(), lab.int())
    assert all(torch.equal(a, b) for a, b in zip(got, want))


# ---- 5. fixture ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["S", "M", "L"])
def test_fixture_ranks_on_every_row_and_counts(golden, name):
    z = golden
    f, w, lab = G.case_inputs(name, z[f"{name}_redraws"])
    out = zero_shot.zero_shot_ranks(_dev(f), _dev(w), lab)
    for key in ("gt", "eq", "pred"):
        bad = np.nonzero(_host(out[key]) != z[f"{name}_{key}"])[0]
        assert len(bad) == 0, (key, bad[:10], _host(out[key])[bad[:10]], z[f"{name}_{key}"][bad[:10]])
    met = zero_shot.zero_shot_metrics(_dev(f), _dev(w), _dev(lab, torch.int64))
    want = {k: int(z[f"{name}_{k}"]) for k in ("count", "ties", "hits1", "hits5")}
    assert {k: met[k] for k in want} == want and all(type(met[k]) is int for k in want)
    assert type(met["top1"]) is np.float64 and met["top1"] == float(z[f"{name}_top1"]) and met["top5"] == float(z[f"{name}_top5"])


# ---- 6. memory -------------------------------------------------------------------------------------------------------------
def test_no_logit_matrix_is_allocated():
    """B = C = 8192, E = 32: the [B, C] fp32 logits alone would be 256 MiB; the call may add less than 16 MiB to the peak."""
    g = torch.Generator(device=DEV).manual_seed(6)
    f = torch.nn.functional.normalize(torch.randn(8192, 32, device=DEV, generator=g), dim=1)
    w = torch.nn.functional.normalize(torch.randn(8192, 32, device=DEV, generator=g), dim=1)
    lab = torch.randint(0, 8192, (8192,), device=DEV, generator=g)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    met = zero_shot.zero_shot_metrics(f, w, lab)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print(f"peak memory rise {rise / 2 ** 20:.2f} MiB")
    assert rise < 16 * 2 ** 20, rise
    assert met["count"] == 8192 and 0 <= met["hits1"] <= met["hits5"] < 8192


# ---- 7. zero-sized inputs --------------------------------------------------------------------------------------------------
def test_zero_sized_inputs_launch_nothing():
    from clipa_amd import lib
    f, w = torch.ones(4, 8, device=DEV), torch.ones(3, 8, device=DEV)
    got = ops.zeroshot_ranks(f[:0], w, torch.zeros((0, 2), device=DEV, dtype=torch.int32))
    assert all(tuple(t.shape) == (0,) and t.dtype == torch.int32 for t in got)
    out = zero_shot.zero_shot_ranks(f[:0], w, torch.zeros(0, dtype=torch.int64))
    assert sorted(out) == ["eq", "gt", "pred"] and all(tuple(t.shape) == (0,) for t in out.values())
    met = zero_shot.zero_shot_metrics(f[:0], w, np.zeros(0, dtype=np.int64))
    assert met["count"] == 0 and met["hits1"] == 0 and met["ties"] == 0 and math.isnan(met["top1"])
    # the C entries: B = 0 and C = 0 return before any pointer is looked at
    lib.call("clipa_zeroshot_ranks", None, None, None, 0, 3, 8, 1, 8, 8, None, None, None, ops._stream())
    lib.call("clipa_zeroshot_class_mean", None, None, 0, 0, 8, 8, 0.0, None, 8, ops._stream())
    assert tuple(ops.zeroshot_class_mean(f[:0], [0]).shape) == (0, 8)


# ---- 8. build_classifier and evaluate_zero_shot on a stand-in model --------------------------------------------------------
class StandIn(torch.nn.Module):
    """Returns planted features: token row n holds the prompt's index in column 0, an "image" is its row index."""

    def __init__(self, prompt_emb, image_feat):
        super().__init__()
        self.prompt_emb, self.image_feat = prompt_emb, image_feat
        self.text_calls, self.image_calls = [], []

    def encode_text(self, tokens, normalize=False):
        self.text_calls.append((tokens.shape[0], normalize, self.training, torch.is_grad_enabled()))
        return self.prompt_emb[tokens[:, 0]]

    def encode_image(self, images, normalize=False):
        self.image_calls.append((images.shape[0], normalize, self.training, torch.is_grad_enabled()))
        return self.image_feat[images]


def test_build_classifier_and_evaluate_on_a_recording_model(golden):
    f, w, lab = G.case_inputs("S", golden["S_redraws"])
    emb, offsets = G.classmean_inputs()                       # 37 classes, like case S; E = 199 against 71: two models' worth
    emb = np.ascontiguousarray(emb[:, :71])
    emb /= np.linalg.norm(emb, axis=1, keepdims=True)
    pc = np.repeat(np.arange(37), np.diff(offsets))
    perm = np.random.RandomState(12).permutation(len(pc))
    m = StandIn(_dev(emb), _dev(f))
    m.train()
    tokens = torch.zeros((len(pc), 16), device=DEV, dtype=torch.int64)
    tokens[:, 0] = _dev(perm, torch.int64)                    # prompt n of the caller is planted row perm[n]
    clf = zero_shot.build_classifier(m, tokens, pc[perm], 37, text_batch_size=64, eps=1e-8)
    n_calls = math.ceil(len(pc) / 64)
    assert n_calls == 4 and m.text_calls == [(64, True, False, False)] * 3 + [(len(pc) - 192, True, False, False)]
    assert m.training                                         # the mode is put back
    assert clf.dtype == torch.float32 and tuple(clf.shape) == (37, 71)
    stable = perm[np.argsort(pc[perm], kind="stable")]
    assert np.array_equal(_host(clf), _host(ops.zeroshot_class_mean(_dev(emb[stable]), offsets, 1e-8)))
    # prompt order does not matter beyond float32 noise, and the sorted order needs no gather
    m.text_calls.clear()
    tokens[:, 0] = torch.arange(len(pc), device=DEV)
    clf_sorted = zero_shot.build_classifier(m, tokens, torch.from_numpy(pc), 37, text_batch_size=1024, eps=1e-8)
    assert len(m.text_calls) == 1 and np.abs(_host(clf_sorted) - _host(clf)).max() <= 4 * float(golden["W_dev"])
    assert np.array_equal(_host(clf_sorted), Z.class_mean_fp32(emb, offsets, 1e-8))
    m.eval()
    zero_shot.build_classifier(m, tokens, pc, 37)
    assert not m.training

    # evaluate: two datasets over the planted features, with the fixture's classifier
    wd = _dev(w)
    idx = torch.arange(300, device=DEV)
    multi = np.stack([lab, np.where(np.arange(300) % 2 == 0, (lab + 1) % 37, -1)], axis=1)
    sets = {"imagenet-zeroshot-val": iter([(idx[:128], _dev(lab[:128], torch.int64)), (idx[128:130], _dev(lab[128:130], torch.int32)),
                                           (idx[130:], _dev(lab[130:], torch.int64))]),
            "real": [(idx[:150], _dev(multi[:150], torch.int64)), (idx[150:], _dev(multi[150:], torch.int64))]}
    m.train()
    res = zero_shot.evaluate_zero_shot(m, wd, sets, topk=(1, 5))
    assert m.training
    assert m.image_calls == [(128, True, False, False), (2, True, False, False), (170, True, False, False),
                             (150, True, False, False), (150, True, False, False)]
    assert list(res) == ["imagenet-zeroshot-val-top1", "imagenet-zeroshot-val-top5", "imagenet-zeroshot-val-count", "real-top1",
                         "real-top5", "real-count"]
    assert all(type(res[k]) is np.float64 for k in res if "top" in k) and all(type(res[k]) is int for k in res if "count" in k)
    one = zero_shot.zero_shot_metrics(_dev(f), wd, lab)
    assert res["imagenet-zeroshot-val-top1"] == one["top1"] == float(golden["S_top1"])
    assert res["imagenet-zeroshot-val-top5"] == one["top5"] == float(golden["S_top5"]) and res["imagenet-zeroshot-val-count"] == 300
    two = zero_shot.zero_shot_metrics(_dev(f), wd, multi)
    assert res["real-top1"] == two["top1"] >= one["top1"] and res["real-top5"] == two["top5"] and res["real-count"] == 300
    # a label outside [-1, C) in any batch is an error, found at the dataset's one sync
    with pytest.raises(RuntimeError, match=r"evaluate_zero_shot \(bad\): 1 labels values outside"):
        zero_shot.evaluate_zero_shot(m, wd, {"bad": [(idx[:4], torch.tensor([0, 1, 37, 2], device=DEV))]})
    assert m.training


# ---- 9. on a toy engine model ----------------------------------------------------------------------------------------------
def _toy_prompts(C, T, ctx, vocab):
    """Class prompts that a random text tower tells apart: class-specific token ids, the end-of-text token (the largest id, where
    the tower pools) at a class-specific position.  Random token rows give class embeddings too alike for the margin condition."""
    toks = torch.zeros((C * T, ctx), dtype=torch.int64)
    for c in range(C):
        for t in range(T):
            toks[c * T + t, :] = 1 + c * 40 + t
            toks[c * T + t, 1::2] = 1 + c * 40 + 20 + t
            toks[c * T + t, -1 - (c % 5)] = vocab - 1
    return toks


def _toy_images(B, size, seed):
    """uint8 images of one colour gradient each: a random vision tower maps noise images to nearly one feature vector."""
    rng = np.random.RandomState(seed)
    base = rng.randint(0, 256, size=(B, 3, 1, 1))
    gx = rng.randint(-4, 5, size=(B, 3, 1, 1)) * np.arange(size).reshape(1, 1, 1, size)
    gy = rng.randint(-4, 5, size=(B, 3, 1, 1)) * np.arange(size).reshape(1, 1, size, 1)
    return torch.from_numpy(np.clip(base + gx + gy, 0, 255).astype(np.uint8))


def test_evaluate_zero_shot_on_an_engine_model():
    """Real towers.  The recorded features (what encode_image / encode_text returned) go through ranks_fp64 on the host; outside
    the 64 * dev margin the engine's ranks are those, and the evaluator's counts differ from the fp64 ones by at most the rows
    inside the margin - of which there may be at most 2 %.  (Checked when this test was written, with the fp32 oracle towers
    and with their features perturbed by 1 % thirty times: no row inside the margin.)"""
    g = load_golden("cls_erf")
    m = clipa_amd.CLIP(**g.cfg, output_dict=True)
    m.load_state_dict(g.sd, strict=True)
    m.to(DEV).train()
    ctx, vocab = g.cfg["text_cfg"]["context_length"], g.cfg["text_cfg"]["vocab_size"]
    size = g.cfg["vision_cfg"]["image_size"]
    C, T, B = 11, 3, 96
    toks, images = _toy_prompts(C, T, ctx, vocab), _toy_images(B, size, seed=17).to(DEV)
    pc = np.repeat(np.arange(C), T)
    perm = np.random.RandomState(1).permutation(C * T)
    rng = np.random.RandomState(2)
    lab = np.stack([rng.randint(0, C, size=B), np.where(rng.rand(B) < 0.3, rng.randint(0, C, size=B), -1)], axis=1)
    rec = {"text": [], "image": []}
    enc_t, enc_i = m.encode_text, m.encode_image
    m.encode_text = lambda *a, **k: (rec["text"].append(enc_t(*a, **k)), rec["text"][-1])[1]
    m.encode_image = lambda *a, **k: (rec["image"].append(enc_i(*a, **k)), rec["image"][-1])[1]
    try:
        clf = zero_shot.build_classifier(m, toks[perm].to(DEV), pc[perm], C, text_batch_size=16)
        res = zero_shot.evaluate_zero_shot(m, clf, {"toy": [(images[:50], _dev(lab[:50], torch.int64)),
                                                            (images[50:], _dev(lab[50:], torch.int64))]}, topk=(1, 5))
    finally:
        m.encode_text, m.encode_image = enc_t, enc_i
    assert m.training and [len(t) for t in rec["text"]] == [16, 16, 1] and [len(t) for t in rec["image"]] == [50, 46]
    emb = _host(torch.cat(rec["text"]).float())
    feat = _host(torch.cat(rec["image"]).float())
    assert np.abs(np.linalg.norm(emb, axis=1) - 1).max() < 1e-5 and np.abs(np.linalg.norm(feat, axis=1) - 1).max() < 1e-5
    # the classifier is the class mean of the recorded prompt embeddings
    order = np.argsort(pc[perm], kind="stable")
    offsets = np.arange(0, C * T + 1, T)
    w64 = Z.class_mean_fp64(emb[order], offsets, 0.0)
    w = _host(clf)
    assert np.abs(w - w64).max() <= 4 * np.abs(Z.class_mean_fp32(emb[order], offsets, 0.0) - w64).max() + 1e-12
    # ranks of the recorded features against that classifier
    v = Z.logits_fp64(feat, w)
    dev = np.abs(Z.chain_fp32(feat, w).astype(np.float64) - v).max()
    gt, eq, pred = Z.ranks_from_logits(v, lab)
    mask = Z.label_mask(lab, C)
    t = np.where(mask, v, -np.inf).max(axis=1)
    near = np.where(mask, np.inf, np.abs(v - t[:, None])).min(axis=1)
    top2 = np.sort(v, axis=1)[:, -2:]
    inside = np.minimum(near, top2[:, 1] - top2[:, 0]) < 64 * dev
    print(f"toy model: dev {dev:.3g}, rows inside the 64 dev margin {int(inside.sum())} of {B}, fp64 top-1 {(gt == 0).mean():.3f}")
    assert inside.sum() <= 0.02 * B
    out = zero_shot.zero_shot_ranks(_dev(feat), clf, lab)
    for key, want in (("gt", gt), ("eq", eq), ("pred", pred)):
        assert np.array_equal(_host(out[key])[~inside], want[~inside]), key
    assert res["toy-count"] == B and type(res["toy-top1"]) is np.float64
    for k in (1, 5):
        sure = int((gt[~inside] < k).sum())
        assert sure <= round(res[f"toy-top{k}"] * B) <= sure + int(inside.sum())
